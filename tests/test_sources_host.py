"""Host-side checks of the moving point sources (no GPU): the position-file parser, nframes, the oracle's literal loops against its
vectorised forms (tests/sources_oracle.py), and known answers of the definitions in include/sagen.h."""
import numpy as np
import pytest

import render_oracle as RO
import sources_oracle as SO

RATE = 48000


def _sig(n, seed):
    return np.random.RandomState(seed).normal(size=n).astype(np.float32).astype(np.float64)


def test_position_file_round_trip_header_form(tmp_path):
    from spatialaudiogen_amd.sources import read_position_file
    pts = {'dog': np.array([[0.5, -0.25, 1.5], [-3.0, 0.1, 2.0]]), 'rain': np.zeros((0, 3)), 'cat': np.array([[1e-3, 1.25, 0.0]])}
    fn = str(tmp_path / 'pos.txt')
    with open(fn, 'w') as f:
        f.write('<BGI>beach.jpg<BGI>.\n')
        f.write('dog dog.wav dog.png 2\n0.5 -0.25 1.5\n-3.0 0.1 2.0\n')
        f.write('rain rain.wav 0\n')
        f.write('cat audio/cat.wav 1\n%r %r %r\n' % (1e-3, 1.25, 0.0))
        f.write('\nignored after.wav 0\n')                                  # reading stops at the first empty line
    ids, points, wavs, imgs, bg = read_position_file(fn)
    assert ids == ['dog', 'rain', 'cat'] and bg == 'beach.jpg'
    assert wavs == {'dog': 'dog.wav', 'rain': 'rain.wav', 'cat': 'audio/cat.wav'} and imgs == {'dog': 'dog.png'}
    for k in ids:
        assert points[k].shape == pts[k].shape and points[k].dtype == np.float64 and np.array_equal(points[k], pts[k])
    with open(fn, 'w') as f:
        f.write('dog dog.wav 2\n0.5 -0.25 1.5\n')
    with pytest.raises(ValueError):
        read_position_file(fn)


def test_position_file_plain_form(tmp_path):
    from spatialaudiogen_amd.sources import read_position_file
    cp = np.array([[3.0, 0.2, 2.0], [-3.0, -0.4, 1.2], [0.1, 0.0, 0.7]])
    fn = str(tmp_path / 'plain.txt')
    with open(fn, 'w') as f:
        for p in cp:
            f.write('%r %r %r\n' % tuple(float(v) for v in p))
    ids, points, wavs, imgs, bg = read_position_file(fn)
    assert ids == ['source'] and wavs == {} and imgs == {} and bg is None and np.array_equal(points['source'], cp)


def test_nframes_is_int_of_duration_times_rate():
    """position.py:78-82: duration = N / float(rate), nframes = int(duration * rate) - which is N - 1 for some N."""
    short = [n for n in range(1, 60000) if SO.nframes_of(n, RATE) != n]
    assert short and all(SO.nframes_of(n, RATE) == n - 1 for n in short)
    for n in (4801, 11999, 12000, 12001, 52799, short[0]):
        assert SO.nframes_of(n, RATE) == int((n / float(RATE)) * RATE)


def test_trajectory_index_is_floor_of_linspace():
    """idx of the definition equals numpy's floor(linspace(0, P - 1, nframes)) (position.py:85), and the product's host trajectory
    (sources.trajectory, used for the radius check) equals the oracle's."""
    from spatialaudiogen_amd.sources import trajectory
    cp = np.array([[-1.0, 0.3, 1.0], [0.5, 1.8, 0.8], [1.2, 0.5, 0.0], [np.pi / 2, 0.0, 0.12], [2.5, -0.6, 1.4]])
    for n in (4801, 11999, 12000, 12001):
        nf = SO.nframes_of(n, RATE)
        want = np.floor(np.linspace(0, 4, nf)).astype(int)
        i = np.arange(nf)
        got = np.where(i == nf - 1, 4, np.floor(i * (4 / float(nf - 1))).astype(int))
        assert np.array_equal(got, want)
        pol = SO.track(cp, n, RATE, i)[0]
        assert np.array_equal(trajectory(cp, n, RATE, i), pol)
        for k in (0, 1, nf // 4, nf // 4 + 1, nf // 2, nf - 2, nf - 1):
            assert np.allclose(pol[k], SO.tic(cp, n, RATE, k), rtol=0, atol=1e-15)


def test_loops_equal_the_vectorised_forms():
    cps = [np.array([[0.7, -0.3, 1.5]]), np.array([[3.0, 0.2, 2.0], [-3.0, -0.4, 1.2]]),
           np.array([[-1.0, 0.3, 1.0], [0.5, 1.8, 0.8], [1.2, 0.5, 0.0], [np.pi / 2, 0.0, 0.12], [2.5, -0.6, 1.4]])]
    far = cps[:2] + [cps[2] + np.array([0., 0., 0.6])]
    sig = [_sig(700, 1), _sig(701, 2), _sig(699, 3)]
    n = min(SO.nframes_of(len(s), RATE) for s in sig)
    for order in (1, 2):
        assert np.allclose(SO.encode_loop(sig, cps, RATE, order, 0, n), SO.encode(sig, cps, RATE, order, 0, n), rtol=0, atol=1e-12)
    assert np.allclose(SO.encode_loop(sig, far, RATE, 2, 3, n - 3, True, 0.5), SO.encode(sig, far, RATE, 2, 3, n - 3, True, 0.5), rtol=0, atol=1e-12)
    assert np.allclose(SO.mic_loop(sig, cps, RATE, 0, n), SO.mic(sig, cps, RATE, 0, n), rtol=0, atol=1e-12)
    dirs, left, right = RO.make_hrirs(41, ntaps=24)
    for zb in (0, 23):
        assert np.allclose(SO.hrir_loop(sig, cps, RATE, dirs, left, right, zb, 5, 300), SO.hrir(sig, cps, RATE, dirs, left, right, zb, 5, 300), rtol=0, atol=1e-12)


def test_static_source_at_plus_x():
    s = _sig(480, 4)
    n = SO.nframes_of(480, RATE)
    for order in (1, 2):
        a = SO.encode_loop([s], [np.array([[0., 0., 2.]])], RATE, order, 0, n)
        assert np.array_equal(a[:, 0], s[:n]) and np.array_equal(a[:, 3], s[:n]) and not a[:, 1:3].any()


def test_static_encode_equals_the_plane_wave():
    s = _sig(480, 5)
    n = SO.nframes_of(480, RATE)
    for order in (1, 2):
        a = SO.encode([s], [np.array([[0.7, -0.3, 1.7]])], RATE, order, 0, n)
        assert np.allclose(a, RO.plane_wave(order, 0.7, -0.3, s[:n]), rtol=0, atol=1e-14)


def test_mic_left_ear_leads_for_a_source_at_plus_y():
    """A source at (0, 2, 0): the left ear (0, 0.1, 0) is 1.9 m away, the right 2.1 m: delays int(1.9 / 343 * 48000) = 265 and
    int(2.1 / 343 * 48000) = 293, gains 1 / 2.9 and 1 / 3.1."""
    s = _sig(1000, 6)
    n = SO.nframes_of(1000, RATE)
    y = SO.mic_loop([s], [np.array([[np.pi / 2, 0., 2.]])], RATE, 0, n)
    dl, dr = int(1.9 / 343. * RATE), int(2.1 / 343. * RATE)
    assert (dl, dr) == (265, 293)
    assert not y[:dl, 0].any() and not y[:dr, 1].any()
    assert np.allclose(y[dl:, 0], s[:n - dl] / 2.9, rtol=0, atol=1e-14) and np.allclose(y[dr:, 1], s[:n - dr] / 3.1, rtol=0, atol=1e-14)


def test_zero_and_negative_radius_rules():
    assert np.array_equal(SO.unit(2.0, 1.0, 0.), [1., 0., 0.])
    assert np.allclose(SO.unit(0.4, -0.2, -1.5), -SO.unit(0.4, -0.2, 1.5), rtol=0, atol=0)
    cp = np.array([[0.4, -0.2, 1.0], [0.4, -0.2, -1.0]])              # r runs through zero: the direction flips, the path does not wrap
    pol, u = SO.track(cp, 4801, RATE, np.arange(SO.nframes_of(4801, RATE)))
    assert (pol[:, 2] > 0).any() and (pol[:, 2] < 0).any()
    assert np.allclose(u[pol[:, 2] > 0], SO.unit(0.4, -0.2, 1.), rtol=0, atol=1e-15) and np.allclose(u[pol[:, 2] < 0], -SO.unit(0.4, -0.2, 1.), rtol=0, atol=1e-15)
    # the cartesian position is |r| u: set_polar(-r) and set_polar(r) at the antipode are the same place
    s = _sig(600, 7)
    n = SO.nframes_of(600, RATE)
    a = SO.mic_loop([s], [np.array([[0.4, -0.2, -1.5]])], RATE, 0, n)
    b = SO.mic_loop([s], [np.array([[0.4 + np.pi, 0.2, 1.5]])], RATE, 0, n)
    assert np.allclose(a, b, rtol=0, atol=1e-14)
