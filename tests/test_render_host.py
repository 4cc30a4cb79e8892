"""The host side of the renderings (no device): harmonics, rotations, decoders, the HRIR set and its tie rule, every builder's taps
against the fp64 oracle's long form (tests/render_oracle.py), the entry's argument checks by return code, and both command lines'
parsing and refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import render_oracle as RO
from spatialaudiogen_amd import ambisonics as A
from spatialaudiogen_amd import render as R
from spatialaudiogen_amd import feeder


def _dirs(seed, n):
    d = np.random.RandomState(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.mark.parametrize('order', [1, 2])
def test_closed_form_harmonics_match_the_lpmv_formula(order):
    phi, nu = A.to_polar(_dirs(1, 200))
    got = A.sh_matrix_at(phi, nu, order)
    assert got.shape == (200, (order + 1) ** 2)
    assert np.abs(got - RO.sh_lpmv(phi, nu, order)).max() <= 1e-14
    np.testing.assert_array_equal(A.sh_matrix_at(phi, nu, 1), A.sh_order1(phi, nu))          # the existing order-1 function is a prefix
    with pytest.raises(ValueError):
        A.sh_matrix_at(phi, nu, 3)


@pytest.mark.parametrize('order', [1, 2])
def test_rotation_matrix_defining_property(order):
    r = np.random.RandomState(2)
    d = _dirs(3, 136)
    for _ in range(8):
        yaw, pitch, roll = r.uniform(-np.pi, np.pi, 3)
        M = A.rotation_matrix(order, yaw, pitch, roll)
        rot = RO.rot3(yaw, pitch, roll)
        assert np.abs(RO.sh_lpmv(*RO.polar(d @ rot.T), order=order) - RO.sh_lpmv(*RO.polar(d), order=order) @ M.T).max() <= 1e-12
        # a listener turning their head hears the inverse
        assert np.abs(A.head_rotation_matrix(order, yaw, pitch, roll) @ M - np.eye(M.shape[0])).max() <= 1e-12


@pytest.mark.parametrize('order', [1, 2])
def test_rotation_matrix_composition_identity_and_yaw(order):
    n = (order + 1) ** 2
    assert np.abs(A.rotation_matrix(order, 0., 0., 0.) - np.eye(n)).max() <= 1e-12
    a, b = (0.7, -0.4, 1.9), (-2.1, 0.3, 0.5)
    ab = RO.rot3(*a) @ RO.rot3(*b)
    assert np.abs(A.rotation_matrix(order, *a) @ A.rotation_matrix(order, *b) - A.sh_rotation(order, ab)).max() <= 1e-12
    assert np.abs(A.rotation_matrix(order, 0.3) @ A.rotation_matrix(order, 0.9) - A.rotation_matrix(order, 1.2)).max() <= 1e-12
    for yaw in (0.7, -2.5, np.pi / 2):
        assert np.abs(A.rotation_matrix(order, yaw)[:4, :4] - feeder.rotation_matrix_z(yaw)).max() <= 1e-12
    # a source at azimuth phi moves to phi + yaw
    x = RO.sh_lpmv(0.4, 0.2, order)
    assert np.abs(A.rotation_matrix(order, 0.5) @ x - RO.sh_lpmv(0.9, 0.2, order)).max() <= 1e-12


def test_rotation_xyz_is_rz_ry_rx():
    assert np.abs(A.rotation_xyz(0.3, -1.1, 2.0) - RO.rot3(0.3, -1.1, 2.0)).max() <= 1e-15
    assert np.allclose(A.rotation_xyz(np.pi / 2) @ [1, 0, 0], [0, 1, 0])                  # yaw turns front to left
    assert np.allclose(A.rotation_xyz(0, np.pi / 2) @ [1, 0, 0], [0, 0, -1])              # right-handed about y
    assert np.allclose(A.rotation_xyz(0, 0, np.pi / 2) @ [0, 1, 0], [0, 0, 1])


@pytest.mark.parametrize('order', [1, 2])
def test_decode_matrix_both_methods(order):
    pos = _dirs(5, 14) * 2.5
    Y = RO.sh_lpmv(*RO.polar(pos), order=order)
    assert np.abs(A.decode_matrix(pos, order, 'projection') - Y).max() <= 1e-14
    D = A.decode_matrix(pos, order, 'pseudoinv')
    assert D.shape == Y.shape and np.abs(D - np.linalg.pinv(Y).T).max() <= 1e-13
    ambi = np.random.RandomState(6).normal(size=(50, Y.shape[1]))
    for method in ('projection', 'pseudoinv'):
        assert np.abs(ambi @ A.decode_matrix(pos, order, method).T - RO.decode(ambi, pos, order, method)).max() <= 1e-12
    with pytest.raises(ValueError):
        A.decode_matrix(pos, order, 'allrad')
    assert np.abs(A.ring_positions(order) - RO.ring(order)).max() <= 1e-15 and len(A.ring_positions(order)) == 2 * (order + 1) ** 2


def test_cipic_dir_round_trip_and_tie_rule(tmp_path):
    dirs, left, right = RO.make_hrirs(11)
    RO.write_cipic_dir(str(tmp_path / 'hrir'), left, right, 48000)
    assert sorted(os.listdir(str(tmp_path / 'hrir')))[:2] == ['0azleft.wav', '0azright.wav'] and len(os.listdir(str(tmp_path / 'hrir'))) == 46
    assert os.path.exists(str(tmp_path / 'hrir' / 'neg80azleft.wav'))
    h = R.HrirSet.from_cipic_dir(str(tmp_path / 'hrir'))
    assert h.rate == 48000 and h.ntaps == 200 and h.left.shape == (23 * 50, 200)
    np.testing.assert_array_equal(h.left, left)                        # sample order of a file = time order of the response
    np.testing.assert_array_equal(h.right, right)
    assert np.abs(h.directions - dirs).max() <= 1e-15
    for d in _dirs(12, 50):
        assert h.closest(3. * d) == int(np.argmax(dirs @ d))
    # the reference's rings have EXACT ties.  Order 1 (S = 8): the speakers on the interaural axis are equally close to
    # (az = -+80, el = 0) and (az = +-80, el = 180).  Order 2 (S = 18, 20 degrees apart): the speakers at +-40, +-60, +-120, +-140
    # degrees lie half way between two azimuths of the set.  The lowest index (azimuth-major, elevation-minor) wins.
    ne = len(RO.ELEVATIONS)
    idx = lambda az, el: RO.AZIMUTHS.index(az) * ne + RO.ELEVATIONS.index(el)
    n_ties = {1: 0, 2: 0}
    for order in (1, 2):
        for spk in RO.ring(order):
            dots = dirs @ spk
            cand = np.flatnonzero(dots >= dots.max() - 1e-12)
            n_ties[order] += len(cand) > 1
            assert h.closest(spk) == cand[0] == cand.min()
    assert n_ties[1] == 2 and n_ties[2] == 8
    ring = RO.ring(1)
    left_spk, right_spk = ring[6], ring[2]                             # phi = +pi/2 (y = +1) and -pi/2
    assert abs(left_spk[1] - 1) < 1e-15 and abs(right_spk[1] + 1) < 1e-15
    dl = dirs @ left_spk
    assert abs(dl[idx(-80, 0)] - dl[idx(80, 180)]) <= 1e-12 and dl[idx(-80, 0)] >= dl.max() - 1e-12
    assert h.closest(left_spk) == idx(-80, 0) < idx(80, 180)
    dr = dirs @ right_spk
    assert abs(dr[idx(80, 0)] - dr[idx(-80, 180)]) <= 1e-12 and dr[idx(80, 0)] >= dr.max() - 1e-12
    assert h.closest(right_spk) == idx(-80, 180) < idx(80, 0)
    spk60 = RO.ring(2)[12]                                             # phi = +60 degrees: between az = -65 and az = -55 at el = 0
    assert abs(np.arctan2(spk60[1], spk60[0]) - np.pi / 3) < 1e-12 and h.closest(spk60) == idx(-65, 0)
    with pytest.raises(IOError):
        R.HrirSet.from_cipic_dir(str(tmp_path / 'missing'))


def _apply(taps, x, zero_before):
    y = np.zeros((x.shape[0], taps.shape[0]))
    for o in range(taps.shape[0]):
        for c in range(x.shape[1]):
            y[:, o] += np.convolve(x[:, c], taps[o, c])[:x.shape[0]]
    y[:zero_before] = 0.
    return y


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('mode', ['wy', 'ears', 'speakers', 'mic', 'hrir'])
def test_builders_match_the_oracles_long_form(mode, order):
    if mode == 'wy' and order == 2:
        with pytest.raises(ValueError):
            R.build_taps('wy', 2)
        return
    n_ch = (order + 1) ** 2
    x = np.random.RandomState(20 + order).normal(size=(2000, n_ch))
    dirs, left, right = RO.make_hrirs(13)
    hset = R.HrirSet(dirs, left, right, 48000)
    for decode in ((None, 'projection', 'pseudoinv') if mode in ('ears', 'speakers') else (None,)):
        taps, zb = R.build_taps(mode, order, 48000, hrir=hset if mode == 'hrir' else None, decode=decode)
        ref = RO.render(mode, x, order, 48000, hrirs=(dirs, left, right), decode_method=decode)
        assert taps.shape[1] == n_ch and taps.shape[0] == ref.shape[1]
        got = _apply(taps, x, zb)
        assert np.abs(got - ref).max() <= 1e-12 * max(1., np.abs(ref).max()), (mode, order, decode)
    if mode == 'mic':
        assert taps.shape == (2, n_ch, 154)                        # delays 125 .. 153 samples at 48 kHz
        if order == 1:                                             # (the ear-side speaker of the 8-ring is 0.9 m away: int(0.9 / 343 * 48000))
            assert min(int(np.flatnonzero(np.abs(taps[e]).sum(0))[0]) for e in range(2)) == 125
    if mode == 'hrir':
        assert zb == 199 and taps.shape == (2, n_ch, 200)
        with pytest.raises(ValueError, match='44100'):
            R.build_taps('hrir', order, 44100, hrir=hset)
        with pytest.raises(ValueError):
            R.build_taps('hrir', order, 48000)
    if mode == 'speakers':
        pos = _dirs(30, 7)
        t2, _ = R.build_taps('speakers', order, positions=pos, decode='pseudoinv')
        assert np.abs(_apply(t2, x, 0) - RO.render_speakers(x, order, pos, 'pseudoinv')).max() <= 1e-12


def test_head_trajectory_is_the_inverse_field_rotation():
    tr = R.head_trajectory(2, [0., 30., 90.], [0., 10., 0.], [0., 0., -20.])
    assert tr.shape == (3, 9, 9) and np.abs(tr[0] - np.eye(9)).max() <= 1e-12
    assert np.abs(tr[1] - RO.head_rotation(2, 30., 10., 0.)).max() <= 1e-12
    assert np.abs(tr[2] @ A.rotation_matrix(2, np.pi / 2, 0., -20. * np.pi / 180.) - np.eye(9)).max() <= 1e-12
    # a source straight ahead, head turned 90 degrees to the left: the source is now at the right (azimuth -90 degrees)
    tr1 = R.head_trajectory(1, [90.])
    assert np.abs(tr1[0] @ RO.sh_lpmv(0., 0., 1) - RO.sh_lpmv(-np.pi / 2, 0., 1)).max() <= 1e-12


@pytest.fixture(scope='module')
def lib():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_entry_refuses_bad_arguments_before_any_device_call(lib):
    buf = (C.c_float * 64)()
    f = lib.sagen_render_fir
    ok = dict(x=buf, n_hist=0, n=4, channels=4, taps=buf, outputs=2, ntaps=3, rot=None, n_rot=0, rot_hop=0, pos0=0, zero_before=0, y=buf)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['x'], a['n_hist'], a['n'], a['channels'], a['taps'], a['outputs'], a['ntaps'], a['rot'], a['n_rot'], a['rot_hop'],
                 a['pos0'], a['zero_before'], a['y'], None)
    assert call(x=None) == -1 and call(taps=None) == -1 and call(y=None) == -1                # SAGEN_ERR_NULL
    assert b'sagen_render_fir' in lib.sagen_last_error()
    assert call(n=0) == -2 and call(n_hist=-1) == -2 and call(outputs=0) == -2 and call(ntaps=0) == -2 and call(channels=0) == -2   # SAGEN_ERR_SHAPE
    assert call(pos0=-1) == -2 and call(n_hist=3, pos0=2) == -2
    assert call(rot=buf, n_rot=0, rot_hop=4800) == -2 and call(rot=buf, n_rot=1, rot_hop=0) == -2
    for kw in (dict(channels=3), dict(channels=16), dict(outputs=33), dict(ntaps=513)):                                    # SAGEN_ERR_UNSUPPORTED
        assert call(**kw) == -3, kw
        assert b'supported' in lib.sagen_last_error()


def _ambix(tmp_path, channels, rate=48000, n=6000):
    fn = str(tmp_path / ('in%d_%d.wav' % (channels, rate)))
    feeder.save_wav(fn, 0.1 * np.random.RandomState(3).normal(size=(n, channels)), rate)
    return fn


def test_render_cli_parsing_and_refusals(tmp_path):
    a = R.parse_arguments(['in.wav', 'out.wav'])
    assert (a.render, a.decode, a.hrir_dir, a.normalize, a.overwrite, a.yaw, a.pitch, a.roll) == ('ears', None, None, None, False, 0., 0., 0.)
    a = R.parse_arguments(['in.wav', 'out.wav', '--render', 'hrir', '--hrir_dir', 'd', '--yaw', '30', '--normalize', '0.95', '--overwrite'])
    assert (a.render, a.hrir_dir, a.yaw, a.normalize, a.overwrite) == ('hrir', 'd', 30., 0.95, True)
    with pytest.raises(SystemExit):
        R.parse_arguments(['in.wav', 'out.wav', '--render', 'stereo'])
    out = str(tmp_path / 'out.wav')
    with pytest.raises(SystemExit, match='hrir_dir'):
        R.main([_ambix(tmp_path, 4), out, '--render', 'hrir'])
    with pytest.raises(SystemExit, match='wy'):
        R.main([_ambix(tmp_path, 9), out, '--render', 'wy'])
    with pytest.raises(SystemExit, match='channels'):
        R.main([_ambix(tmp_path, 5), out])
    with pytest.raises(SystemExit, match='decode'):
        R.main([_ambix(tmp_path, 4), out, '--render', 'mic', '--decode', 'pseudoinv'])
    assert not os.path.exists(out)
    open(out, 'w').close()
    with pytest.raises(SystemExit, match='exists'):
        R.main([_ambix(tmp_path, 4), out])


def test_hrir_refusals_come_from_main_before_device_work(tmp_path, monkeypatch):
    """Both command lines read the HRIR files and build the taps on the host BEFORE they select a device: a rate mismatch or a
    missing directory ends main() with its message while torch.cuda.set_device has not been called (it is made to fail here)."""
    import torch
    from spatialaudiogen_amd import deploy

    def no_device(*_a, **_k):
        raise AssertionError('the device was touched before the refusal')
    monkeypatch.setattr(torch.cuda, 'set_device', no_device)
    dirs, left, right = RO.make_hrirs(14, ntaps=32)
    h44 = str(tmp_path / 'h44')
    RO.write_cipic_dir(h44, left, right, 44100)
    out, ren = str(tmp_path / 'o.wav'), str(tmp_path / 'r.wav')
    with pytest.raises(SystemExit, match='44100'):
        R.main([_ambix(tmp_path, 4), out, '--render', 'hrir', '--hrir_dir', h44])
    with pytest.raises(SystemExit, match='does not exist'):
        R.main([_ambix(tmp_path, 9), out, '--render', 'hrir', '--hrir_dir', str(tmp_path / 'none')])
    d = _params_dir(tmp_path)
    with pytest.raises(SystemExit, match='44100'):
        deploy.main([d, str(tmp_path / 'nowhere'), '--output_fn', out, '--render', 'hrir', '--render_fn', ren, '--hrir_dir', h44])
    with pytest.raises(SystemExit, match='does not exist'):
        deploy.main([d, str(tmp_path / 'nowhere'), '--output_fn', out, '--render', 'hrir', '--render_fn', ren, '--hrir_dir', str(tmp_path / 'none')])
    assert not os.path.exists(out) and not os.path.exists(ren)
    # the host part on its own: taps, zero_before and the rotation of --yaw, no Renderer
    RO.write_cipic_dir(str(tmp_path / 'h48'), left, right, 48000)
    args = R.parse_arguments(['in.wav', 'out.wav', '--render', 'hrir', '--hrir_dir', str(tmp_path / 'h48'), '--yaw', '30'])
    taps, zb, rot = R.rendering_from_arguments(args, 4, 48000, 'render')
    assert taps.shape == (2, 4, 32) and zb == 31 and np.abs(rot[0] - RO.head_rotation(1, 30.)).max() <= 1e-12


def _params_dir(tmp_path):
    d = tmp_path / 'model'
    d.mkdir()
    (d / 'train-params.txt').write_text(
        "ambi_order: 1\naudio_rate: 48000\nvideo_rate: 10\ncontext: 1.0\nsample_dur: 0.1\nencoders: ['audio']\n"
        "separation: unet_mask\nnum_sep_tracks: 32\nloc_units: [512, 512]\n")
    return str(d)


def test_deploy_cli_parsing_and_refusals(tmp_path):
    from spatialaudiogen_amd import deploy
    a = deploy.parse_arguments(['m', 'clip'])
    assert a.render is None and a.render_fn is None and a.output_fn == 'output.wav'
    a = deploy.parse_arguments(['m', 'clip', '--render', 'mic', '--render_fn', 'o.wav', '--pitch', '-10', '--groups', '10'])
    assert (a.render, a.render_fn, a.pitch, a.groups) == ('mic', 'o.wav', -10., 10)
    with pytest.raises(SystemExit):
        deploy.parse_arguments(['m', 'clip', '--render', 'mic'])                     # no --render_fn
    with pytest.raises(SystemExit):
        deploy.parse_arguments(['m', 'clip', '--render_fn', 'o.wav'])
    d = _params_dir(tmp_path)
    out, ren = str(tmp_path / 'a.wav'), str(tmp_path / 'r.wav')
    with pytest.raises(SystemExit, match='hrir_dir'):
        deploy.main([d, str(tmp_path / 'nowhere'), '--output_fn', out, '--render', 'hrir', '--render_fn', ren])
    with pytest.raises(SystemExit, match='decode'):
        deploy.main([d, str(tmp_path / 'nowhere'), '--output_fn', out, '--render', 'wy', '--render_fn', ren, '--decode', 'projection'])
    assert not os.path.exists(out) and not os.path.exists(ren)


def test_normalize_peak():
    y = np.array([[0.1, -0.4], [0.2, 0.3]])
    assert abs(np.abs(R.normalize_peak(y, 0.95)).max() - 0.95) <= 1e-15
    np.testing.assert_array_equal(R.normalize_peak(np.zeros((3, 2)), 0.95), np.zeros((3, 2)))
