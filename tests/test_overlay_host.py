"""The host side of the power-map overlay, without a GPU: the colour table, the resize rule and the whole contract as the fp64
oracle states it (tests/overlay_oracle.py: orientation, silence, counting), the product's host helpers against it, and the command
line's refusals.  The kernels' twin runs the op-level cases in tests/test_cpu_twin_overlay.py."""
import os

import numpy as np
import pytest

import overlay_oracle as OO
from spatialaudiogen_amd import ambisonics, overlay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = os.path.join(ROOT, 'tests', 'golden', 'skimage_resize_v1.npz')


def pin_arrays():
    """The seeded arrays tools/overlay_pin.py hands to skimage.transform.resize: name -> (array, (H, W))."""
    r = np.random.RandomState(1234)
    return {'grey_up': (r.uniform(size=(7, 12)), (16, 24)),
            'grey_with_zero': (np.maximum(r.uniform(size=(7, 12)) - 0.3, 0.), (16, 24)),
            'grey_down': (r.uniform(size=(7, 12)) + 0.1, (5, 7)),
            'colour_up': (r.uniform(size=(7, 12, 3)) + 0.2, (16, 24)),
            'colour_product': (r.uniform(size=(37, 72, 3)), (224, 448)),
            'identity': (r.uniform(size=(7, 12)), (7, 12))}


# ---- the colour table -----------------------------------------------------------------------------------------------------------
def test_colour_table():
    t = overlay.ylorrd_table()
    assert t.shape == (256, 3) and t.dtype == np.float64
    assert np.abs(t - OO.ylorrd_table()).max() <= 1e-15
    assert np.abs(t - np.load(os.path.join(ROOT, 'tests', 'golden', 'ylorrd_256.npy'))).max() <= 1e-15
    assert np.array_equal(t[0], np.array([255, 255, 204]) / 255.) and np.array_equal(t[255], np.array([128, 0, 38]) / 255.)


def test_colour_table_equals_matplotlib():
    pytest.importorskip('matplotlib')
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    assert np.abs(overlay.ylorrd_table() - plt.cm.YlOrRd(np.linspace(0, 1, 256))[:, :3]).max() <= 1e-15


def test_product_does_not_import_matplotlib():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, '-c', 'import sys; import spatialaudiogen_amd.overlay as o; o.ylorrd_table(); '
                        'assert "matplotlib" not in sys.modules'], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-500:]


# ---- resize -----------------------------------------------------------------------------------------------------------------------
def test_resize_identity_and_fast_form():
    for name, (a, (H, W)) in pin_arrays().items():
        if name == 'colour_product':
            a, H, W = a[:9, :10], 31, 47                             # (the per-pixel loop is slow in Python)
        assert np.array_equal(OO.resize(a, H, W), OO.resize_fast(a, H, W)), name
    a = pin_arrays()['identity'][0]
    assert np.array_equal(OO.resize(a, 7, 12), a)
    a3 = pin_arrays()['colour_up'][0]
    assert np.array_equal(OO.resize(a3, 7, 12), a3)


def test_resize_constant_map_has_no_fade_but_a_map_with_zero_has():
    k = np.full((7, 12), 0.37)
    up = OO.resize(k, 28, 36)
    assert np.abs(up[2:-2, 2:-2] - 0.37).max() <= 1e-15
    # on the border the constant-0 padding would pull the value down; lo = hi = 0.37 > 0 clips it back up: k, not a fade
    assert np.array_equal(up[0], np.full(36, 0.37)) and np.array_equal(up[:, -1], np.full(28, 0.37))
    z = k.copy()
    z[3, 5] = 0.                                                     # now lo = 0: the border fades towards the padding
    up = OO.resize(z, 28, 36)
    assert up[0, 0] < 0.37 * 0.5 and up[0].max() < 0.37 and up[14, 0] < 0.37 and abs(up[8, 3] - 0.37) <= 1e-15
    assert up.min() >= 0. and up.max() <= 0.37


def test_resize_against_scikit_image_pin():
    """tools/overlay_pin.py writes this file on a machine that has scikit-image 0.13.1."""
    if not os.path.exists(PIN):
        pytest.skip('resize UNPINNED against scikit-image 0.13.1')
    with np.load(PIN) as z:
        for name, (a, (H, W)) in pin_arrays().items():
            assert np.abs(OO.resize_fast(a, H, W) - z[name]).max() <= 1e-12, name


# ---- the contract on the oracle ---------------------------------------------------------------------------------------------------
def _plane_wave(az_deg, el_deg, n, order=1, seed=0):
    s = np.random.RandomState(seed).normal(size=n) * 0.2
    y = ambisonics.sh_matrix_at(np.deg2rad(az_deg), np.deg2rad(el_deg), order)
    return s[:, None] * y[None, :]


def _most_opaque(frames_out):
    """On white frames the blue channel falls with alpha and with the colour index: its minimum is the most opaque pixel."""
    f = frames_out.astype(int)[..., 2]
    return np.unravel_index(np.argmin(f.sum(0)), f.shape[1:])


def test_orientation_left_is_left_and_up_is_up():
    H, W = 74, 144
    white = np.full((5, H, W, 3), 255, np.uint8)
    out, maps = OO.overlay(_plane_wave(90., 0., 48000), white, 1)
    assert maps.shape == (2, 37, 72) and out.shape == (5, H, W, 3)
    row, col = _most_opaque(out)
    assert abs(row - H // 2) <= 3 and abs(col - W // 4) <= 6, (row, col)       # azimuth +90 (left) is a quarter in from the left edge
    out, _ = OO.overlay(_plane_wave(90., 60., 48000), white, 1)
    row, col = _most_opaque(out)
    assert row <= H // 4 and abs(col - W // 4) <= 6, (row, col)                 # +60 elevation: (90 - 60) / 180 of the height
    out, _ = OO.overlay(_plane_wave(-90., -60., 48000), white, 1)
    row, col = _most_opaque(out)
    assert row >= 3 * H // 4 and abs(col - 3 * W // 4) <= 6, (row, col)
    # the product's flipped harmonics give the oracle's flipped map: same rows, no flip pass
    x = _plane_wave(90., 60., 4800 * 5, seed=3) + 0.01 * np.random.RandomState(4).normal(size=(24000, 4))
    sh = overlay.overlay_sh(1, 5.)
    direct = np.sqrt(np.mean((x[::5] @ sh.T) ** 2, 0)).reshape(37, 72)
    assert np.abs(direct - OO.maps(x, 1)[0]).max() <= 1e-12
    assert np.argmax(direct) // 72 == 6                                          # +60 degrees: row (90 - 60) / 5


def test_second_order_harmonics_known_values_and_product_agreement():
    """ACN / SN3D at order 2 from first principles: known values at a few directions, and the product's trigonometric form
    (ambisonics.sh_matrix_at, which overlay_sh is built from) against the oracle's independent Cartesian polynomials on the whole
    5-degree mesh - a wrong normalisation or channel order on either side shows here."""
    q = np.sqrt(3.)
    known = {(0., 0.): [1, 0, 0, 1, 0, 0, -0.5, 0, q / 2],            # front: U = sqrt3 / 2, R = -1 / 2
             (90., 0.): [1, 1, 0, 0, 0, 0, -0.5, 0, -q / 2],          # left: U = -sqrt3 / 2
             (45., 0.): [1, np.sqrt(.5), 0, np.sqrt(.5), q / 2, 0, -0.5, 0, 0],      # V peaks between front and left
             (0., 90.): [1, 0, 1, 0, 0, 0, 1, 0, 0],                  # zenith: R = 1
             (0., 45.): [1, 0, np.sqrt(.5), np.sqrt(.5), 0, 0, 0.25, q / 2, q / 4],  # S peaks between front and up
             (90., 45.): [1, np.sqrt(.5), np.sqrt(.5), 0, 0, q / 2, 0.25, 0, -q / 4]}
    for (az, el), want in known.items():
        for got in (OO.harmonics(np.deg2rad(az), np.deg2rad(el), 2), ambisonics.sh_matrix_at(np.deg2rad(az), np.deg2rad(el), 2)):
            assert np.abs(got - np.array(want, np.float64)).max() <= 1e-15, (az, el, got)
    phi, nu = ambisonics.spherical_mesh(5.)
    for order in (1, 2):
        mine = OO.harmonics(phi[::-1].reshape(-1), nu[::-1].reshape(-1), order)
        assert np.abs(overlay.overlay_sh(order) - mine).max() <= 1e-15
    # SN3D: the mean over the sphere of each squared harmonic of degree n is 1 / (2 n + 1) (Gauss-Legendre x uniform azimuth)
    xs, ws = np.polynomial.legendre.leggauss(8)
    az = np.arange(16) * 2 * np.pi / 16
    y = OO.harmonics(az[None, :], np.arcsin(xs)[:, None], 2)
    mean_sq = np.einsum('i,ijc->c', ws / 2., y ** 2) / 16.
    assert np.abs(mean_sq - np.array([1.] + [1 / 3.] * 3 + [1 / 5.] * 5)).max() <= 1e-14


def test_second_order_maps_are_sharper():
    x1, x2 = _plane_wave(30., 10., 24000, 1), _plane_wave(30., 10., 24000, 2)
    m1, m2 = OO.maps(x1, 1)[0], OO.maps(x2, 2)[0]
    assert np.unravel_index(np.argmax(m2), m2.shape) == np.unravel_index(np.argmax(m1), m1.shape) == (16, 29)
    assert (m2 / m2.max() > 0.5).sum() < (m1 / m1.max() > 0.5).sum()
    assert overlay.overlay_sh(2).shape == (37 * 72, 9)


def test_silent_stream_returns_the_frames():
    frames = np.random.RandomState(2).randint(0, 256, size=(12, 9, 10, 3)).astype(np.uint8)
    out, maps = OO.overlay(np.zeros((72000, 4)), frames, 1, res=30.)
    assert maps.shape == (3, 7, 12) and not maps.any() and np.array_equal(out, frames[:10])


@pytest.mark.parametrize('n_rows,n_maps', [(23999, 1), (24000, 1), (47999, 2), (48000, 2), (120003, 5)])
def test_counting(n_rows, n_maps):
    x = np.random.RandomState(n_maps).normal(size=(n_rows, 4)) * 0.1
    assert OO.maps(x, 1, res=30.).shape[0] == n_maps
    full = 5 * (n_maps - 1)
    for n_frames in sorted(set([max(full - 2, 0), full, full + 3])):
        frames = np.zeros((n_frames, 4, 6, 3), np.uint8)
        assert OO.overlay(x, frames, 1, res=30.)[0].shape[0] == min(n_frames, full)
        assert overlay.emitted_frames(n_rows, n_frames) == (n_maps, min(n_frames, full))


# ---- the command line's refusals (all before the device is touched) -----------------------------------------------------------------
def _clip(tmp_path, channels=4, sizes=((8, 12),) * 3):
    from PIL import Image
    from spatialaudiogen_amd import feeder as F
    wav = str(tmp_path / 'in.wav')
    F.save_wav(wav, 0.1 * np.random.RandomState(0).normal(size=(4800, channels)), 48000)
    fdir = tmp_path / 'frames'
    fdir.mkdir()
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(np.full((h, w, 3), 40 * i, np.uint8)).save(str(fdir / ('%06d.jpg' % i)))
    return wav, str(fdir)


def test_command_line_refusals(tmp_path):
    (tmp_path / 'a').mkdir()
    wav, fdir = _clip(tmp_path / 'a', channels=5)
    with pytest.raises(SystemExit) as e:
        overlay.main([wav, fdir, str(tmp_path / 'out_a')])
    assert '5 channels' in str(e.value) and not os.path.exists(str(tmp_path / 'out_a'))
    (tmp_path / 'b').mkdir()
    wav, fdir = _clip(tmp_path / 'b', sizes=((8, 12), (8, 12), (8, 16)))
    with pytest.raises(SystemExit) as e:
        overlay.main([wav, fdir, str(tmp_path / 'out_b')])
    assert '000002.jpg' in str(e.value) and 'one size' in str(e.value)
    (tmp_path / 'c').mkdir()
    wav, fdir = _clip(tmp_path / 'c')
    out = tmp_path / 'out_c'
    out.mkdir()
    (out / '000000.png').write_bytes(b'x')
    with pytest.raises(SystemExit) as e:
        overlay.main([wav, fdir, str(out)])
    assert '--overwrite' in str(e.value) and (out / '000000.png').read_bytes() == b'x'


def test_overlay_refuses_other_channel_counts_before_loading_anything():
    with pytest.raises(ValueError):
        overlay.Overlay(5)
