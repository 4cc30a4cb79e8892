"""The power-map overlay on the device (csrc/overlay.hip through ops.power_map_windows / ops.overlay_blend / overlay.Overlay)
against the fp64 oracle (tests/overlay_oracle.py), and the drivers on top: W2XYZ.deploy_and_overlay and the two command lines.

MAPS: max|got - ref| <= 1e-5 max(1, max|ref|) per map, the bar of the project's other power maps (tests/test_gpu_ops.py).

BLEND: out == floor(pre) at every pixel whose fp64 value before truncation `pre` (the oracle's, computed from the SAME fp32 maps,
table and frames) is farther than 1e-9 from an integer; at the others either neighbour.  No share of pixels is exempt.  1e-9: about
20 fp64 operations on magnitudes <= 255 accumulate <= 6e-13 of rounding; three orders of margin on top.  The colour index
int(v 255) is as sharp an edge, so each case first asserts ON THE ORACLE that no node's v 255 (clamped zeros aside) lies within
1e-9 of an integer - seeded inputs meet this with probability about 1 - 5e-5 at these sizes.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_overlay.py)."""
import os

import numpy as np
import pytest

import overlay_oracle as OO
from util import ensure_lib

pytestmark = pytest.mark.gpu

MAP_BAR = 1e-5
EDGE = 1e-9
OP_CASES = ('test_maps_match_oracle or test_maps_silent_window_and_spread_scales or test_maps_short_stream_and_bad_channels or '
            'test_blend_matches_oracle or test_blend_slice_of_a_longer_stream or test_blend_special_maps_and_frames or '
            'test_blend_refuses_a_missing_map or test_overlay_in_pieces_is_bit_identical or test_overlay_silent_stream or '
            'test_overlay_counting or test_overlay_plane_wave_peaks')


def _dev():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    if _lib.IS_CPU_TWIN:
        return 'cpu'
    import torch
    assert torch.cuda.is_available()
    return 'cuda'


def _t(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _sh(order, res):
    from spatialaudiogen_amd import overlay
    return overlay.overlay_sh(order, res).astype(np.float32)


def assert_maps_close(got, ref, what=''):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for m in range(ref.shape[0]):
        err, top = np.abs(got[m].astype(np.float64) - ref[m]).max(), max(1., np.abs(ref[m]).max())
        print('%s map %d: max err %.3g (bar %.3g)' % (what, m, err, MAP_BAR * top))
        assert err <= MAP_BAR * top


# ---- maps, op level -------------------------------------------------------------------------------------------------------------
def _oracle_maps(x, order, res, stride, window):
    """overlay_oracle's maps of x[::stride] with `window` samples per map (its own fp64 harmonics, flipud applied afterwards; the
    device gets the product's fp32 harmonics in flipped row order, so this also pins the orientation)."""
    return OO.maps_of(x.astype(np.float64)[::stride], order, res, window)


@pytest.mark.parametrize('res', [30., 5.])
@pytest.mark.parametrize('tail', ['two_and_a_bit', 'exactly_three'])
@pytest.mark.parametrize('stride,window', [(5, 4800), (1, 37), (3, 1), (5, 257)])
@pytest.mark.parametrize('channels', [4, 9])
def test_maps_match_oracle(channels, stride, window, tail, res):
    """2 windows x stride + 7 rows leave a partial window (and, for stride > 1, a partial stride step); 'exactly three' ends on the
    last sample of window 3, its stride step incomplete: the last row read is the last row of the buffer."""
    from spatialaudiogen_amd import ops
    dev = _dev()
    order = {4: 1, 9: 2}[channels]
    n_rows = 2 * window * stride + 7 if tail == 'two_and_a_bit' else (3 * window - 1) * stride + 1
    n_maps = len(range(0, n_rows, stride)) // window
    assert n_maps == 3 if tail == 'exactly_three' else n_maps >= 2
    x = (0.3 * np.random.RandomState(channels + stride + window).normal(size=(n_rows, channels))).astype(np.float32)
    got = ops.power_map_windows(_t(x, dev), _t(_sh(order, res), dev), stride, window).cpu().numpy()
    assert got.shape[0] == n_maps and got.dtype == np.float32
    ref = _oracle_maps(x, order, res, stride, window)
    assert_maps_close(got.reshape(ref.shape), ref, 'C%d s%d w%d %s res %g' % (channels, stride, window, tail, res))


@pytest.mark.parametrize('channels', [4, 9])
def test_maps_silent_window_and_spread_scales(channels):
    from spatialaudiogen_amd import ops
    dev = _dev()
    order, stride, window, res = {4: 1, 9: 2}[channels], 5, 4800, 5.
    r = np.random.RandomState(5)
    x = r.normal(size=(4 * window * stride, channels)) * np.logspace(-3, 0, channels)[None, :]       # channel scales 1e-3 .. 1
    x[window * stride:2 * window * stride] = 0.                                                      # window 1 is silent
    x = x.astype(np.float32)
    got = ops.power_map_windows(_t(x, dev), _t(_sh(order, res), dev), stride, window).cpu().numpy()
    ref = _oracle_maps(x, order, res, stride, window)
    assert got.shape[0] == 4 and not got[1].any() and got[0].all() and got[2].all()
    assert_maps_close(got.reshape(ref.shape), ref, 'silent / scales C%d' % channels)


def test_maps_short_stream_and_bad_channels():
    import ctypes as C
    import torch
    from spatialaudiogen_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    sh = _t(_sh(1, 30.), dev)
    P = sh.shape[0]
    x = _t(np.ones((16, 4), np.float32), dev)                    # its first 15 rows: ceil(15 / 5) = 3 decimated samples < window 4
    rms = torch.full((2, P), -7., dtype=torch.float32, device=dev)
    scratch = torch.zeros(64, dtype=torch.float64, device=dev)
    stream = ops._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert l.sagen_power_map_windows(ptr(x), 15, 4, 5, 4, ptr(sh), P, ptr(rms), ptr(scratch), 512, stream) == 0
    assert bool((rms == -7.).all()) and not bool(scratch.any())                                   # nothing was touched
    assert ops.power_map_windows(x[:15], sh, 5, 4).shape == (0, P)
    assert l.sagen_power_map_windows(ptr(x), 16, 4, 5, 4, ptr(sh), P, ptr(rms), ptr(scratch), 512, stream) == 0      # 16 rows: one map
    assert bool((rms[0] != -7.).all()) and bool((rms[1] == -7.).all())
    x5 = _t(np.ones((40, 5), np.float32), dev)
    sh5 = _t(np.ones((P, 5), np.float32), dev)
    assert l.sagen_power_map_windows(ptr(x5), 40, 5, 1, 4, ptr(sh5), P, ptr(rms), ptr(scratch), 512, stream) == -3    # SAGEN_ERR_UNSUPPORTED
    assert b'channels=5' in l.sagen_last_error()
    assert l.sagen_power_map_windows_scratch_bytes(3, 5) == 0 and l.sagen_power_map_windows_scratch_bytes(3, 9) == 3 * 45 * 8


# ---- blend, op level ------------------------------------------------------------------------------------------------------------
def _raw_maps(n, mh, mw, seed):
    return (0.05 + np.random.RandomState(seed).uniform(size=(n, mh, mw))).astype(np.float32)


def _frames(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)


def assert_blend_rule(got, maps, frames, lut, fpm, map0=0, frame0=0, what=''):
    """The module docstring's rule against the oracle fed the same fp32 maps, table and frames."""
    ref, pre, v255 = OO.blend(maps, frames, lut, fpm, map0, frame0)
    live = v255 != 0.                                               # (the clamped zeros sit ON an integer by construction)
    assert np.abs(v255[live] - np.rint(v255[live])).min(initial=1.) > EDGE, 'input condition: a colour index sits on an integer'
    assert got.shape == pre.shape and got.dtype == np.uint8
    near = np.abs(pre - np.rint(pre)) <= EDGE
    g = got.astype(np.float64)
    ok = np.where(near, (g == np.rint(pre)) | (g == np.rint(pre) - 1.), g == np.floor(pre))
    print('%s: %d pixels, %d within %g of an integer, %d wrong, %d differ from the oracle\'s uint8' % (what, ok.size, near.sum(), EDGE, (~ok).sum(), (got != ref).sum()))
    assert ok.all(), '%d of %d pixels break the rule (worst |got - pre| %.3g)' % ((~ok).sum(), ok.size, np.abs(g - pre)[~ok].max())


def _blend(maps, map0, lut, frames, frame0, fpm):
    from spatialaudiogen_amd import ops
    dev = _dev()
    return ops.overlay_blend(_t(maps, dev), map0, _t(lut, dev), _t(frames, dev), frame0, fpm).cpu().numpy()


BLEND_SHAPES = [
    (7, 12, 7, 12, 5, 5),           # identity
    (7, 12, 16, 24, 5, 5),          # upscale
    (7, 12, 5, 7, 5, 5),            # downscale, odd sizes (no vector path: 7 % 4)
    (37, 72, 224, 448, 10, 5),      # the product's shapes, 10 frames
    (3, 4, 9, 10, 6, 3),            # frames_per_map 3
    (7, 12, 16, 24, 7, 5),          # a frame count that is no multiple of frames_per_map
    (5, 9, 11, 1030, 3, 5),         # more than one workgroup along a row (512 pixels each), a ragged last one
    (2, 127, 6, 131, 2, 5),         # a map wider than the frame's rows are long in workgroups: 129 staged columns, 131 pixels
]


@pytest.mark.parametrize('mh,mw,h,w,n,fpm', BLEND_SHAPES)
def test_blend_matches_oracle(mh, mw, h, w, n, fpm):
    lut = OO.ylorrd_table()
    maps = _raw_maps((n - 1) // fpm + 2, mh, mw, 11 + h)
    frames = _frames(n, h, w, 13 + w)
    got = _blend(maps, 0, lut, frames, 0, fpm)
    assert_blend_rule(got, maps, frames, lut, fpm, what='blend %dx%d -> %dx%d, %d frames' % (mh, mw, h, w, n))


def test_blend_slice_of_a_longer_stream():
    """map0 / frame0 non-zero: frames 7..18 of a stream with their maps 1..4 equal the same slice of the whole."""
    lut = OO.ylorrd_table()
    maps, frames = _raw_maps(6, 7, 12, 3), _frames(25, 16, 24, 4)
    whole = _blend(maps, 0, lut, frames, 0, 5)
    part = _blend(maps[1:5], 1, lut, frames[7:19], 7, 5)
    assert np.array_equal(part, whole[7:19])
    assert_blend_rule(part, maps[1:5], frames[7:19], lut, 5, 1, 7, what='slice')
    assert_blend_rule(whole, maps, frames, lut, 5, what='whole')


def test_blend_special_maps_and_frames():
    lut = OO.ylorrd_table()
    r = np.random.RandomState(8)
    # (a) opposite ramps at beta = 0.4, 0.6: the interpolated value is > 0.35 everywhere, so v > 0 and lo > 0 - resize keeps exact zeros
    t = np.linspace(0., 1., 7 * 12).reshape(7, 12) + 0.002 * r.uniform(size=(7, 12))
    maps = np.stack([1. + t, 2. - t], 0).astype(np.float32)
    frames = _frames(2, 16, 24, 5)
    v = OO.blend(maps, frames, lut, 5, 0, 2)[2]
    assert v.min() > 0.
    assert_blend_rule(_blend(maps, 0, lut, frames, 2, 5), maps, frames, lut, 5, 0, 2, what='lo > 0')
    # (b) an all-equal map (max - min = 0) next to a live one, and two of them
    maps = np.stack([np.full((7, 12), 0.25, np.float32), _raw_maps(1, 7, 12, 6)[0], np.full((7, 12), 3., np.float32), np.full((7, 12), 3., np.float32)], 0)
    frames = _frames(15, 16, 24, 7)
    got = _blend(maps, 0, lut, frames, 0, 5)
    assert_blend_rule(got, maps, frames, lut, 5, what='flat maps')
    assert np.array_equal(got[0], frames[0])                        # beta = 0 on a flat map: v = 0, alpha = 0
    # (c) frames at 0 and at 255
    maps = _raw_maps(2, 7, 12, 9)
    frames = np.stack([np.zeros((16, 24, 3), np.uint8), np.full((16, 24, 3), 255, np.uint8), np.zeros((16, 24, 3), np.uint8),
                       np.full((16, 24, 3), 255, np.uint8)], 0)
    assert_blend_rule(_blend(maps, 0, lut, frames, 0, 5), maps, frames, lut, 5, what='black / white frames')


def test_blend_refuses_a_missing_map():
    from spatialaudiogen_amd import _lib
    lut = OO.ylorrd_table()
    maps, frames = _raw_maps(2, 3, 4, 1), _frames(6, 9, 10, 2)
    for map0, frame0, n in ((0, 0, 6), (1, 0, 1), (0, 5, 1), (1, 9, 2)):          # cur missing, prev missing, cur missing, cur missing
        with pytest.raises(_lib.SagenError) as e:
            _blend(maps, map0, lut, frames[:n], frame0, 5)
        assert e.value.code == -2                                   # SAGEN_ERR_SHAPE
    assert _blend(maps, 0, lut, frames[:5], 0, 5).shape == (5, 9, 10, 3)
    assert _blend(maps, 0, lut, frames[:0], 0, 5).shape == (0, 9, 10, 3)


# ---- Overlay, streams in pieces -------------------------------------------------------------------------------------------------
def _stream_signal(channels, n_rows, seed):
    r = np.random.RandomState(seed)
    env = 0.1 + np.abs(np.sin(np.arange(n_rows) / 9000.))[:, None]
    return (0.3 * env * r.normal(size=(n_rows, channels)) * (1. + np.arange(channels))[None, :] / channels).astype(np.float32)


def _run_overlay(ov, x, frames, row_pieces, frame_pieces):
    """Feed the two streams in pieces (the shorter list is padded with empty pieces); returns the concatenated output."""
    import torch
    ov.reset()
    xt, ft = _t(x, ov.device), _t(frames, ov.device)
    out, i, j = [], 0, 0
    for k in range(max(len(row_pieces), len(frame_pieces))):
        a = row_pieces[k] if k < len(row_pieces) else 0
        b = frame_pieces[k] if k < len(frame_pieces) else 0
        out.append(ov.process(xt[i:i + a] if a else None, ft[j:j + b]))
        i, j = i + a, j + b
    assert i == x.shape[0] and j == frames.shape[0]
    out = [o for o in out if o.shape[0]]
    return torch.cat(out, 0).cpu().numpy() if out else np.zeros((0,) + frames.shape[1:], np.uint8)


def _cut(total, pieces):
    """`pieces` repeated until `total` is used up."""
    out, k = [], 0
    while sum(out) < total:
        out.append(min(pieces[k % len(pieces)], total - sum(out)))
        k += 1
    return out


@pytest.mark.parametrize('channels', [4, 9])
def test_overlay_in_pieces_is_bit_identical(channels):
    from spatialaudiogen_amd import overlay
    n_rows, n_frames = 120003, 27                                   # 5 maps -> 20 frames finished, 7 left pending
    x, frames = _stream_signal(channels, n_rows, 21), _frames(n_frames, 16, 24, 22)
    ov = overlay.Overlay(channels, device=_dev())
    whole = _run_overlay(ov, x, frames, [n_rows], [n_frames])
    maps = ov.maps().cpu().numpy()
    assert whole.shape == (20, 16, 24, 3) and maps.shape == (5, 37, 72)
    even = _run_overlay(ov, x, frames, _cut(n_rows, [4800]), _cut(n_frames, [1]))
    assert np.array_equal(even, whole) and np.array_equal(ov.maps().cpu().numpy().view(np.uint32), maps.view(np.uint32))
    ragged = _run_overlay(ov, x, frames, _cut(n_rows, [1, 4799, 24001, 3, 23996, 5000]), _cut(n_frames, [0, 3, 7]))
    assert np.array_equal(ragged, whole) and np.array_equal(ov.maps().cpu().numpy().view(np.uint32), maps.view(np.uint32))
    late = _run_overlay(ov, x, frames, [0] * 3 + [n_rows], [n_frames])          # all the frames before any audio
    assert np.array_equal(late, whole)
    # and the whole against the oracle: its maps, then the blend rule on the device's own maps
    assert_maps_close(maps, OO.maps(x, {4: 1, 9: 2}[channels]), 'Overlay C%d' % channels)
    assert_blend_rule(whole, maps, frames[:20], OO.ylorrd_table(), 5, what='Overlay C%d' % channels)


def test_overlay_silent_stream():
    """Silence: every map is 0, v = 0, alpha = 0 - the frames come back bit for bit (and only 5 (n_maps - 1) of them)."""
    from spatialaudiogen_amd import overlay
    frames = _frames(12, 16, 24, 30)
    ov = overlay.Overlay(4, device=_dev())
    out = _run_overlay(ov, np.zeros((3 * 24000, 4), np.float32), frames, [3 * 24000], [12])
    assert np.array_equal(out, frames[:10]) and not ov.maps().cpu().numpy().any()


@pytest.mark.parametrize('az,el', [(90., 0.), (-60., 30.), (135., -45.)])
def test_overlay_plane_wave_peaks(az, el):
    """A plane wave encoded by the oracle's own harmonics (Cartesian polynomials, independent of the product's) must peak at its
    direction's pixel of the product's map, at both orders: row (90 - el) / 5, column (175 - az) / 5.  And the order-2 beam
    (1 + cos g + (3 cos^2 g - 1) / 2) / 3 is narrower than the order-1 beam (1 + cos g) / 2: fewer nodes above half the peak."""
    from spatialaudiogen_amd import overlay
    above_half = {}
    for channels, order in ((4, 1), (9, 2)):
        x = OO.plane_wave(az, el, 0.2 * np.random.RandomState(3).normal(size=24000), order).astype(np.float32)
        ov = overlay.Overlay(channels, device=_dev())
        ov.process(_t(x, ov.device), None)
        m = ov.maps().cpu().numpy()
        assert m.shape == (1, 37, 72)
        assert np.unravel_index(np.argmax(m[0]), (37, 72)) == (int(round((90. - el) / 5.)), int(round((175. - az) / 5.)))
        assert_maps_close(m, OO.maps(x, order), 'plane wave C%d' % channels)
        above_half[order] = int((m[0] > 0.5 * m.max()).sum())
    assert above_half[2] < above_half[1], above_half


@pytest.mark.parametrize('n_rows', [23999, 24000, 47999, 48000, 120003])
def test_overlay_counting(n_rows):
    """n_maps = len(ambix[::5]) // 4800, and min(frames, 5 (n_maps - 1)) frames are written: fewer, as many and more frames given."""
    from spatialaudiogen_amd import overlay
    n_maps = len(np.zeros(n_rows)[::5]) // 4800
    assert n_maps == {23999: 1, 24000: 1, 47999: 2, 48000: 2, 120003: 5}[n_rows]
    full = 5 * (n_maps - 1)
    x = _stream_signal(4, n_rows, 40)
    ov = overlay.Overlay(4, angular_res=30., device=_dev())
    for n_frames in sorted(set([max(full - 2, 0), full, full + 3])):
        frames = _frames(n_frames, 4, 6, n_frames)
        out = _run_overlay(ov, x, frames, [n_rows], [n_frames])
        want = min(n_frames, full)
        assert out.shape[0] == want and ov.maps().shape == (n_maps, 7, 12)
        assert overlay.emitted_frames(n_rows, n_frames) == (n_maps, want)
        ref = OO.overlay(x, frames, 1, res=30.)[0]
        assert ref.shape[0] == want


# ---- driver level (needs the device) ----------------------------------------------------------------------------------------------
class Params(object):
    ambi_order, audio_rate, video_rate, context, sample_dur = 1, 48000, 10, 1.0, 0.1
    separation, num_sep_tracks, fft_window = 'unet_mask', 32, 0.025
    context_units, freq_mask_units, loc_units = [64, 128, 128], [], [512, 512]

    def __init__(self, encoders):
        self.encoders = encoders


def test_deploy_and_overlay_matches_deploy_and_the_oracle():
    """The 12 s clip of the rendering test deployed for 10 s = 95 windows = 456 000 rows -> 19 maps -> 90 frames (the last batch is
    partial: only its valid rows and frames may reach the overlay).  ambi is bit-identical to deploy(); the maps match the oracle's
    maps of that output; the frames obey the blend rule on the device's own maps; grouped launches and a renderer change nothing."""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import overlay, render as R
    from spatialaudiogen_amd.deploy import W2XYZ, ClipArrays
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    from util import rng
    enc = ['audio']
    audio = (0.3 * rng(12).normal(size=(12 * 48000, 4))).astype(np.float32)
    frames = _frames(120, 32, 64, 50)
    model = W2XYZ(params=Params(enc), variables=init_weights(variable_specs(enc), seed=4, mode='test'))
    want = model.deploy(ClipArrays(audio), 0., 10.)
    assert want.shape == (95 * 4800, 4)
    ov = overlay.Overlay(4)
    clip = ClipArrays(audio, frames=frames)
    ambi, painted = model.deploy_and_overlay(clip, 0., 10., ov)
    assert np.array_equal(ambi.view(np.uint32), want.view(np.uint32))
    maps = ov.maps().cpu().numpy()
    assert maps.shape == (19, 37, 72) and painted.shape == (90, 32, 64, 3) and painted.dtype == np.uint8
    assert_maps_close(maps, OO.maps(want, 1), 'deploy_and_overlay')
    # frame F is the one the feeder selects for output window F: frame_index of the window's (shifted) time
    from spatialaudiogen_amd.deploy import frame_index, window_times
    ts = window_times(ClipArrays(audio).chunks_t, 0., 10.)
    used = frames[[frame_index(t, 10) for t in ts[:90]]]
    assert_blend_rule(painted, maps, used, OO.ylorrd_table(), 5, what='deploy_and_overlay')
    taps, zb = R.build_taps('mic', 1, 48000)
    model.groups = 3
    ambi3, painted3, rendered = model.deploy_and_overlay(clip, 0., 10., ov, R.Renderer(taps, zb))
    model.groups = 1
    assert np.array_equal(ambi3.view(np.uint32), want.view(np.uint32)) and np.array_equal(painted3, painted)
    assert rendered.shape == (95 * 4800, 2)
    with pytest.raises(ValueError):
        model.deploy_and_overlay(ClipArrays(audio), 0., 10., ov)        # no decoded frames
    with pytest.raises(ValueError):
        model.deploy_and_overlay(clip, 0., 10., None)
    assert np.array_equal(model.deploy(ClipArrays(audio), 0., 10.).view(np.uint32), want.view(np.uint32))


def _read_pngs(folder):
    from spatialaudiogen_amd.feeder import imread
    names = sorted(f for f in os.listdir(folder) if f.endswith('.png'))
    assert names == ['%06d.png' % i for i in range(len(names))]
    return np.stack([imread(os.path.join(folder, f)) for f in names], 0) if names else np.zeros((0, 0, 0, 3), np.uint8)


def test_command_lines_end_to_end(tmp_path, capsys):
    """deploy --overlay_dir and the overlay command line on temporary files: 2.5 s = 20 windows = 96 000 rows -> 4 maps -> 15 PNG
    frames that equal what the drivers return, next to an unchanged ambisonic wav; the count is printed."""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from test_feeder import make_clip
    from spatialaudiogen_amd import deploy, feeder as F, overlay
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    enc = ['audio']
    model_dir = tmp_path / 'model'
    model_dir.mkdir()
    np.savez(str(model_dir / 'variables.npz'), **init_weights(variable_specs(enc), seed=8, mode='test'))
    (model_dir / 'train-params.txt').write_text(
        "encoders: ['audio']\nseparation: unet_mask\nambi_order: 1\naudio_rate: 48000\nvideo_rate: 10\ncontext: 1.0\n"
        "num_sep_tracks: 32\nloc_units: [512, 512]\n")
    clip_dir = str(tmp_path / 'clip')
    make_clip(clip_dir, secs=4, video=True)                         # an audio-only MODEL on a clip that has frames
    plain_fn, ambi_fn, out_dir, maps_fn = str(tmp_path / 'plain.wav'), str(tmp_path / 'ambi.wav'), str(tmp_path / 'painted'), str(tmp_path / 'maps.npz')
    deploy.main([str(model_dir), clip_dir, '--deploy_duration', '2.5', '--output_fn', plain_fn])
    capsys.readouterr()
    deploy.main([str(model_dir), clip_dir, '--deploy_duration', '2.5', '--output_fn', ambi_fn, '--overlay_dir', out_dir, '--save_maps', maps_fn])
    assert 'wrote 15 frames to %s (4 maps of 37x72)' % out_dir in capsys.readouterr().out
    assert open(plain_fn, 'rb').read() == open(ambi_fn, 'rb').read()                 # the ambisonic wav is written as before
    model = deploy.W2XYZ(str(model_dir))
    ov = overlay.Overlay(4)
    pred, painted = model.deploy_and_overlay(clip_dir, 0., 2.5, ov)
    got = _read_pngs(out_dir)
    assert got.shape == (15, 224, 448, 3) and np.array_equal(got, painted)
    assert np.array_equal(np.load(maps_fn)['maps'], ov.maps().cpu().numpy())
    ts = deploy.window_times(F.read_pow_list(os.path.join(clip_dir, 'audio_pow.lst'))[0], 0., 2.5)             # the feeder's frame per window
    picks = [deploy.frame_index(t, 10) for t in ts[:15]]
    assert len(ts) == 20 and picks[0] == 0 and picks[-1] in (13, 14) and sorted(picks) == picks
    jpgs = np.stack([F.imread(os.path.join(clip_dir, 'video', '%06d.jpg' % i)) for i in picks], 0)
    assert_blend_rule(painted, ov.maps().cpu().numpy(), jpgs, OO.ylorrd_table(), 5, what='deploy --overlay_dir')
    with pytest.raises(SystemExit):                                 # the folder holds frames now
        deploy.main([str(model_dir), clip_dir, '--deploy_duration', '2.5', '--output_fn', ambi_fn, '--overlay_dir', out_dir])

    # the overlay command line on the wav the deploy wrote and the clip's frames from 000000 on
    out2 = str(tmp_path / 'painted2')
    overlay.main([ambi_fn, os.path.join(clip_dir, 'video'), out2, '--block', '7'])
    assert 'wrote 15 frames to %s (4 maps of 37x72)' % out2 in capsys.readouterr().out
    data, rate = F.load_wav(ambi_fn)
    ov.reset()
    frames = np.stack([F.imread(os.path.join(clip_dir, 'video', '%06d.jpg' % i)) for i in range(40)], 0)
    ref = ov.process(torch.as_tensor(data.astype(np.float32)).cuda(), torch.as_tensor(frames).cuda()).cpu().numpy()
    assert np.array_equal(_read_pngs(out2), ref)
    assert_blend_rule(ref, ov.maps().cpu().numpy(), frames[:15], OO.ylorrd_table(), 5, what='overlay command line')
    with pytest.raises(SystemExit):
        overlay.main([ambi_fn, os.path.join(clip_dir, 'video'), out2])
    overlay.main([ambi_fn, os.path.join(clip_dir, 'video'), out2, '--overwrite', '--angular_res', '30'])
    assert 'wrote 15 frames to %s (4 maps of 7x12)' % out2 in capsys.readouterr().out
