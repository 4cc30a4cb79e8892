"""Dense optical flow and the flow folder's byte coding on the device (csrc/flow.hip through ops.optical_flow / ops.flow_encode /
flow.FlowEstimator) against the fp64 numpy restatement of tests/flow_oracle.py, which is written from the description of the
algorithm with whole-array index arithmetic and shares nothing with csrc/flow_core.h.

PARITY TOLERANCE.  The flow is compared as |got - restated| in pixels after the restatement's own rounding to fp32.  The procedure:
measure the CPU twin (the product's fp64 arithmetic, associated differently from numpy's) against the restatement over the parity
cases below, allow 100 x the worst value seen, capped at 1e-6 px, plus one fp32 ulp of the value.  Measured on the twin over all
PARITY cases: worst 0.0 - every fp32 value equal.  The fp64 fields behind them differ by reassociation only, of the order of
1e-14 px after a few thousand contractive updates, against 1.2e-7 .. 4.8e-7 px between neighbouring fp32 values of a flow of
1 .. 8 px; against the restatement BEFORE its rounding the twin differs by 6e-8 .. 4.5e-7 px, which is the fp32 rounding itself.
So the allowance is 100 x 0 = 0 plus the one ulp: two fp64 values 1e-14 apart may still fall on either side of a rounding edge (the
rolled frames of test_roll do: their warp coordinates x + u round differently four columns further on), and one ulp is the smallest
difference two fp32 numbers can have.  TOL(value) = spacing of the restated fp32 value.  Each case prints its figure before it asserts.

ENCODE RULE.  got == floor(pre) wherever the restatement's value before truncation `pre` is farther than EDGE = 1e-6 from an
integer; within EDGE of an integer r either r - 1 or r passes.  pre is at most 255, computed in fp64 on both sides from fp32
inputs through sqrt (exact to the last place) and atan2 (an ulp or two): differences of order 1e-13; 1e-6 leaves seven orders.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_flow.py)."""
import os

import numpy as np
import pytest

import flow_oracle as FO
from util import ensure_lib

pytestmark = pytest.mark.gpu

WORST_SEEN = 0.0                # twin against restatement over PARITY, px (see above)
EDGE = 1e-6
OP_CASES = ('test_parity or test_fusion_depth or test_identical_frames or test_known_shift or test_roll or test_split_clip or '
            'test_encode or test_round_trip or test_error_codes')


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


def _flow(frames, **kw):
    from spatialaudiogen_amd import flow as F, ops
    dev = _dev()
    return ops.optical_flow(_t(frames, dev), F.FlowParams(**kw).struct(*frames.shape[1:3])).cpu().numpy()


# name -> (h, w, frames, parameters)
PARITY = {
    '32x64_levels3': (32, 64, 2, dict(levels=3)),
    '40x72_levels3_ragged_tiles': (40, 72, 2, dict(levels=3)),
    '16x32_levels3_halo_wider_than_the_image': (16, 32, 2, dict(levels=3)),
    '64x128_levels4_iters10': (64, 128, 2, dict(levels=4, iters=10)),
    '32x64_no_wrap': (32, 64, 2, dict(levels=3, wrap=False)),
    '32x64_four_frames': (32, 64, 4, dict(levels=3)),
    '32x64_warps1_iters1': (32, 64, 2, dict(levels=3, warps=1, iters=1)),
}
_CACHE = {}


def _case(name):
    """(frames, restated flow rounded to fp32): computed once per case and shared."""
    if name not in _CACHE:
        h, w, n, kw = PARITY[name]
        frames = FO.pattern_frames(h, w, [(1.7 * k, 0.6 * k) for k in range(n)], seed=h)
        ref = FO.optical_flow(frames, **kw).astype(np.float32)
        ref.setflags(write=False)
        _CACHE[name] = (frames, ref)
    return _CACHE[name]


def tolerance(ref):
    return min(100. * WORST_SEEN, 1e-6) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def assert_flow_close(got, ref, what):
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print('%s: %d values, max |flow| %.3f px, max |got - restated| %.3g px, %d values differ' % (what, d.size, np.abs(ref).max(), d.max(), (d > 0).sum()))
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    bad = d > tolerance(ref)
    assert not bad.any(), '%s: %d values beyond the tolerance, max |got - restated| = %.3g px' % (what, bad.sum(), d.max())


@pytest.mark.parametrize('name', sorted(PARITY))
def test_parity(name):
    frames, ref = _case(name)
    assert np.abs(ref).max() > 1.                                   # the flow is not trivial
    assert_flow_close(_flow(frames, **PARITY[name][3]), ref, name)


@pytest.mark.parametrize('name', ['40x72_levels3_ragged_tiles', '16x32_levels3_halo_wider_than_the_image'])
def test_fusion_depth_does_not_change_a_bit(name):
    frames, _ = _case(name)
    kw = PARITY[name][3]
    auto = _flow(frames, fuse=0, **kw)
    for fuse in (1, 2, 3, 8):
        assert np.array_equal(_flow(frames, fuse=fuse, **kw), auto), 'fuse %d' % fuse


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def test_identical_frames_give_exactly_zero():
    frames = FO.pattern_frames(64, 128, [(0., 0.)] * 3, seed=2)
    got = _flow(frames, levels=4)
    assert got.shape == (2, 64, 128, 2) and not got.any()


def test_known_shift_and_the_seam():
    """The pattern displaced by (3.3, 0) at 64 x 128, levels 4, the defaults otherwise: |u - 3.3| <= 0.25 and |v| <= 0.35 everywhere;
    in the columns next to the seam |u - 3.3| <= 0.25 with wrap and > 5 without (the CPU twin measures 0.054, 0.089, 0.029 and 29.6)."""
    frames = FO.pattern_frames(64, 128, [(0., 0.), (3.3, 0.)], seed=0)
    got = _flow(frames, levels=4)[0]
    seam = [0, 1, 126, 127]
    print('wrap: max |u - 3.3| %.3f, max |v| %.3f, seam columns %.3f' % (np.abs(got[..., 0] - 3.3).max(), np.abs(got[..., 1]).max(),
                                                                        np.abs(got[:, seam, 0] - 3.3).max()))
    assert np.abs(got[..., 0] - 3.3).max() <= 0.25 and np.abs(got[..., 1]).max() <= 0.35
    assert np.abs(got[:, seam, 0] - 3.3).max() <= 0.25
    clamped = _flow(frames, levels=4, wrap=False)[0]
    print('no wrap: seam columns %.3f' % np.abs(clamped[:, seam, 0] - 3.3).max())
    assert np.abs(clamped[:, seam, 0] - 3.3).max() > 5.


def test_roll_by_the_coarsest_pixel_rolls_the_flow():
    """Both frames rolled by k = 2^(levels - 1) columns: every 2 x 2 block of every level moves whole, so the flow rolls with them."""
    frames, _ = _case('32x64_levels3')
    k = 4
    base = _flow(frames, levels=3)
    rolled = _flow(np.roll(frames, k, axis=2), levels=3)
    assert_flow_close(rolled, np.roll(base, k, axis=2), 'rolled by %d' % k)


def test_split_clip_gives_equal_bytes():
    """7 frames at once, and as 3 + 4 with the last frame of the first piece handed on: FlowEstimator keeps nothing between calls."""
    from spatialaudiogen_amd import flow as F
    dev = _dev()
    frames = FO.pattern_frames(32, 64, [(0.9 * k, -0.4 * k) for k in range(7)], seed=5)
    est = F.FlowEstimator(F.FlowParams(levels=3), device=dev)
    whole = est.process(_t(frames, dev)).cpu().numpy()
    assert whole.shape == (7, 32, 64, 2) and whole.dtype == np.float32
    a = est.process(_t(frames[:3], dev)).cpu().numpy()
    b = est.process(_t(frames[3:], dev), prev=_t(frames[2], dev)).cpu().numpy()
    assert np.array_equal(np.concatenate([a, b], 0), whole)
    assert not whole[0].any() and np.abs(whole[1:]).max() > 0.5
    assert np.array_equal(whole[1:], _flow(frames, levels=3))


# ---- the byte coding ----------------------------------------------------------------------------------------------------------------
def _encode_flows():
    flow = np.random.RandomState(11).uniform(-6., 6., size=(3, 48, 96, 2)).astype(np.float32)
    flow[0, 5, 7], flow[1, 40, 90], flow[2, 0, 0] = (0.001, -0.002), (-0.003, 0.0035), (0., 0.)       # |flow| < 0.005: angle 0
    return flow


def _encode(flow):
    from spatialaudiogen_amd import ops
    dev = _dev()
    rgb, limits = ops.flow_encode(_t(flow, dev))
    return rgb.cpu().numpy(), limits.cpu().numpy()


def assert_truncation_rule(got, pre, what):
    r = np.rint(pre)
    near = np.abs(pre - r) <= EDGE
    # the planted pixels (angle 0) and each frame's minimum / maximum pixel (0 and 255) are the only ones expected
    assert near.mean() <= 1e-3, 'input condition: %d of %d values within %g of an integer' % (near.sum(), near.size, EDGE)
    g = got.astype(np.float64)
    ok = np.where(near, (g == r - 1.) | (g == r), g == np.floor(pre))
    print('%s: %d values, %d within %g of an integer, %d wrong' % (what, pre.size, near.sum(), EDGE, (~ok).sum()))
    assert ok.all(), '%d of %d values break the truncation rule' % ((~ok).sum(), ok.size)


def test_encode_truncation_rule_and_limits():
    flow = _encode_flows()
    rgb, limits = _encode(flow)
    pre, ref_limits = FO.encode(flow)
    assert rgb.shape == (3, 48, 96, 3) and rgb.dtype == np.uint8 and limits.shape == (3, 2) and limits.dtype == np.float32
    assert np.array_equal(limits, ref_limits)
    assert not rgb[..., 1].any()
    assert_truncation_rule(rgb[..., 0], pre[..., 0], 'angle')
    assert_truncation_rule(rgb[..., 2], pre[..., 2], 'magnitude')
    assert rgb[0, 5, 7, 0] == 0 and rgb[1, 40, 90, 0] == 0 and rgb[2, 0, 0, 0] == 0


def test_encode_narrow_magnitudes_get_a_span_of_one():
    flow = np.zeros((2, 8, 12, 2), np.float32)
    flow[0, ..., 0] = np.linspace(2., 2.5, 96).reshape(8, 12)       # magnitudes 2 .. 2.5: hi = lo + 1
    flow[1, ..., 1] = np.linspace(-3., 3., 96).reshape(8, 12)       # magnitudes ~0 .. 3: kept
    rgb, limits = _encode(flow)
    pre, ref_limits = FO.encode(flow)
    assert np.array_equal(limits, ref_limits)
    assert limits[0, 0] == np.float32(2.) and limits[0, 1] == np.float32(3.) and limits[1, 1] == np.float32(3.)
    assert rgb[0, ..., 2].max() in (127, 128) and rgb[1, ..., 2].max() in (254, 255)


def test_round_trip_through_the_feeder(tmp_path):
    """encode -> files -> feeder.FlowFrames: channel 2 is the magnitude within one step (hi - lo) / 255, channels 0 and 1 are the
    NEGATED flow (the reference adds pi and never takes it off) within mag 2 pi / 255 + (hi - lo) / 255."""
    from PIL import Image
    from spatialaudiogen_amd.feeder import FlowFrames
    flow = _encode_flows()
    rgb, limits = _encode(flow)
    folder = str(tmp_path / 'flow')
    os.makedirs(folder)
    for k in range(3):
        Image.fromarray(rgb[k]).save(os.path.join(folder, '%06d.jpg' % k), format='PNG')      # lossless bytes under the name the reader opens
    np.save(os.path.join(folder, 'flow_limits.npy'), limits)
    got = FlowFrames(folder, os.path.join(folder, 'flow_limits.npy')).frames(0, 3)
    assert got.shape == (3, 48, 96, 3)
    mag = np.sqrt((flow.astype(np.float64) ** 2).sum(-1))
    step = (limits[:, 1].astype(np.float64) - limits[:, 0])[:, None, None] / 255.
    assert (np.abs(got[..., 2] - mag) <= step).all()
    live = mag >= 0.005
    bound = mag * 2. * np.pi / 255. + step
    for c in (0, 1):
        assert (np.abs(got[..., c] - (-flow[..., c].astype(np.float64)))[live] <= bound[live]).all(), c


# ---- error codes ------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_untouched_output():
    import ctypes as C
    import torch
    from spatialaudiogen_amd import _lib, ops
    from spatialaudiogen_amd import flow as F
    dev = _dev()
    l = _lib.lib()
    n, h, w = 3, 32, 64
    frames = _t(FO.pattern_frames(h, w, [(0., 0.), (1., 0.), (2., 0.)], seed=1), dev)
    out = torch.full((n - 1, h, w, 2), 77., dtype=torch.float32, device=dev)
    nbytes = l.sagen_optical_flow_scratch_bytes(n, h, w, 3)
    assert nbytes >= 8 * (n * h * w + (n - 1) * h * w * 2) and nbytes % 8 == 0
    assert l.sagen_optical_flow_scratch_bytes(n, h, w, 9) == 0 and l.sagen_optical_flow_scratch_bytes(1, h, w, 3) == 0
    scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
    stream = ops._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(fr=frames, n_=n, h_=h, w_=w, p='default', o=out, s=scratch, sb=nbytes, **kw):
        prm = _lib.SagenFlowParams(3, 3, 30, 1, 0, 8.)
        for k, v in kw.items():
            setattr(prm, k, v)
        return l.sagen_optical_flow(ptr(fr), n_, h_, w_, None if p is None else C.byref(prm), ptr(o), ptr(s), sb, stream)

    for kw in (dict(fr=None), dict(p=None), dict(o=None), dict(s=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(n_=-1), dict(h_=0), dict(w_=0), dict(h_=-4), dict(h_=30), dict(w_=62), dict(levels=4, h_=36), dict(sb=nbytes - 8), dict(sb=0)):
        assert call(**kw) == -2, (kw, l.sagen_last_error())
    for kw in (dict(levels=0), dict(levels=9), dict(warps=0), dict(warps=17), dict(iters=0), dict(iters=1001), dict(fuse=-1), dict(fuse=9),
               dict(alpha=0.), dict(alpha=-1.), dict(alpha=float('inf')), dict(alpha=float('nan')), dict(h_=4100, w_=4100), dict(w_=8192),
               dict(levels=5), dict(levels=4, h_=24), dict(n_=65536)):
        assert call(**kw) == -3, (kw, l.sagen_last_error())
    assert b'fuse' in (l.sagen_last_error() if call(fuse=9) == -3 else b'')
    assert b'alpha' in (l.sagen_last_error() if call(alpha=0.) == -3 else b'')
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((out == 77.).all())                                 # every refused call left the flow alone
    # n_frames <= 1: success, nothing looked at
    assert call(n_=0, fr=None, p=None, o=None, s=None, sb=0) == 0 and call(n_=1, fr=None, p=None, o=None, s=None, sb=0) == 0 and call(n_=1) == 0
    assert bool((out == 77.).all())
    assert call() == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert not bool((out == 77.).any())

    # the byte coding
    flow = _t(_encode_flows(), dev)
    rgb = torch.full((3, 48, 96, 3), 201, dtype=torch.uint8, device=dev)
    lim = torch.full((3, 2), -5., dtype=torch.float32, device=dev)
    eb = l.sagen_flow_encode_scratch_bytes(3, 48, 96)
    assert eb >= 3 * 2 * 4 and l.sagen_flow_encode_scratch_bytes(0, 48, 96) == 0
    es = torch.zeros(eb // 4, dtype=torch.float32, device=dev)

    def enc(f=flow, n_=3, h_=48, w_=96, r=rgb, li=lim, s=es, sb=eb):
        return l.sagen_flow_encode(ptr(f), n_, h_, w_, ptr(r), ptr(li), ptr(s), sb, stream)

    for kw in (dict(f=None), dict(r=None), dict(li=None), dict(s=None)):
        assert enc(**kw) == -1, kw
    for kw in (dict(n_=-1), dict(h_=0), dict(w_=-2), dict(sb=eb - 4)):
        assert enc(**kw) == -2, (kw, l.sagen_last_error())
    for kw in (dict(h_=4097), dict(w_=5000), dict(n_=65536)):
        assert enc(**kw) == -3, (kw, l.sagen_last_error())
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((rgb == 201).all()) and bool((lim == -5.).all())
    assert enc(n_=0, f=None, r=None, li=None, s=None, sb=0) == 0
    assert enc(n_=0, h_=0, w_=5000, f=None, r=None, li=None, s=None, sb=0) == 0    # no frame: OK whatever the rest says
    assert enc() == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert not bool((lim == -5.).any())

    # the Python layer refuses before the library is asked
    with pytest.raises(TypeError):
        ops.optical_flow(frames.float())
    with pytest.raises(TypeError):
        ops.optical_flow(frames[..., :2])
    with pytest.raises(TypeError):
        ops.optical_flow(frames, F.FlowParams(levels=3))            # the descriptor, not its struct
    with pytest.raises(ValueError):
        ops.optical_flow(frames[:, :30], _lib.SagenFlowParams(3, 3, 30, 1, 0, 8.))
    with pytest.raises(ValueError):
        F.FlowParams(levels=5).struct(h, w)                         # 2 x 4 pixels on the coarsest level
    with pytest.raises(TypeError):
        ops.flow_encode(flow.double())
    with pytest.raises(TypeError):
        ops.flow_encode(flow[..., :1])
    assert ops.optical_flow(frames[:1]).shape == (0, h, w, 2) and ops.flow_encode(flow[:0])[1].shape == (0, 2)


# ---- command line (needs the device) ------------------------------------------------------------------------------------------------
def test_command_line_end_to_end(tmp_path, capsys):
    """5 jpg frames -> the flow folder; the png bytes are ops called on the decoded frames; the folder reads through the feeder."""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from PIL import Image
    from spatialaudiogen_amd import flow as F, ops
    from spatialaudiogen_amd.feeder import FlowFrames, imread
    video, out, out_jpg = str(tmp_path / 'video'), str(tmp_path / 'flow'), str(tmp_path / 'flow_jpg')
    os.makedirs(video)
    frames = FO.pattern_frames(48, 96, [(1.3 * k, 0.5 * k) for k in range(5)], seed=3)
    for k in range(5):
        Image.fromarray(frames[k]).save(os.path.join(video, '%06d.jpg' % k), quality=95)
    decoded = np.stack([imread(os.path.join(video, '%06d.jpg' % k)) for k in range(5)], 0)
    F.main([video, out, '--format', 'png', '--block', '2', '--iters', '10'])
    assert 'wrote 5 flow frames of 48x96 to %s (levels 4, warps 3, iters 10)' % out in capsys.readouterr().out
    assert sorted(os.listdir(out)) == ['%06d.png' % k for k in range(5)] + ['flow_limits.npy']
    limits = np.load(os.path.join(out, 'flow_limits.npy'))
    assert limits.shape == (5, 2) and limits.dtype == np.float32
    d = torch.as_tensor(decoded).cuda()
    flow = ops.optical_flow(torch.cat([d[:1], d], 0), F.FlowParams(levels=4, iters=10).struct(48, 96))
    rgb, lim = ops.flow_encode(flow)
    got = np.stack([imread(os.path.join(out, '%06d.png' % k)) for k in range(5)], 0)
    assert np.array_equal(got, rgb.cpu().numpy()) and np.array_equal(limits, lim.cpu().numpy())
    assert not got[0].any() and limits[0, 0] == 0. and limits[0, 1] == 1.       # frame 0 against itself
    with pytest.raises(SystemExit):
        F.main([video, out, '--iters', '10'])
    with pytest.raises(SystemExit):
        F.main([video, out_jpg, '--levels', '6'])                   # 48 x 96 cannot be halved five times
    assert not os.path.exists(out_jpg)
    F.main([video, out, '--iters', '10', '--overwrite'])
    assert sorted(os.listdir(out)) == ['%06d.jpg' % k for k in range(5)] + ['flow_limits.npy']
    back = FlowFrames(out, os.path.join(out, 'flow_limits.npy')).frames(0, 5)
    assert back.shape == (5, 48, 96, 3) and np.isfinite(back).all()
