"""The output stage at the op level - sagen_render_fir (csrc/render.hip: render_fir_kernel<4|9>), sagen_encode_sources and
sagen_binauralize_sources (csrc/sources.hip: sources_encode_kernel<4|9>, sources_mic_kernel, sources_hrir_kernel<V4>) - held to the
order of summation include/sagen.h promises, through ctypes on caller-owned buffers.  test_gpu_render.py and test_gpu_sources.py
hold the same kernels to a relative RMS error over 12 000 to 48 000 samples, which cannot see one wrong sample or one wrong path.

Buffers.  y is prefilled with NaN and followed by a NaN guard slice that must stay NaN.  x, the taps, the rotation matrices, the
signals (rows and the columns behind each signal), the directions and the HRIR table are interior slices of larger allocations whose
other elements are NaN: an over-read turns an output into NaN instead of reading a lucky zero.  Every buffer is a live allocation.

Checks per case (u = 2^-24; the cases and operands are output_oracle.render_cases / source_cases, seeded):
  a. BIT FOR BIT on the device against output_oracle's restatement: every step in fp32, one accumulator per output, channels /
     sources outermost, taps ascending, one correctly rounded fma each (the rotation: al = float32(s - m hop) / float32(hop),
     be = 1 - al, M = fma(al, R[m1], be R[m]), x'[c] = fma over e ascending).  Not under the CPU twin, which sums in double.
  b. an ELEMENTWISE bound against the fp64 oracles, on the device and the twin; where it is 0 the output must be exactly 0.
       unrotated render, hrir: |y - fp64| <= (n + 8) u A, n = the terms of that output (taps that reach a sample), A = sum |h x|:
         n fma roundings, each at most u of a partial sum that never exceeds A to first order; + 8 for the second order.
       rotated render: (C K + C + 12) u A', A' = sum |h| Xbar, Xbar_c(s) = sum_e ((1 - a)|R[m]| + a|R[m1]|)_ce |x_e|: the entry
         M_ce carries the roundings of al, be, be R[m] and the fma - 4 u relative to ((1 - a)|R[m]| + a|R[m1]|)_ce - the row sum x'_c
         C fma roundings relative to Xbar_c, and the FIR C K more: (C K + C + 4 + second order) u A'.
       encode, mic: (S + 4) u A, A = sum_s |coef sig|: one rounding of the fp64 coefficient to fp32 plus S fma roundings.
     Measured with a sequential fp32 restatement, the worst |err| / bound is 0.047 at C 9, K 7, 0.0038 at C 4, K 200 and 0.0008 at
     C 9, K 512: the bound is sharp only for short sums; the long ones are seen by (a) and (c).  On the cases here (the device's
     values ARE the restatement's, so test_output_oracle_host.py measures them): render 0.191 (C 4, K 10), rotated render 0.12
     (C 4, K 5), 0.085 at C 9, K 7, 0.0015 at C 4, K 511, 0.0006 at C 9, K 512; encode 0.39, mic 0.29, hrir 0.25 (K 7).
  c. INTEGER KNOWN ANSWERS, bit for bit on the device and the twin.  Render: samples -3..3, taps -2..2, rotation matrices signed
     permutations, rot_hop a power of two (output_oracle.INT_HOP): al, M, x' and every partial sum are exact dyadics
     (C K 6 x 256 < 2^24), so y equals the fp64 reference exactly at every K, n and seam.  Hrir: integer signals and taps with moving
     sources - a wrong index at one sample or a wrong LDS slot at a 256-sample seam changes an integer.
  d. relative RMS error <= 1e-5, the bar of test_gpu_render.py / test_gpu_sources.py, unchanged.
  e. INPUT CONDITIONS, asserted on the restatement alone (and for every case on the host by test_output_oracle_host.py): the
     restatement takes trajectory, direction, distance and nearest index from the fp64 oracle, whose sin / cos may differ from the
     device's by ~1e-16.  No fp64 coefficient lies within 2^-40 (relative) or 2^-46 (absolute) of an fp32 rounding tie, no delay
     dist / 343 rate within 1e-9 of an integer, no candidate direction between 1e-13 and 1e-9 below the maximum (the rule of
     test_gpu_sources.test_track_nearest).  No sample is exempted from any check; a seed that violates a condition is replaced.
     The seeds here measure: nearest tie 2.5e-12 relative (bar 9.1e-13) and 1.7e-14 absolute (bar 1.4e-14), nearest integer delay
     1.6e-4 (bar 1e-9), no ambiguous direction.  (64 moving sources would put a coefficient inside the tie band in most seeds - the
     band is 2^-16 of all values - so the S = 64 scenes move four sources and hold sixty still.)

Cases.  Render, C in {4, 9}: K over output_oracle.TAPS - all twelve (K % 4, full % 3) combinations of the three tap loops, plus 1, 2, 3,
511, 512; n over the lane of 8, the item of 512 and the tile of 1024; outputs 1, 2, 3, 5, 32; n_hist 0, 1, K - 2, K - 1, K + 5 at
pos0 == n_hist and at pos0 = 2^33 + 5; zero_before before pos0, at pos0 + 3, at pos0 + 700, past the end; n_rot 1, 2, 5 at rot_hop 1, 3, 8,
1000 with a control-point seam inside the history rows and inside a tile, a trajectory that ends inside the call and calls wholly
past its end.  Sources: orders 1 and 2, S 1, 3, 64, the distance model off and on, t0 0, 1, 255, 300, n 1, 255, 256, 257, 700, an r == 0
control point, a negative r, nframes 1 and 2 with P > 1, nframes == N - 1 (N = 27 at 48 000, N = 15 at 44 100) with a sample at N - 1
that must not be read, a source 2 cm from an ear; hrir K 1, 3, 4, 7, 200, 512 (K % 4 == 0 both 16-byte aligned and offset by 4 bytes:
both kernel variants, the same bits), D 1, 65, 2048, 2049, 4096, the maximum in the second chunk of the search, a direction duplicated
at 100 and 3000 (100 wins), sources of different nframes, t0 not a multiple of 256 with t - k reaching before 0, zero_before 0, K - 1
and mid-workgroup.

The whole file also runs against the CPU twin (tests/test_cpu_twin_output_ops.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import output_oracle as OO
import sources_oracle as SO
from util import ensure_lib, rel_rms_err

pytestmark = pytest.mark.gpu

TWIN = os.path.basename(os.environ.get('SAGEN_LIB', '')) == 'libsagen_cpu.so'     # the CPU twin: host tensors, sums in double


@pytest.fixture(scope='module')
def T():
    import torch
    if not TWIN:
        assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    ensure_lib()
    return torch


def _device():
    return 'cpu' if TWIN else 'cuda'


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(T):
    return None if TWIN else C.c_void_p(T.cuda.current_stream().cuda_stream)


def _framed(T, a):
    """`a` on the device as the interior of an allocation with one NaN slice in front of it and one behind."""
    if a is None:
        return None
    a = T.as_tensor(np.ascontiguousarray(a))
    big = T.full((a.shape[0] + 2,) + tuple(a.shape[1:]), float('nan'), dtype=a.dtype, device=_device())
    big[1:-1] = a.to(big.device)
    return big[1:-1]


def _guarded(T, shape):
    """A NaN-filled output with one more leading slice behind it, which must still be all NaN after the call."""
    big = T.full((shape[0] + 1,) + tuple(shape[1:]), float('nan'), dtype=T.float32, device=_device())
    return big[:shape[0]], big[shape[0]:]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _where(bad):
    return [tuple(int(v) for v in b) for b in np.argwhere(bad)[:8]]


def _check_random(name, got, restated, ref, bound):
    """(d), (b) and (a) of the module docstring; prints each figure before it asserts."""
    assert got.shape == ref.shape == restated.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), (name, 'outputs not written, or NaN read from outside an operand', _where(~np.isfinite(got)))
    err = rel_rms_err(got, ref)
    diff = np.abs(got.astype(np.float64) - ref)
    frac = np.where(bound > 0, diff / np.maximum(bound, 1e-300), 0.)
    differ = _bits(got) != _bits(restated)
    print('%s: rel rms %.3g (bar %.0e); worst element at %.3g of its bound; %d of %d outputs differ in bits from the restatement%s'
          % (name, err, OO.RMS_BAR, frac.max(), differ.sum(), differ.size, ' (twin: not held)' if TWIN else ''))
    assert err <= OO.RMS_BAR, (name, err)
    bad = diff > bound
    assert not bad.any(), (name, 'elementwise bound', int(bad.sum()), [(w, float(got[w]), float(ref[w]), float(bound[w])) for w in _where(bad)])
    none = bound == 0
    assert not got[none].any(), (name, 'outputs without a contributing term must be exactly 0')
    if not TWIN:
        assert not differ.any(), (name, 'bits', int(differ.sum()), [(w, float(got[w]), float(restated[w])) for w in _where(differ)])


def _check_integers(name, got, ref):
    want = ref.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref), (name, 'the integer reference is not exact in fp32')
    bad = _bits(got) != _bits(want + np.float32(0))       # (the reference's -0.0 of an all-zero sum is +0.0 in a sum that starts at +0.0)
    assert not bad.any(), (name, 'integer known answer', int(bad.sum()), [(w, float(got[w]), float(want[w])) for w in _where(bad)])


# ---- sagen_render_fir -----------------------------------------------------------------------------------------------------------
def _run_render(T, case, operands):
    from spatialaudiogen_amd import _lib
    x, taps, rot, hop = operands
    xd, td, rd = _framed(T, x), _framed(T, taps), _framed(T, rot)
    assert case.C != 4 or xd.data_ptr() % 16 == 0
    y, guard = _guarded(T, (case.n, case.O))
    _lib.check(_lib.lib().sagen_render_fir(_ptr(xd), case.n_hist, case.n, case.C, _ptr(td), case.O, case.K, _ptr(rd), case.n_rot, hop, case.pos0,
                                           case.zero_before, _ptr(y), _stream(T)))
    out = y.cpu().numpy()
    assert bool(T.isnan(guard).all()), (case.name, 'written past y')
    return out


@pytest.mark.parametrize('case', OO.render_cases(), ids=lambda c: c.name)
def test_render_sweep(T, case):
    operands = OO.render_operands(case)
    args, kw = OO.render_call(case, operands)
    A, terms = OO.render_abs_sum(*args, **kw)
    _check_random(case.name, _run_render(T, case, operands), OO.render_fir_fp32(*args, **kw), OO.render_ref(*args, **kw),
                  OO.render_bound(case, A, terms))
    ints = OO.render_operands(case, True)
    args, kw = OO.render_call(case, ints)
    _check_integers(case.name, _run_render(T, case, ints), OO.render_ref(*args, **kw))


# ---- sagen_encode_sources / sagen_binauralize_sources -----------------------------------------------------------------------------
def _run_sources(T, case, scene, misalign=False):
    from spatialaudiogen_amd import _lib, ops
    c, l = case, _lib.lib()
    lengths = [len(s) for s in scene.signals]
    table = ops.SourceTable(list(scene.cps), lengths, c.rate, _device())
    assert list(table.nframes) == [SO.nframes_of(N, c.rate) for N in lengths]
    ld = max(lengths) + 3
    sig = np.full((c.S, ld), np.nan, np.float32)
    for k, s in enumerate(scene.signals):
        sig[k, :len(s)] = s
    sd = _framed(T, sig)
    outs = {'encode': (c.order + 1) ** 2, 'mic': 2, 'hrir': 2}[c.op]
    y, guard = _guarded(T, (c.n, outs))
    if c.op == 'encode':
        rc = l.sagen_encode_sources(*((_ptr(sd), ld) + table.args() + (outs, c.distance_model, OO.RADIUS, c.t0, c.n, _ptr(y), _stream(T))))
    elif c.op == 'mic':
        rc = l.sagen_binauralize_sources(*((_ptr(sd), ld) + table.args() + (_lib.SAGEN_SOURCES_MIC, None, None, 0, 0, 0, c.t0, c.n, _ptr(y), _stream(T))))
    else:
        dd = _framed(T, scene.dirs)
        size = c.D * 2 * c.K
        buf = T.full((size + 16,), float('nan'), dtype=T.float32, device=_device())
        assert buf.data_ptr() % 16 == 0
        off = 5 if misalign else 4                       # 16-byte aligned, or 4 bytes past that
        hd = buf[off:off + size]
        hd.copy_(T.as_tensor(scene.hrir.reshape(-1)))
        assert (hd.data_ptr() % 16 == 0) != misalign
        rc = l.sagen_binauralize_sources(*((_ptr(sd), ld) + table.args() + (_lib.SAGEN_SOURCES_HRIR, _ptr(dd), _ptr(hd), c.D, c.K, c.zero_before, c.t0,
                                                                           c.n, _ptr(y), _stream(T))))
    _lib.check(rc)
    out = y.cpu().numpy()
    assert bool(T.isnan(guard).all()), (c.name, 'written past y')
    return out


@pytest.mark.parametrize('case', OO.source_cases(), ids=lambda c: c.name)
def test_sources_sweep(T, case):
    scene = OO.source_scene(case)
    restated = OO.source_restate(case, scene)
    assert restated.cond.problems() == [], (case.name, 'choose another seed')
    ref, bound = OO.source_ref(case, scene), OO.source_bound(case, restated)
    variants = (False, True) if case.op == 'hrir' and case.K % 4 == 0 else (False,)
    for misalign in variants:
        _check_random(case.name + (' (table offset by 4 bytes)' if misalign else ''), _run_sources(T, case, scene, misalign), restated.y, ref, bound)
    if case.op == 'hrir':
        ints = OO.source_scene(case, True)
        for misalign in variants:
            _check_integers(case.name, _run_sources(T, case, ints, misalign), OO.source_ref(case, ints))
    if case.scene == 'tie':                              # the duplicate at 3000 carries other taps: index 100 must have been taken
        near = SO.nearest_all(scene.dirs, SO.track(scene.cps[0], len(scene.signals[0]), case.rate, np.arange(case.t0, case.t0 + case.n))[1])[0]
        assert (near == 100).all() and not np.array_equal(scene.hrir[100], scene.hrir[3000])
