"""Op-level forward contractions (sagen_conv2d, sagen_fc, sagen_deconv2d of csrc/api.hip over csrc/igemm.hip, igemm3.hip, igemm3dw.hip,
conv3p.hip, the batch-norm statistics they accumulate and the split-K reducer) against plain fp64 references (forward_oracle.py) on
randomised and directed geometries, under every kernel selection the op level can reach.  The companion of test_gpu_backward_ops.py.

The fp16x2 plane families (conv3h, conv3hr, conv3g, the space-to-depth tiles, stem8, stempool) are not reachable through the op-level
ABI: they are out of scope here and keep their model-level tests (forward_oracle.NOT_AT_OP_LEVEL names every such tile with its reason).
The bf16 conv3g_kernel tiles ARE launched by sagen_conv2d on the planes it writes when SAGEN_FORCE_TILE names one (dense 3x3 cases without
a prologue) and are swept that way; the two-team conv3pp_kernel tiles would be too and are left out on purpose (forward_oracle.NOT_SWEPT).

Checks, per case and per scratch size (sagen_conv2d_scratch_bytes, and the pre-planes size that sends a dense 3x3 conv to the
fp32-activation kernels):
  * WHICH KERNEL RUNS: the library's own answer (sagen_conv2d_kernel_name / sagen_fc_kernel_name / sagen_deconv2d_kernel_name, which share
    the descriptor construction and the tile choice with the ops) equals forward_oracle.forward_plan: tile, split-K, plane pre-pass;
  * relative RMS error at the bar test_gpu_ops.py holds: < 2e-5;
  * an ELEMENTWISE bound: |y - fp64| <= (n + 8) * 2^-24 * A, n = the number of contracted terms of that output (taps inside the image x
    Cin), A = sum |xin * w| over them.  Derivation: an fp32 sum of n products, in any order and with any grouping (matrix-instruction
    blocks, zero-padded K tiles and padded taps, which add exact zeros), makes at most n roundings on the way to one output, each of at
    most 2^-24 of a partial sum that never exceeds A to first order: n * 2^-24 * A.  Split-K does not loosen it: partial z sums n_z
    terms of magnitude A_z (sum A_z = A), so the partials carry at most max(n_z) * 2^-24 * A together and the reducer's S - 1
    additions (S - 1) * 2^-24 * A more: ceil(n / S) + S - 1 <= n + 8 for every S the library picks (it keeps 8 K tiles per partial).
    The bf16x3 kernels form each fp32 product from three bf16 planes per operand and drop the low x low terms (2^-16 * 2^-16 of
    |x * w| each, plus the planes' own truncation): the + 8 covers them, as in the backward sweeps.  A fused bias is one more addition
    of a term of magnitude |bias|: n + 1 and A + |bias|.  The prologue relu(x*scale + shift) is computed in fp32 before the contraction
    (in the kernel's operand load or in the plane pre-pass): two roundings, each at most 2^-24 * (|x*scale| + |shift|), and ReLU is
    1-Lipschitz, so A grows by 2 * sum (|x*scale| + |shift|) * |w|.  The CPU twin accumulates in double and rounds once: its n is 1.
    Where the bound is 0 (no term contributes) the output must be exactly the bias, ReLU'd if asked.
    The RMS bar cannot see a tap dropped at one border pixel, one wrong column of an N tail or one unwritten row of an M tail; on these
    small images this bound does;
  * INTEGER KNOWN ANSWERS: inputs and weights from the integers -2..2, prologue scales from {-2,-1,1,2}, shifts from -2..2, small integer
    biases.  Every bf16 plane split, product and fp32 partial sum is then exact (n * 2 * 6 < 2^24), so y equals the integer reference
    BIT FOR BIT in every kernel family at every split-K, and bn_stats equals the exact integer sum and sum of squares as fp64 (the
    kernels sum one tile's rows in fp32 first: exact while 256 consecutive pixels' squares stay below 2^24, forward_oracle.stats_exact,
    which test_forward_oracle_host.py asserts for every case with statistics).  This is the check that sees a row dropped from the
    statistics;
  * bn_stats on random data, per channel, against the fp64 sums of the reference.  With b the elementwise bound of the raw output
    (no bias) and v the reference: the sum is off by at most sum b for the outputs' own errors plus (256 + 8) * 2^-24 * sum (|v| + b)
    for the fp32 additions of one tile's rows (at most 256, and the levels of the cross-lane reduction); the sum of squares by at most
    sum (2 |v| b + b^2) plus (256 + 8 + 1) * 2^-24 * sum (|v| + b)^2 (one more rounding for each square);
  * y and bn_stats are prefilled with NaN, and so is a guard slice behind each: an element no kernel writes fails, and so does a write
    past the end (inside a live allocation: nothing here provokes a fault).
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import forward_oracle as FO
from util import ensure_lib, rel_rms_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {k: os.environ[k] for k in FO.SELECTION_KEYS if k in os.environ}          # the kernel selection this process runs under
TWIN = os.path.basename(os.environ.get('SAGEN_LIB', '')) == 'libsagen_cpu.so'     # the CPU twin (test_cpu_twin_ops.py): host tensors, no plan
TOL = 2e-5
U = 2.0 ** -24


@pytest.fixture(scope='module')
def T():
    import torch
    if not TWIN:
        assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    ensure_lib()
    return torch


def _dev(T, a):
    if a is None:
        return None
    t = T.as_tensor(np.ascontiguousarray(a))
    return t if TWIN else t.cuda()


def _guarded(T, shape, dtype=None):
    """A NaN-filled output with one more leading slice behind it, which must still be all NaN after the call."""
    big = T.full((shape[0] + 1,) + tuple(shape[1:]), float('nan'), dtype=dtype or T.float32, device='cpu' if TWIN else 'cuda')
    return big[:shape[0]], big[shape[0]:]


def _ran(c, scratch):
    """What the library says it runs for the case (None on the twin, which has no kernels to choose from)."""
    if TWIN:
        return None
    from spatialaudiogen_amd import _lib, ops
    l, buf = _lib.lib(), C.create_string_buffer(128)
    if isinstance(c, FO.ConvCase):
        nbytes = ops.conv_2d_scratch_bytes(c.B, c.H, c.W, c.kh, c.kw, c.cin, c.cout, scratch == 'full')
        _lib.check(l.sagen_conv2d_kernel_name(c.B, c.H, c.W, c.cin, c.kh, c.kw, c.cout, c.sh, c.sw, int(c.padding == 'SAME'), int(bool(c.prologue)),
                                              int(c.stats), int(c.bias), nbytes, buf, 128))
    elif isinstance(c, FO.FcCase):
        _lib.check(l.sagen_fc_kernel_name(c.M, c.K, c.N, int(c.bias), l.sagen_fc_scratch_bytes(c.M, c.K, c.N), buf, 128))
    else:
        _lib.check(l.sagen_deconv2d_kernel_name(c.B, c.H, c.W, c.cin, c.kh, c.kw, c.cout, c.sh, c.sw, int(c.bias),
                                                l.sagen_deconv2d_scratch_bytes(c.kh, c.kw, c.cin, c.cout, c.sh, c.sw), buf, 128))
    ran, want = buf.value.decode(), FO.plan_string(FO.forward_plan(c, ENV, scratch))
    assert ran == want, 'selection %s, %s scratch: the library runs %s, expected %s' % (ENV, scratch, ran, want)
    return ran


def _finish(raw, bias, relu):
    y = raw + (0.0 if bias is None else np.asarray(bias, np.float64))
    return np.maximum(y, 0.0) if relu else y


def _bound(A, A_pro, terms, bias):
    """The elementwise bound of the module docstring."""
    n = np.ones_like(A) if TWIN else np.broadcast_to(terms, A.shape) + (0 if bias is None else 1)
    return (n + 8) * U * (A + 2.0 * A_pro + (0.0 if bias is None else np.abs(np.asarray(bias, np.float64))))


def _check_random_stats(ran, st, raw, b):
    """bn_stats of random data against the reference's fp64 sums, at the bound the module docstring derives."""
    assert np.isfinite(st).all(), ('bn_stats not written', ran)
    v, b = np.abs(raw).reshape(-1, raw.shape[-1]), b.reshape(-1, raw.shape[-1])
    tol = np.concatenate([b.sum(0) + 264 * U * (v + b).sum(0), (2 * v * b + b * b).sum(0) + 265 * U * ((v + b) ** 2).sum(0)])
    diff = np.abs(st - FO.stats_ref(raw))
    print('%s: bn_stats at most %.3g of their bound' % (ran, (diff / np.maximum(tol, 1e-300)).max()))
    bad = np.argwhere(diff > tol)
    assert bad.size == 0, ('bn_stats (sum | sum of squares per channel)', ran, [(int(k), float(st[k]), float(FO.stats_ref(raw)[k]), float(tol[k])) for k in bad[:8, 0]])


def _check_random(c, ran, y, raw, A, A_pro, terms, bias, relu):
    """Finite everywhere, the RMS bar, the elementwise bound (module docstring); prints the worst element's fraction of its bound."""
    assert np.isfinite(y).all(), ('elements not written', ran, int((~np.isfinite(y)).sum()))
    ref = _finish(raw, bias, relu)
    assert y.shape == ref.shape
    err = rel_rms_err(y, ref)
    bound = _bound(A, A_pro, terms, bias)
    diff = np.abs(y.astype(np.float64) - ref)
    frac = diff / np.maximum(bound, 1e-300)
    worst = tuple(int(k) for k in np.unravel_index(np.argmax(np.where(bound > 0, frac, 0.0)), frac.shape))
    print('%s %s: rel-RMS %.2e, worst element %s at %.3g of its bound' % (c.name, ran, err, worst, frac[worst]))
    assert err < TOL, (ran, err)
    bad = np.argwhere(diff > bound)
    assert bad.size == 0, ('elementwise bound', ran, len(bad), [(tuple(b), float(y[tuple(b)]), float(ref[tuple(b)]), float(bound[tuple(b)])) for b in bad[:8]])
    none = (A + 2.0 * A_pro) == 0                                              # no term contributes: exactly the bias, ReLU'd if asked
    if none.any():
        want = np.broadcast_to(_finish(np.zeros(1), bias, relu).astype(np.float32), y.shape)
        assert np.array_equal(y[none], want[none]), ('outputs without a contributing term', ran)


def _check_integers(ran, y, raw_i, bias, relu, what='integer known answer'):
    ref_i = _finish(raw_i, bias, relu).astype(np.float32)
    bad = np.argwhere(y != ref_i)
    assert bad.size == 0, (what, ran, len(bad), [(tuple(b), float(y[tuple(b)]), float(ref_i[tuple(b)])) for b in bad[:8]])


# ------------------------------------------------------------------------------------------------------------------------
# sagen_conv2d (+ bn_stats)
# ------------------------------------------------------------------------------------------------------------------------
CONV_CASES, FC_CASES, DECONV_CASES = FO.conv_cases(), FO.fc_cases(), FO.deconv_cases()


def _run_conv(T, ops, c, operands, scratch):
    x, w, b, sc, sf = operands
    Ho, Wo = FO.conv_out(c)[:2]
    out, guard = _guarded(T, (c.B, Ho, Wo, c.cout))
    st, st_guard = _guarded(T, (1, 2 * c.cout), T.float64) if c.stats else (None, None)
    got = ops.conv_2d(_dev(T, x), _dev(T, w), (c.sh, c.sw), c.padding, _dev(T, b), c.relu, _dev(T, sc), _dev(T, sf), return_bn_stats=c.stats,
                      out=out, stats_out=st[0] if c.stats else None, planes_scratch=scratch == 'full')
    y = got[0] if c.stats else got
    assert y.data_ptr() == out.data_ptr()
    assert bool(T.isnan(guard).all()), 'written past y'
    if c.stats:
        assert got[1].data_ptr() == st.data_ptr() and bool(T.isnan(st_guard).all()), 'written past bn_stats'
    return y.cpu().numpy(), (st[0].cpu().numpy() if c.stats else None)


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: c.name)
def test_conv_sweep(T, case):
    """Every case with the full scratch and, where the two differ, with the pre-planes scratch, under the kernel selection of this
    process's environment (test_forward_sweeps_under_kernel_selection re-runs it per switch).  The module docstring states the checks."""
    from spatialaudiogen_amd import ops
    c, geo = case, ((case.sh, case.sw), case.padding)
    x, w, b, sc, sf = operands = FO.conv_operands(c)
    raw = FO.conv_ref(x, w, *geo, sc, sf)
    A = FO.conv_abs_ref(x, w, *geo, sc, sf)
    A_pro = FO.conv_prologue_abs_ref(x, w, *geo, sc, sf) if c.prologue else np.zeros_like(A)
    terms = FO.conv_terms(x.shape, w.shape, *geo)
    ints = FO.conv_operands(c, integers=True)
    exact = FO.integer_exact(int(terms.max()), FO.CONV_INT_X_RANGE[c.prologue])
    raw_i = FO.conv_ref(ints[0], ints[1], *geo, ints[3], ints[4]) if exact else None
    for scratch in FO.SCRATCHES if FO.has_plane_room(c) and not TWIN else FO.SCRATCHES[:1]:
        ran = _ran(c, scratch)
        y, st = _run_conv(T, ops, c, operands, scratch)
        _check_random(c, ran, y, raw, A, A_pro, terms, b, c.relu)
        if c.stats:
            _check_random_stats(ran, st, raw, _bound(A, A_pro, terms, None))
        if exact:
            yi, sti = _run_conv(T, ops, c, ints, scratch)
            _check_integers(ran, yi, raw_i, ints[2], c.relu)
            if c.stats:
                assert FO.stats_exact(raw_i), 'the case is too large for exact fp32 tile sums'
                want = FO.stats_ref(raw_i)
                bad = np.argwhere(sti != want)
                assert bad.size == 0, ('integer bn_stats (sum | sum of squares per channel)', ran, len(bad), [(int(k), float(sti[k]), float(want[k])) for k in bad[:8, 0]])


# ------------------------------------------------------------------------------------------------------------------------
# sagen_fc (+ the split-K reducer)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', FC_CASES, ids=lambda c: c.name)
def test_fc_sweep(T, case):
    from spatialaudiogen_amd import ops
    c = case
    ran = _ran(c, 'full')
    x, w, b = FO.fc_operands(c)
    out, guard = _guarded(T, (c.M, c.N))
    y = ops.fully_connected(_dev(T, x), _dev(T, w), _dev(T, b), c.relu, out=out)
    assert y.data_ptr() == out.data_ptr() and bool(T.isnan(guard).all()), 'written past y'
    _check_random(c, ran, y.cpu().numpy(), FO.fc_ref(x, w), FO.fc_abs_ref(x, w), np.zeros((c.M, c.N)), np.full((1, 1), float(c.K)), b, c.relu)
    if FO.integer_exact(c.K):
        xi, wi, bi = FO.fc_operands(c, integers=True)
        out, guard = _guarded(T, (c.M, c.N))
        yi = ops.fully_connected(_dev(T, xi), _dev(T, wi), _dev(T, bi), c.relu, out=out).cpu().numpy()
        assert bool(T.isnan(guard).all()), 'written past y'
        _check_integers(ran, yi, FO.fc_ref(xi, wi), bi, c.relu)


# ------------------------------------------------------------------------------------------------------------------------
# sagen_deconv2d
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', DECONV_CASES, ids=lambda c: c.name)
def test_deconv_sweep(T, case):
    from spatialaudiogen_amd import ops
    c = case
    ran = _ran(c, 'full')
    x, w, b = FO.deconv_operands(c)
    raw = FO.deconv_ref(x, w, (c.sh, c.sw))
    out, guard = _guarded(T, raw.shape)
    y = ops.deconv_2d(_dev(T, x), _dev(T, w), (c.sh, c.sw), _dev(T, b), c.relu, out=out)
    assert y.data_ptr() == out.data_ptr() and bool(T.isnan(guard).all()), 'written past y'
    terms = FO.deconv_terms(x.shape, w.shape, (c.sh, c.sw))
    _check_random(c, ran, y.cpu().numpy(), raw, FO.deconv_abs_ref(x, w, (c.sh, c.sw)), np.zeros_like(raw), terms, b, c.relu)
    if FO.integer_exact(int(terms.max())):
        xi, wi, bi = FO.deconv_operands(c, integers=True)
        out, guard = _guarded(T, raw.shape)
        yi = ops.deconv_2d(_dev(T, xi), _dev(T, wi), (c.sh, c.sw), _dev(T, bi), c.relu, out=out).cpu().numpy()
        assert bool(T.isnan(guard).all()), 'written past y'
        _check_integers(ran, yi, FO.deconv_ref(xi, wi, (c.sh, c.sw)), bi, c.relu)


# ------------------------------------------------------------------------------------------------------------------------
# the kernel selections: SAGEN_NO_P3, SAGEN_FP32_ONLY, SAGEN_FORCE_TILE = every tile the op level can be forced onto
# ------------------------------------------------------------------------------------------------------------------------
SELECTIONS = [('SAGEN_NO_P3', {'SAGEN_NO_P3': '1'}), ('SAGEN_FP32_ONLY', {'SAGEN_FP32_ONLY': '1'})] + \
             [(FO.TILE_NAMES[i], {'SAGEN_FORCE_TILE': str(i)}) for i in FO.swept_tiles()]
_stopped = []          # why no further child is started: an earlier one did not return 0


@pytest.mark.parametrize('env', [e for _, e in SELECTIONS], ids=[n for n, _ in SELECTIONS])
def test_forward_sweeps_under_kernel_selection(T, env):
    """The switches are read once per process: one child per selection, running only the cases the selection changes
    (forward_oracle.selection_cases), each with its own timeout and started only after the previous one returned 0.  Every child
    asserts per case that the library runs what forward_oracle.forward_plan says the switch selects."""
    from spatialaudiogen_amd import _lib
    assert not _stopped, 'not started: %s' % _stopped[0]
    if 'SAGEN_FORCE_TILE' in env:
        i = int(env['SAGEN_FORCE_TILE'])
        assert _lib.lib().sagen_tile_name(i).decode() == FO.TILE_NAMES[i]
    names = [c.name for c in FO.selection_cases(env)]
    assert names, env
    k = '(test_conv_sweep or test_fc_sweep or test_deconv_sweep) and (%s)' % ' or '.join(names)
    child_env = {k_: v for k_, v in os.environ.items() if k_ not in FO.SELECTION_KEYS}
    child_env.update(env)
    cmd = [sys.executable, '-m', 'pytest', '-m', 'gpu', '-q', '-x', '-rP', '-p', 'no:cacheprovider', os.path.abspath(__file__), '-k', k]
    try:
        r = subprocess.run(cmd, env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _stopped.append('the child of %s ran into its timeout' % env)
        pytest.fail('%s: timeout\n%s' % (env, str(e.stdout or '')[-4000:]))
    if r.returncode != 0:
        _stopped.append('the child of %s returned %d' % (env, r.returncode))
    assert r.returncode == 0, '%s (exit status %d):\n%s\n%s' % (env, r.returncode, r.stdout[-6000:], r.stderr[-1000:])
    print('\n'.join(l for l in r.stdout.split('\n') if 'of its bound' in l))
    assert re.search(r'(?<![0-9])%d passed' % len(names), r.stdout) and 'skipped' not in r.stdout and 'failed' not in r.stdout, (env, names, r.stdout[-500:])


# ------------------------------------------------------------------------------------------------------------------------
# refusals: a negative status and a message, decided on the host, outputs untouched
# ------------------------------------------------------------------------------------------------------------------------
def test_unsupported_forward_calls_are_refused_with_outputs_untouched(T):
    from spatialaudiogen_amd import ops
    from spatialaudiogen_amd._lib import SagenError
    z = lambda *s: T.zeros(*s, dtype=T.float32, device='cuda')

    def refused(fn, *shape):
        out = T.full(shape, float('nan'), dtype=T.float32, device='cuda')
        with pytest.raises(SagenError) as e:
            fn(out)
        T.cuda.synchronize()
        assert e.value.code < 0 and len(str(e.value)) > 20, str(e.value)
        assert bool(T.isnan(out).all()), 'a refused call wrote to its output'

    refused(lambda o: ops.conv_2d(z(1, 6, 6, 12), z(3, 3, 12, 8), 1, 'SAME', out=o), 1, 6, 6, 8)                    # multi-tap: cin a power of two
    refused(lambda o: ops.conv_2d(z(1, 6, 6, 6), z(1, 1, 6, 8), 1, 'SAME', out=o), 1, 6, 6, 8)                      # 1x1: cin a multiple of 4
    refused(lambda o: ops.conv_2d(z(1, 6, 6, 8), z(3, 3, 8, 8), 1, 'SAME', in_scale=z(8), in_shift=z(8), out=o), 1, 6, 6, 8)      # prologue: cin % 16
    refused(lambda o: ops.conv_2d(z(1, 6, 6, 16), z(1, 1, 16, 8), 1, 'SAME', in_scale=z(16), in_shift=z(16), out=o), 1, 6, 6, 8)  # prologue: one tap
    refused(lambda o: ops.conv_2d(z(1, 6, 6, 16), z(3, 3, 16, 8), 1, 'SAME', in_scale=z(16), out=o), 1, 6, 6, 8)    # scale without shift
    refused(lambda o: ops.conv_2d(z(1, 6, 6, 3), z(3, 3, 3, 8), 1, 'SAME', in_scale=z(3), in_shift=z(3), out=o), 1, 6, 6, 8)
    refused(lambda o: ops.conv_2d(z(1, 6, 8, 1), z(3, 6, 1, 8), (1, 4), 'VALID', out=o), 1, 4, 1, 8)                # cin 1: kw % 4
    refused(lambda o: ops.conv_2d(z(1, 6, 12, 1), z(3, 12, 1, 8), (1, 4), 'VALID', out=o), 1, 4, 1, 8)              # cin 1, kh > 1: kw a power of two
    refused(lambda o: ops.fully_connected(z(5, 6), z(6, 8), out=o), 5, 8)                                           # k a multiple of 4
    refused(lambda o: ops.deconv_2d(z(1, 2, 2, 12), z(2, 2, 8, 12), (2, 2), out=o), 1, 4, 4, 8)                     # cin a power of two
    refused(lambda o: ops.deconv_2d(z(1, 2, 2, 8), z(1, 1, 8, 8), (2, 2), out=o), 1, 3, 3, 8)                       # kernel >= stride
