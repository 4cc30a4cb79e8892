"""Op-level backward kernels (csrc/wgrad.hip, backward.hip, the adjoints of fft.hip / train.hip) against plain fp64 references
(backward_oracle.py) on randomised and directed geometries, under every weight-gradient kernel selection.

Checks of the two contraction sweeps, per case:
  * relative RMS error at the bars the project holds: weight gradient < 1e-5, data gradient < 2e-5;
  * an ELEMENTWISE bound on the weight gradient: |dw - fp64| <= (n + 8) * 2^-24 * sum |G * D|, n = the number of contracted pixels.
    Derivation: an fp32 sum of n products, in any order and with any grouping (matrix-instruction blocks, pixel ranges reduced
    afterwards), makes at most n roundings on the way to one output, each of at most 2^-24 of a partial sum that never exceeds
    sum |G * D| to first order: n * 2^-24 * sum |G * D|.  The bf16x3 kernels form each fp32 product from three bf16 planes per operand
    and drop the low x low terms (2^-16 * 2^-16 of |g * d| each plus the planes' own truncation): the + 8 covers them.  The reference
    kernel accumulates in fp64 and rounds once: its n is 1.  Where no pixel contributes the bound is 0: such taps must be exactly 0.
    The RMS bar cannot see one pixel lost at one tap or one channel; on these small images this bound does;
  * integer known answers: operands from the integers -2..2.  Every bf16 plane split, product and fp32 partial sum is then exact
    (n * 2 * 2 < 2^24), so the result equals the integer reference BIT FOR BIT in every kernel family at every split;
  * outputs are prefilled with NaN, and so is a guard slice behind them: an element no kernel writes fails, and so does a write past the end.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import backward_oracle as BO
from util import rng, ensure_lib, rel_rms_err, rms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {k: os.environ[k] for k in BO.SELECTION_KEYS if k in os.environ}          # the kernel selection this process runs under
WGRAD_CASES = BO.wgrad_cases()
DGRAD_CASES = BO.dgrad_cases()


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    return torch


def _nan(T, *shape):
    return T.full(shape, float('nan'), dtype=T.float32, device='cuda')


def _guarded(T, *shape):
    """A NaN-filled output with one more leading slice behind it, which must still be all NaN after the call."""
    big = _nan(T, shape[0] + 1, *shape[1:])
    return big[:shape[0]], big[shape[0]:]


def _launch_description(c, split):
    from spatialaudiogen_amd import _lib
    l = _lib.lib()
    buf = C.create_string_buffer(128)
    nbytes = l.sagen_wgrad_scratch_bytes(c.kh, c.kw, c.Cg, c.Cd) if split else 0
    _lib.check(l.sagen_wgrad_kernel_name(c.B, c.HG, c.WG, c.Cg, c.Hd, c.Wd, c.Cd, c.kh, c.kw, c.sh, c.sw, c.h0, c.w0, nbytes, buf, 128))
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------------------------------
# sagen_wgrad
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_randomised_sweep(T, case):
    """Every case with and without pixel-range splitting, under the kernel selection of this process's environment
    (test_wgrad_sweep_under_every_kernel_selection re-runs it per switch).  The module docstring states the checks."""
    from spatialaudiogen_amd import ops
    c = case
    geo = dict(kh=c.kh, kw=c.kw, stride=(c.sh, c.sw), origin=(c.h0, c.w0))
    G, D = BO.wgrad_operands(c)
    ref = BO.wgrad_ref(G, D, **geo)
    scale = BO.wgrad_abs_ref(G, D, **geo)
    n = c.B * c.Hd * c.Wd
    Gi, Di = BO.wgrad_operands(c, integers=True)
    ref_i = BO.wgrad_ref(Gi, Di, **geo).astype(np.float32) if BO.integer_exact(n) else None
    gd, dd = T.as_tensor(G).cuda(), T.as_tensor(D).cuda()
    gid, did = T.as_tensor(Gi).cuda(), T.as_tensor(Di).cuda()
    for split in (True, False):
        plan = BO.wgrad_plan(c, ENV, split)
        ran = _launch_description(c, split)
        assert ran == BO.plan_string(plan), 'selection %s, split %s: the library runs %s, expected %s' % (ENV, split, ran, BO.plan_string(plan))
        out, guard = _guarded(T, c.kh, c.kw, c.Cg, c.Cd)
        dw = ops.wgrad(gd, dd, c.kh, c.kw, (c.sh, c.sw), (c.h0, c.w0), split=split, out=out)
        assert dw.data_ptr() == out.data_ptr()
        assert bool(T.isnan(guard).all()), ('written past the output', ran)
        dw = dw.cpu().numpy()
        assert np.isfinite(dw).all(), ('elements not written', ran, int((~np.isfinite(dw)).sum()))
        err = rel_rms_err(dw, ref)
        n_acc = 1 if plan.kernel == 'wgrad_ref_kernel' else n          # (wgrad_ref_kernel: `double acc`, one rounding at the store)
        excess = np.abs(dw.astype(np.float64) - ref) - (n_acc + 8) * 2.0 ** -24 * scale
        worst = np.unravel_index(np.argmax(excess), excess.shape)
        print('%s split=%d %s: rel-RMS %.2e, worst element %s at %.3g of its bound' % (
            c.name, split, ran, err, worst, abs(dw[worst] - ref[worst]) / max((n_acc + 8) * 2.0 ** -24 * scale[worst], 1e-300)))
        assert err < 1e-5, (ran, err)
        assert excess.max() <= 0, ('elementwise bound', ran, worst, float(dw[worst]), float(ref[worst]), float(scale[worst]))
        if ref_i is not None:
            out, guard = _guarded(T, c.kh, c.kw, c.Cg, c.Cd)
            dwi = ops.wgrad(gid, did, c.kh, c.kw, (c.sh, c.sw), (c.h0, c.w0), split=split, out=out).cpu().numpy()
            assert bool(T.isnan(guard).all()), ('written past the output', ran)
            bad = np.argwhere(dwi != ref_i)
            assert bad.size == 0, ('integer known answer', ran, len(bad), [(tuple(b), float(dwi[tuple(b)]), float(ref_i[tuple(b)])) for b in bad[:8]])


def _child(env_add, args, timeout):
    env = {k: v for k, v in os.environ.items() if k not in BO.SELECTION_KEYS and k not in ('SAGEN_NO_H2', 'SAGEN_RED_BLOCKS')}
    env.update(env_add)
    r = subprocess.run([sys.executable, '-m', 'pytest', '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider'] + args, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, '%s %s:\n%s\n%s' % (env_add, args, r.stdout[-4000:], r.stderr[-1000:])
    return r.stdout


def test_wgrad_sweep_under_every_kernel_selection(T):
    """The switches are read once per process: one child per setting, one after another, none after the first that fails.  Every child
    asserts per case that the library runs the family the switch names (sagen_wgrad_kernel_name against backward_oracle.wgrad_plan);
    here: that the matrix as a whole reaches each family.  Under SAGEN_FP32_ONLY the forward sweeps run in the same child."""
    here = os.path.join(ROOT, 'tests', 'test_gpu_backward_ops.py')
    reached = set()
    for env in BO.SELECTIONS:
        for c in WGRAD_CASES:
            p = BO.wgrad_plan(c, env)
            reached.add(p.kernel + ('+fold' if p.fold > 1 else ''))
    assert reached == {'wgrad_ref_kernel', 'wgrad_kernel', 'wgrad3r_kernel', 'wgrad3_kernel', 'wgrad3_kernel+fold'}
    for env in BO.SELECTIONS[1:]:
        args, k = [here], 'wgrad_randomised_sweep'
        if 'SAGEN_FP32_ONLY' in env:
            args.append(os.path.join(ROOT, 'tests', 'test_gpu_ops.py'))
            k += ' or conv_2d_randomised_generic_geometry or conv3x3_stride1_randomised_geometry or deconv_2d_randomised_geometry'
        out = _child(env, args + ['-k', k], timeout=600)
        assert ' passed' in out and 'skipped' not in out and 'no tests ran' not in out, (env, out[-500:])


@pytest.mark.parametrize('switch', ['SAGEN_FP32_ONLY', 'SAGEN_NO_H2'])
def test_whole_network_gradients_on_the_advertised_fallbacks(T, switch):
    """The README's fallbacks end to end: every variable's gradient of audio+video at B = 2 against fp64 autograd, at that test's bars."""
    node = os.path.join(ROOT, 'tests', 'test_gpu_backward.py') + '::test_every_variable_gradient_matches_fp64_autograd[encoders4-2-5-1]'
    out = _child({switch: '1'}, [node], timeout=900)
    assert '1 passed' in out, out[-500:]


def test_wgrad_without_scratch_runs_one_pixel_range(T):
    """include/sagen.h: the scratch is optional; without one (whatever scratch_bytes says) the call runs one pixel range."""
    from spatialaudiogen_amd import _lib
    c = next(c for c in WGRAD_CASES if c.name == 'fc-3000')
    G, D = BO.wgrad_operands(c, integers=True)
    gd, dd = T.as_tensor(G).cuda(), T.as_tensor(D).cuda()
    out = _nan(T, c.kh, c.kw, c.Cg, c.Cd)
    l = _lib.lib()
    rc = l.sagen_wgrad(gd.data_ptr(), c.B, c.HG, c.WG, c.Cg, dd.data_ptr(), c.Hd, c.Wd, c.Cd, c.kh, c.kw, c.sh, c.sw, c.h0, c.w0, out.data_ptr(),
                       None, l.sagen_wgrad_scratch_bytes(c.kh, c.kw, c.Cg, c.Cd), None)
    T.cuda.synchronize()
    assert rc == 0, l.sagen_last_error()
    assert np.array_equal(out.cpu().numpy(), BO.wgrad_ref(G, D, 1, 1).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------------
# sagen_conv2d_bwd_data
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', DGRAD_CASES, ids=lambda c: c.name)
def test_dgrad_randomised_sweep(T, case):
    """dx against fp64 autograd of tf.nn.convolution at 2e-5; the rows / columns a strided VALID conv never reads exactly 0; integer
    known answers bit for bit; dx prefilled with NaN."""
    from spatialaudiogen_amd import ops
    c = case
    w, dy = BO.dgrad_operands(c)
    ref = BO.dgrad_ref((c.B, c.H, c.W, c.cin), w, (c.sh, c.sw), c.padding, dy)
    out, guard = _guarded(T, c.B, c.H, c.W, c.cin)
    dx = ops.conv_2d_bwd_data(T.as_tensor(dy).cuda(), T.as_tensor(w).cuda(), (c.H, c.W), (c.sh, c.sw), c.padding, out=out).cpu().numpy()
    assert bool(T.isnan(guard).all()), 'written past the output'
    assert np.isfinite(dx).all(), ('elements not written', int((~np.isfinite(dx)).sum()))
    r0, c0 = BO.dgrad_unread(c)
    assert np.all(dx[:, r0:] == 0) and np.all(dx[:, :, c0:] == 0), 'rows from %d / columns from %d are read by no window' % (r0, c0)
    err = rel_rms_err(dx, ref)
    print('%s: rel-RMS %.2e' % (c.name, err))
    assert err < 2e-5, err
    n = c.kh * c.kw * c.cout
    if BO.integer_exact(n):
        wi, dyi = BO.dgrad_operands(c, integers=True)
        ref_i = BO.dgrad_ref((c.B, c.H, c.W, c.cin), wi, (c.sh, c.sw), c.padding, dyi).astype(np.float32)
        dxi = ops.conv_2d_bwd_data(T.as_tensor(dyi).cuda(), T.as_tensor(wi).cuda(), (c.H, c.W), (c.sh, c.sw), c.padding,
                                   out=_nan(T, c.B, c.H, c.W, c.cin)).cpu().numpy()
        bad = np.argwhere(dxi != ref_i)
        assert bad.size == 0, ('integer known answer', len(bad), [(tuple(b), float(dxi[tuple(b)]), float(ref_i[tuple(b)])) for b in bad[:8]])


# ------------------------------------------------------------------------------------------------------------------------
# sagen_bn_bwd
# ------------------------------------------------------------------------------------------------------------------------
def _bn_cases():
    cases, k = [], 0
    for C_ in BO.BN_LEGAL_C:
        big = {4: 6272 * 2, 64: 6272 * 3, 256: 6272, 1024: 6272}.get(C_)
        for npix in [1, 3, 17, 1001] + ([big] if big else []):
            cases.append((C_, npix, bool(k & 1), bool(k & 2), bool(k & 4)))          # gb, act, want_dz: all eight combinations in turn
            k += 1
    return cases


@pytest.mark.parametrize('case', _bn_cases(), ids=lambda c: 'C%d-n%d-gb%d-act%d-dz%d' % c)
def test_bn_bwd_sweep(T, case):
    """Every legal channel count, pixel counts from 1, each optional operand present and absent, gamma of both signs with one channel
    at 0, one channel of constant y (variance 0: eps decides).  Bars: dy 2e-5, dgamma and dbeta 1e-5, dz exact."""
    from spatialaudiogen_amd import ops
    C_, npix, has_gb, has_act, want_dz = case
    r = rng(C_ * 131 + npix)
    y = (r.normal(size=(npix, C_)) * r.uniform(0.5, 2.0, size=C_) + r.normal(size=C_)).astype(np.float32)
    y[:, C_ // 2] = np.float32(0.75)                                        # constant channel
    gamma = (r.uniform(0.5, 1.5, size=C_) * r.choice([-1.0, 1.0], size=C_)).astype(np.float32)
    gamma[0], gamma[1], gamma[C_ - 1] = 1.25, -0.75, 0.0
    beta = r.normal(0, 0.2, size=C_).astype(np.float32)
    ga = r.normal(size=y.shape).astype(np.float32)
    gb = r.normal(size=y.shape).astype(np.float32) if has_gb else None
    res = r.normal(size=y.shape).astype(np.float32) if has_act else None
    dy_ref, dg_ref, db_ref, act = BO.bn_bwd_ref(ga, gb, res, y, gamma, beta, relu=has_act)
    dev = lambda a: None if a is None else T.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    yd = dev(y)
    stats = T.stack([yd.double().sum(0), (yd.double() ** 2).sum(0)]).contiguous()
    outs = (_nan(T, npix, C_), _nan(T, C_), _nan(T, C_)) + ((_nan(T, npix, C_),) if want_dz else ())
    got = ops.bn_bwd(dev(ga), yd, stats, dev(gamma), dev(beta), act=dev(act), g2=dev(gb), want_dz=want_dz, out=outs)
    got = [t.cpu().numpy() for t in got]
    assert all(np.isfinite(t).all() for t in got), 'elements not written'
    errs = rel_rms_err(got[0], dy_ref), rel_rms_err(got[1], dg_ref), rel_rms_err(got[2], db_ref)
    print('bn_bwd C=%d n=%d: dy %.2e dgamma %.2e dbeta %.2e' % ((C_, npix) + errs))
    assert errs[0] < 2e-5 and errs[1] < 1e-5 and errs[2] < 1e-5, errs
    assert np.all(got[0][:, C_ - 1] == 0)                                   # gamma = 0: nothing reaches y
    if want_dz:
        dz = ga + gb if has_gb else ga
        assert np.array_equal(got[3], dz * (np.asarray(act, np.float32) > 0) if has_act else dz)


def test_bn_bwd_with_64_reduction_blocks(T):
    _child({'SAGEN_RED_BLOCKS': '64'}, [os.path.join(ROOT, 'tests', 'test_gpu_backward_ops.py'), '-k', 'bn_bwd_sweep'], timeout=600)


# ------------------------------------------------------------------------------------------------------------------------
# sagen_maxpool3x3s2_bwd
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 2, 2, 4), (1, 3, 2, 12), (3, 2, 5, 64), (2, 7, 8, 128), (2, 12, 9, 12), (1, 11, 14, 4), (2, 6, 6, 64),
                                   (1, 5, 5, 128)], ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_bwd_sweep(T, shape):
    """Odd and even sizes down to 2x2, channel counts off the path's, a second incoming gradient, gammas of both signs: 1e-6."""
    from spatialaudiogen_amd import ops
    from oracle.torch_ref import bn_train, _same
    import torch.nn.functional as F
    B, H, W, C_ = shape
    r = rng(B * 1000 + H * 100 + W * 10 + C_)
    y0 = r.normal(size=shape).astype(np.float32)
    gamma = (r.uniform(0.5, 1.5, size=C_) * np.where(np.arange(C_) % 3 == 1, -1.0, 1.0)).astype(np.float32)
    beta = r.normal(0, 0.3, size=C_).astype(np.float32)
    yd = T.as_tensor(y0).cuda()
    stats = T.stack([yd.double().sum((0, 1, 2)), (yd.double() ** 2).sum((0, 1, 2))]).contiguous()
    gd, bd = T.as_tensor(gamma).cuda(), T.as_tensor(beta).cuda()
    sc, sh = ops.bn_finalize(stats, shape, gd, bd)
    pooled = ops.maxpool3x3s2(yd, sc, sh)
    g1, g2 = r.normal(size=tuple(pooled.shape)).astype(np.float32), r.normal(size=tuple(pooled.shape)).astype(np.float32)
    yt = T.as_tensor(y0, dtype=T.float64).permute(0, 3, 1, 2)
    z = bn_train(yt, T.as_tensor(gamma, dtype=T.float64), T.as_tensor(beta, dtype=T.float64)).detach().requires_grad_(True)
    (pt, pb), (pl, pr) = _same(H, 3, 2), _same(W, 3, 2)
    p = F.max_pool2d(F.pad(F.relu(z), (pl, pr, pt, pb), value=float('-inf')), 3, 2)
    assert rel_rms_err(pooled.cpu().numpy(), p.detach().permute(0, 2, 3, 1).numpy()) < 1e-5
    p.backward(T.as_tensor(g1.astype(np.float64) + g2, dtype=T.float64).permute(0, 3, 1, 2))
    dz = ops.maxpool3x3s2_bwd(yd, stats, gd, bd, pooled, T.as_tensor(g1).cuda(), g2=T.as_tensor(g2).cuda()).cpu().numpy()
    err = rel_rms_err(dz, z.grad.permute(0, 2, 3, 1).numpy())
    assert err < 1e-6, err


# ------------------------------------------------------------------------------------------------------------------------
# sagen_mask_istft_mix_bwd, sagen_stft_loss_grad, sagen_adam_update
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,K', [(1, 64), (3, 16), (5, 32), (1, 16), (3, 64)])
def test_mask_istft_mix_adjoint_sweep(T, B, K):
    """The adjoint of the separation tail for every supported track count and odd batches, against fp64 autograd of its restatement
    (test_gpu_backward._mix_ref), at the bars of test_mask_istft_mix_adjoint: 2e-5; frames outside the window exactly 0."""
    from spatialaudiogen_amd import ops
    from test_gpu_backward import _mix_ref
    r = rng(300 + 10 * B + K)
    audio = r.normal(size=(B, 52799)).astype(np.float32)
    dmask = r.normal(size=(B, 28, 1024, K)).astype(np.float32)
    coeffs = (0.3 * r.normal(size=(B, 3, 3, K + 1))).astype(np.float32)
    dpred = r.normal(size=(B, 4800, 3)).astype(np.float32)
    _, spec = ops.stft_mag(T.as_tensor(audio).cuda(), 46, 173, 89, 117)
    sp = spec.cpu().double()
    half = T.complex(sp[..., 0], sp[..., 1])
    full = T.cat([half, T.conj(half[:, :, 1:512].flip(-1))], -1)
    dm = T.as_tensor(dmask, dtype=T.float64).requires_grad_(True)
    co = T.as_tensor(coeffs, dtype=T.float64).requires_grad_(True)
    _mix_ref(T, dm, full, co).backward(T.as_tensor(dpred, dtype=T.float64))
    dd, dc = ops.mask_istft_mix_bwd(T.as_tensor(dmask).cuda(), spec, T.as_tensor(coeffs).cuda(), T.as_tensor(dpred).cuda())
    dd, dc = dd.cpu().numpy(), dc.cpu().numpy()
    assert rel_rms_err(dc, co.grad.numpy()) < 2e-5, rel_rms_err(dc, co.grad.numpy())
    assert rel_rms_err(dd, dm.grad.numpy()) < 2e-5, rel_rms_err(dd, dm.grad.numpy())
    assert np.all(dd[:, 0] == 0) and np.all(dd[:, 24:] == 0)


@pytest.mark.parametrize('B', [1, 5, 32])
def test_stft_loss_grad_sweep(T, B):
    """Loss and the WHOLE gradient tensor against fp64 autograd of oracle/torch_ref.stft_loss_torch, with masks that zero channels,
    without a mask, and with only one of the two outputs asked for.  Bars as test_stft_loss_value_and_gradient holds them: loss 1e-5
    relative, gradient 1e-4 of its largest element."""
    from oracle.torch_ref import stft_loss_torch
    from spatialaudiogen_amd import _lib
    r = rng(40 + B)
    gt = 0.3 * r.normal(size=(B, 4800, 3))
    pred = gt * r.uniform(0.5, 1.2, size=(B, 1, 3)) + 0.05 * r.normal(size=gt.shape)
    gt, pred = gt.astype(np.float32), pred.astype(np.float32)
    mask = (r.uniform(size=(B, 3)) > 0.4).astype(np.float32)
    mask[0, 1] = 0.0
    l = _lib.lib()
    pd, gd = T.as_tensor(pred).cuda(), T.as_tensor(gt).cuda()
    for mk in (None, mask, np.zeros((B, 3), np.float32)):
        pt = T.as_tensor(pred, dtype=T.float64).requires_grad_(True)
        loss_ref = stft_loss_torch(pt, T.as_tensor(gt, dtype=T.float64), None if mk is None else T.as_tensor(mk, dtype=T.float64))
        loss_ref.backward()
        g_ref, loss_ref = pt.grad.numpy(), float(loss_ref.detach())
        md = None if mk is None else T.as_tensor(mk).cuda()
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        for want_grad, want_loss in ((True, True), (True, False), (False, True)):
            grad = _nan(T, B, 4800, 3) if want_grad else None
            loss = T.zeros(1, dtype=T.float64, device='cuda') if want_loss else None
            _lib.check(l.sagen_stft_loss_grad(ptr(pd), ptr(gd), ptr(md), B, ptr(grad), ptr(loss), C.c_void_p(T.cuda.current_stream().cuda_stream)))
            if want_loss:
                assert abs(float(loss[0]) - loss_ref) <= 1e-5 * abs(loss_ref), (float(loss[0]), loss_ref)
            if want_grad:
                g = grad.cpu().numpy()
                assert np.isfinite(g).all(), 'elements not written'
                assert np.abs(g - g_ref).max() <= 1e-4 * np.abs(g_ref).max() + 1e-9, (np.abs(g - g_ref).max(), np.abs(g_ref).max())
                if mk is not None:
                    assert np.all(g.transpose(0, 2, 1)[mk == 0] == 0)        # masked channels do not train


@pytest.mark.parametrize('n', [4, 12, 1020, 2 ** 20 + 4])
def test_adam_update_sweep(T, n):
    """One bucket of n floats (tails of every vector width), gradients scaled by 1 / 3 first, at step 1 and at a step count where
    lr_t has converged to lr; against the oracle's TF formulation at the bar of test_adam_bucket_matches_tf_formulation, 2e-6."""
    from oracle import np_oracle as O
    from spatialaudiogen_amd import _lib
    from spatialaudiogen_amd.train import adam_lr_t, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON
    r = rng(n)
    for t, lr in ((1, 1e-2), (20000, 1e-4)):
        p = r.normal(size=n).astype(np.float32)
        g = (r.normal(size=n) * 10.0 ** r.integers(-3, 2, size=n)).astype(np.float32)
        m = (0.1 * r.normal(size=n)).astype(np.float32) if t > 1 else np.zeros(n, np.float32)
        v = (0.01 * r.uniform(size=n)).astype(np.float32) if t > 1 else np.zeros(n, np.float32)
        scale = 1.0 / 3.0
        ref = O.adam_tf(p.astype(np.float64), g.astype(np.float64) * np.float32(scale), m.astype(np.float64), v.astype(np.float64), t, lr)
        lr_t = adam_lr_t(t, lr)
        if t > 1:
            assert abs(lr_t / lr - 1) < 1e-6                                    # (beta2^t has vanished)
        # guard elements behind the bucket: the update must not touch them
        dev = [T.cat([T.as_tensor(a), T.full((4,), 7.0)]).cuda() for a in (p, g, m, v)]
        ptr = lambda x: C.c_void_p(x.data_ptr())
        _lib.check(_lib.lib().sagen_adam_update(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), n, lr_t, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON,
                                                scale, C.c_void_p(T.cuda.current_stream().cuda_stream)))
        got = [x.cpu().numpy() for x in dev]
        for k, name in ((0, 'params'), (2, 'm'), (3, 'v')):
            assert np.all(got[k][n:] == 7.0), name
            assert rel_rms_err(got[k][:n], ref[{0: 0, 2: 1, 3: 2}[k]]) < 2e-6, (name, t, rel_rms_err(got[k][:n], ref[{0: 0, 2: 1, 3: 2}[k]]))
        assert np.array_equal(got[1][:n], g)


# ------------------------------------------------------------------------------------------------------------------------
# refusals: a negative status and a message, decided on the host, outputs untouched
# ------------------------------------------------------------------------------------------------------------------------
def test_unsupported_calls_are_refused_with_outputs_untouched(T):
    from spatialaudiogen_amd import ops
    from spatialaudiogen_amd._lib import SagenError, lib

    def refused(fn, outs):
        with pytest.raises(SagenError) as e:
            fn()
        T.cuda.synchronize()
        assert e.value.code < 0 and len(str(e.value)) > 20, str(e.value)
        for o in outs:
            assert bool(T.isnan(o).all()), 'a refused call wrote to its output'

    z = lambda *s: T.zeros(*s, dtype=T.float32, device='cuda')
    for C_ in (12, 6):                                                          # bn: C must be 4 * a divisor of 256
        outs = (_nan(T, 5, C_), _nan(T, C_), _nan(T, C_))
        refused(lambda: ops.bn_bwd(z(5, C_), z(5, C_), T.zeros(2, C_, dtype=T.float64, device='cuda'), z(C_), z(C_), out=outs), outs)
    for cg, cd in ((8, 6), (6, 8), (64, 30), (30, 64)):                         # wgrad: cg, cd multiples of 4
        out = _nan(T, 3, 3, cg, cd)
        for split in (True, False):
            refused(lambda: ops.wgrad(z(2, 5, 5, cg), z(2, 5, 5, cd), 3, 3, (1, 1), (-1, -1), split=split, out=out), [out])
    # an operand offset by 4 bytes
    l = lib()
    g, d, out = z(2 * 5 * 5 * 8 + 4), z(2 * 5 * 5 * 8 + 4), _nan(T, 3, 3, 8, 8)
    for go, do in ((4, 0), (0, 4)):
        rc = l.sagen_wgrad(g.data_ptr() + go, 2, 5, 5, 8, d.data_ptr() + do, 5, 5, 8, 3, 3, 1, 1, -1, -1, out.data_ptr(), None, 0, None)
        T.cuda.synchronize()
        assert rc < 0 and b'aligned' in l.sagen_last_error() and bool(T.isnan(out).all()), (rc, l.sagen_last_error())
    # dgrad: cout a power of two; strided SAME with padding before
    out = _nan(T, 2, 6, 6, 8)
    refused(lambda: ops.conv_2d_bwd_data(z(2, 6, 6, 24), z(3, 3, 8, 24), (6, 6), 1, 'SAME', out=out), [out])
    out = _nan(T, 2, 7, 7, 8)
    refused(lambda: ops.conv_2d_bwd_data(z(2, 4, 4, 16), z(3, 3, 8, 16), (7, 7), 2, 'SAME', out=out), [out])        # pad before = 1
