"""The kernels behind the numbers `evaluate --all_metrics` reports, op by op through the C ABI, against the plain fp64 references and
the derived bounds of eval_oracle.py (its docstring holds the derivations; test_eval_oracle_host.py proves the references, the case
lists and that each bound sees its mutant).  The companion of test_gpu_spectral_ops.py for csrc/eval.hip (eval_time_kernel, the LSD's
DFT on igemm_kernel, eval_lsd_reduce_kernel), csrc/evalx.hip (evalx_mel_kernel, evalx_env_kernel, evalx_emd_kernel over emd_core.h) and
the two power-map kernel pairs of csrc/elementwise.hip.  With SAGEN_LIB naming the CPU twin the power-map and EMD tests run on host
tensors (test_cpu_twin_ops.py); the twin has no sagen_eval_metrics and no sagen_eval_mel_env.

Every output element of every call is compared; the only entries left out are the named non-finite ones of a poisoned case, which must be
NaN.  Outputs the test allocates itself are prefilled with NaN and carry a NaN guard that must survive.  Nothing here reads or writes
outside live memory and no test provokes a fault: refusals and the EMD solver's `not converged` are ordinary return paths.  Each test
prints the worst fraction of its bound per family as 'EVALOPS {json}' (measurements, not bars).

sagen_eval_metrics / sagen_eval_metrics_c: B in {1, 2, 5, 16}, C = 3 on both entries (bit for bit the same), C = 5 on the _c entry;
the families of eval_oracle.metric_slots() spread over the (b, c) entries.  stft distance, MSE and both power sums within 40 u of the
reference, SNR within 2.2e-5 dB + 8 u |snr|, LSD within the per-frame bound; exact zeros where the difference is zero, and for an impulse
at 4096 / 4799 a stft distance of exactly 0 beside a non-zero MSE.  A NaN in one (b, c) reaches that entry's four values and the
prediction's power sum only; a second call on the same scratch with other data equals a call on a fresh scratch bit for bit.

sagen_eval_mel_env: the shapes of eval_oracle.MEL_SHAPES (C in {1, 2, 3, 4, 5, 8}, B = 1, and 13 x 5 = 65 entries = two blocks of
evalx_finish_kernel), neighbouring channels carrying different families; C = 9 and C = 0 refused with the outputs untouched.

sagen_eval_emd: n in {1, 2, 63, 64, 65, 84, 96} nodes, the families of eval_oracle.emd_cases(n) (more than 64 sources with 1, 4 and
n - 65 sinks, and swapped; uniform against concentrated; the rerouting branch; ties) within 1e-7 |ref| + 1e-12 of the LP and within 1e-12
relative of the serial core (the CPU twin's EmdSerial); 97 refused; a NaN map among good ones; blocked costs raise the counter by the
number of problems that had mass to move, and it is not cleared between calls.

sagen_power_map / sagen_power_map_batched: the cases of eval_oracle.pm_cases() - the 30 and 5 degree matrices and random [P, 4] with
P in {1, 2, 83, 255, 256, 257}; T in {1, 3, 255, 256, 257, 4800, 262657}; 1, 2 and 13 chunks with silent ones between loud ones; plane
waves toward a pole, an equator and a generic node, two plane waves, DC on W, W only (a flat map), noise x 1e-4 and x 30 - within
2^-23 ref[p] + 2^-22 max(ref) elementwise, nulls included, cross-checked against sagen_power_map_windows at stride 1, the single-map
entry with rms[P + 24 ..] poisoned and untouched.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import eval_oracle as E
from util import ensure_lib

pytestmark = pytest.mark.gpu

TWIN = os.path.basename(os.environ.get('SAGEN_LIB', '')) == 'libsagen_cpu.so'
U = E.U


@pytest.fixture(scope='module')
def T():
    import torch
    if not TWIN:
        assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    ensure_lib()
    return torch


def _dev(T, a, dtype=np.float32):
    t = T.as_tensor(np.ascontiguousarray(a, dtype=dtype))
    return t if TWIN else t.cuda()


def _nan(T, n, dtype=None):
    return T.full((int(n),), float('nan'), dtype=dtype or T.float32, device='cpu' if TWIN else 'cuda')


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(T):
    return None if TWIN else C.c_void_p(T.cuda.current_stream().cuda_stream)


def _report(**kw):
    print('EVALOPS ' + json.dumps(kw, sort_keys=True))


def _frac(err, bound):
    """Worst error as a fraction of its bound (0 / 0 = 0: an exact value under a zero bound)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


# ---- sagen_eval_metrics / sagen_eval_metrics_c ------------------------------------------------------------------------------------
def _metrics(T, pred, gt, entry, scratch=None):
    """(ps [4, B, C] float32, pw [2] fp64, scratch) through the ABI; entry '3' = sagen_eval_metrics, 'c' = sagen_eval_metrics_c."""
    from spatialaudiogen_amd import _lib
    l = _lib.lib()
    B, _, Cn = pred.shape
    nbytes = int(l.sagen_eval_scratch_bytes(B) if entry == '3' else l.sagen_eval_scratch_bytes_c(B, Cn))
    if scratch is None:
        scratch = _nan(T, nbytes // 4 + 64)
        _lib.check(l.sagen_eval_init(_ptr(scratch), nbytes, B, _stream(T)))
    p, g = _dev(T, pred), _dev(T, gt)
    ps, pw = _nan(T, (4 + 1) * B * Cn), _nan(T, 4, T.float64)
    if entry == '3':
        assert Cn == 3
        _lib.check(l.sagen_eval_metrics(_ptr(p), _ptr(g), B, _ptr(ps), _ptr(pw), _ptr(scratch), nbytes, _stream(T)))
    else:
        _lib.check(l.sagen_eval_metrics_c(_ptr(p), _ptr(g), B, Cn, _ptr(ps), _ptr(pw), _ptr(scratch), nbytes, _stream(T)))
    ps, pw = ps.cpu().numpy(), pw.cpu().numpy()
    assert np.isnan(ps[4 * B * Cn:]).all() and np.isnan(pw[2:]).all() and np.isnan(scratch[nbytes // 4:].cpu().numpy()).all()
    return ps[:4 * B * Cn].reshape(4, B, Cn), pw[:2], scratch


def _check_metrics(ps, pw, pred, gt, names, tag):
    B, _, Cn = pred.shape
    tm = E.time_metrics_ref(pred, gt)
    lsd, lsd_bound = E.lsd_ref(pred, gt, with_bound=True)
    assert np.isfinite(ps).all() and np.isfinite(pw).all()
    checks = (('stft', ps[0], tm['stft'], E.SUM_C * U * tm['stft']), ('lsd', ps[1], lsd, lsd_bound),
              ('mse', ps[2], tm['mse'], E.SUM_C * U * tm['mse']), ('snr', ps[3], tm['snr'], E.snr_bound(tm['snr'])),
              ('pw', pw, tm['pw'], E.SUM_C * U * tm['pw']))
    fr = {}
    for key, got, ref, bound in checks:
        err = np.abs(got.astype(np.float64) - ref)
        fr[key] = _frac(err, bound)
        worst = int(np.argmax(err - bound))
        print('%s %s worst %.3f of its bound (%s)' % (tag, key, fr[key], names[worst] if key != 'pw' else 'sums'))
    _report(op='eval_metrics', case=tag, **fr)
    for key, got, ref, bound in checks:
        err = np.abs(got.astype(np.float64) - ref)
        bad = np.argwhere(err > bound)
        assert len(bad) == 0, (tag, key, [(names[int(np.ravel_multi_index(tuple(i), err.shape))] if key != 'pw' else 'sums',
                                          float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in bad[:4]])
    for i, name in enumerate(names):
        b, c = divmod(i, Cn)
        if name in ('silent_both', 'identical'):
            assert ps[0, b, c] == 0 and ps[2, b, c] == 0, (tag, name)
        if name == 'silent_both':
            assert ps[1, b, c] == 0 and ps[3, b, c] == 0, (tag, name)
        if name.startswith('imp_') and name.endswith(('_4096', '_4799')):       # beyond every stft_for_loss window
            assert ps[0, b, c] == 0 and ps[2, b, c] > 0, (tag, name, ps[0, b, c], ps[2, b, c])
        if name in ('beyond_lsd_frames',):
            assert ps[1, b, c] == 0 and ps[2, b, c] > 0, (tag, name)


@pytest.mark.parametrize('B', [1, 2, 5, 16])
def test_eval_metrics_families(T, B):
    pred, gt, names = E.metric_batch(B, 3, E.METRIC_STARTS[B])
    ps3, pw3, _ = _metrics(T, pred, gt, '3')
    psc, pwc, _ = _metrics(T, pred, gt, 'c')
    assert np.array_equal(ps3, psc) and np.array_equal(pw3, pwc)                 # channels = 3 computes exactly what the first entry computes
    _check_metrics(ps3, pw3, pred, gt, names, 'B%d_C3' % B)
    pred, gt, names = E.metric_batch(B, 5, E.METRIC_STARTS[B] + 3)
    ps5, pw5, _ = _metrics(T, pred, gt, 'c')
    _check_metrics(ps5, pw5, pred, gt, names, 'B%d_C5' % B)


def test_eval_metrics_through_the_model_entry(T):
    """SptAudioGen.evaluation_ps (the driver's route, with its cached scratch) gives the bits of the direct call."""
    from spatialaudiogen_amd.model import SptAudioGen
    pred, gt, names = E.metric_batch(5, 3, 17)
    net = SptAudioGen(1, encoders=['audio'], separation='unet_mask')
    ps, pw = net.evaluation_ps(_dev(T, pred), _dev(T, gt))
    ref_ps, ref_pw, _ = _metrics(T, pred, gt, '3')
    assert np.array_equal(ps.cpu().numpy(), ref_ps) and np.array_equal(pw.cpu().numpy(), ref_pw)


@pytest.mark.parametrize('Cn', [3, 5])
def test_eval_metrics_nan_stays_in_its_entry(T, Cn):
    pred, gt, names = E.metric_batch(2, Cn, 4)
    clean, clean_pw, _ = _metrics(T, pred, gt, 'c')
    bad = pred.copy()
    bad[1, 100, 1] = np.nan                                                      # inside stft window 0 and LSD frame 0
    ps, pw, _ = _metrics(T, bad, gt, 'c')
    assert np.isnan(ps[:, 1, 1]).all() and np.isnan(pw[0])
    keep = np.ones((2, Cn), bool)
    keep[1, 1] = False
    assert np.array_equal(ps[:, keep], clean[:, keep]) and pw[1] == clean_pw[1]


def test_eval_metrics_second_call_on_the_same_scratch(T):
    """The DFT matrix is initialised once; frames and spectra are rewritten by every call."""
    pa, ga, _ = E.metric_batch(2, 3, 5)
    pb, gb, _ = E.metric_batch(2, 3, 29)
    first, first_pw, scratch = _metrics(T, pa, ga, '3')
    second, second_pw, _ = _metrics(T, pb, gb, '3', scratch=scratch)
    fresh, fresh_pw, _ = _metrics(T, pb, gb, '3')
    assert np.array_equal(second, fresh) and np.array_equal(second_pw, fresh_pw) and not np.array_equal(first, second)
    again, again_pw, _ = _metrics(T, pa, ga, '3', scratch=scratch)
    assert np.array_equal(again, first) and np.array_equal(again_pw, first_pw)


# ---- sagen_eval_mel_env -------------------------------------------------------------------------------------------------------------
_MEL_REF = {}


def _mel_ref(slot):
    name, p, g, imp = slot
    if name not in _MEL_REF:
        _MEL_REF[name] = E.mel_lsd_ref(p, g, with_bound=True) + E.env_ref(p, g, imp)
    return _MEL_REF[name]


def _mel_env(T, pred, gt, channels=None):
    from spatialaudiogen_amd import _lib
    l = _lib.lib()
    B, _, Cn = pred.shape
    n = B * Cn
    mel, env = _nan(T, n + 8), _nan(T, n + 8)
    nbytes = int(l.sagen_eval_mel_env_scratch_bytes(B, Cn))
    scratch = _nan(T, nbytes // 4 + 64)
    p, g = _dev(T, pred), _dev(T, gt)
    rc = l.sagen_eval_mel_env(_ptr(p), _ptr(g), B, Cn if channels is None else channels, _ptr(mel), _ptr(env), _ptr(scratch), nbytes + 256,
                              _stream(T))
    mel, env = mel.cpu().numpy(), env.cpu().numpy()
    assert np.isnan(mel[n:]).all() and np.isnan(env[n:]).all() and np.isnan(scratch[nbytes // 4:].cpu().numpy()).all()
    return rc, mel[:n], env[:n]


@pytest.mark.parametrize('shape', E.MEL_SHAPES, ids=lambda s: 'B%d_C%d' % s[:2])
def test_eval_mel_env_families(T, shape):
    B, Cn, start = shape
    pred, gt, meta = E.mel_batch(B, Cn, start)
    rc, mel, env = _mel_env(T, pred, gt)
    rc2, mel2, env2 = _mel_env(T, pred, gt)
    assert rc == 0 and rc2 == 0 and np.array_equal(mel, mel2) and np.array_equal(env, env2)
    slots = {s[0]: s for s in E.mel_slots()}
    worst = {}
    fails = []
    for i, (name, imp) in enumerate(meta):
        mref, mb, eref, eb = _mel_ref(slots[name])
        fm, fe = _frac(abs(float(mel[i]) - mref), mb), _frac(abs(float(env[i]) - eref), eb)
        fam = 'impulse' if imp else name
        worst[fam] = (max(worst.get(fam, (0, 0))[0], fm), max(worst.get(fam, (0, 0))[1], fe))
        if not (fm <= 1 and fe <= 1):
            fails.append((i, name, float(mel[i]), mref, mb, float(env[i]), eref, eb))
        if name == 'silent_both':
            assert mel[i] == 0 and env[i] == 0
        if name == 'identical':
            assert env[i] == 0
    for fam, (fm, fe) in sorted(worst.items()):
        _report(op='eval_mel_env', case='B%d_C%d' % (B, Cn), family=fam, mel=fm, env=fe)
    assert not fails, fails[:4]


@pytest.mark.parametrize('channels', [9, 0])
def test_eval_mel_env_refuses_other_channel_counts(T, channels):
    pred, gt, _ = E.mel_batch(1, 8, 0)
    rc, mel, env = _mel_env(T, pred, gt, channels=channels)
    assert rc == -3 and np.isnan(mel).all() and np.isnan(env).all()


# ---- sagen_eval_emd -------------------------------------------------------------------------------------------------------------------
def _emd(T, P, Q, cost, counter=None, nodes=None):
    from spatialaudiogen_amd import _lib
    l = _lib.lib()
    n, nd = P.shape
    out = _nan(T, 2 * n + 2, T.float64)
    nc = T.zeros(2, dtype=T.int32, device=out.device) if counter is None else counter
    p, q, c = _dev(T, P), _dev(T, Q), _dev(T, cost, np.float64)
    rc = l.sagen_eval_emd(_ptr(p), _ptr(q), n, nd if nodes is None else nodes, _ptr(c), _ptr(out), _ptr(nc), _stream(T))
    out = out.cpu().numpy()
    assert np.isnan(out[2 * n:]).all() and int(nc[1]) == 0
    return rc, out[:2 * n].reshape(n, 2), nc


@pytest.fixture(scope='module')
def serial():
    """The CPU twin's EmdSerial as a ctypes library: the serial core the lane-parallel walk must equal."""
    from spatialaudiogen_amd import build
    from test_eval_metrics_host import _twin_emd
    lib = C.CDLL(build.build_cpu_twin())
    return lambda P, Q, cost: _twin_emd(lib, P, Q, cost)


@pytest.mark.parametrize('n', E.EMD_NODES)
def test_emd_families(T, serial, n):
    cost = E.emd_metric(n)
    cases = E.emd_cases(n)
    P, Q = np.stack([p for _, p, _ in cases]), np.stack([q for _, _, q in cases])
    rc, got, nc = _emd(T, P, Q, cost)
    rc2, again, _ = _emd(T, P, Q, cost)
    assert rc == 0 and rc2 == 0 and int(nc[0]) == 0 and np.array_equal(got, again)
    lp = E.emd_lp_refs(n)
    ser, ser_nc = serial(P, Q, cost)
    assert ser_nc == 0 and np.isfinite(got).all()
    f_lp = _frac(np.abs(got - lp), 1e-7 * np.abs(lp) + 1e-12)
    f_ser = _frac(np.abs(got - ser), 1e-12 * np.abs(ser))
    _report(op='eval_emd', nodes=n, cases=len(cases), lp=f_lp, serial=f_ser)
    for k, (name, _, _) in enumerate(cases):
        for v in range(2):
            assert abs(got[k, v] - lp[k, v]) <= 1e-7 * abs(lp[k, v]) + 1e-12, (n, name, v, got[k, v], lp[k, v])
            assert abs(got[k, v] - ser[k, v]) <= 1e-12 * abs(ser[k, v]), (n, name, v, got[k, v], ser[k, v])


def test_emd_refuses_97_nodes(T):
    P = np.full((2, 97), 0.5, np.float32)
    rc, got, nc = _emd(T, P, P, np.zeros((97, 97)))
    assert rc == -3 and np.isnan(got).all() and int(nc[0]) == 0


def test_emd_nan_map_among_good_ones(T):
    n = 65
    cost = E.emd_metric(n)
    cases = E.emd_cases(n)
    P, Q = np.stack([p for _, p, _ in cases]), np.stack([q for _, _, q in cases])
    _, clean, _ = _emd(T, P, Q, cost)
    P[2, 64] = np.nan                                                           # the one node of the second pass over the nodes
    Q[5, 0] = np.inf
    rc, got, nc = _emd(T, P, Q, cost)
    keep = np.ones(len(P), bool)
    keep[[2, 5]] = False
    assert rc == 0 and int(nc[0]) == 0 and np.isnan(got[[2, 5]]).all() and np.array_equal(got[keep], clean[keep])


def test_emd_blocked_costs_raise_the_counter(T):
    """Off-diagonal costs of 1e300 are the solver's "no path": every problem with mass to move returns through `not converged`, the
    others stay exact, and the counter is added to, not cleared."""
    p, q, cost, exp, count = E.emd_blocked_case()
    rc, got, nc = _emd(T, p, q, cost)
    assert rc == 0 and int(nc[0]) == count == 4
    assert np.all(np.abs(got - exp) <= 1e-12 * np.abs(exp)) and np.all(got[[0, 4]] == 0) and np.isfinite(got).all()
    rc, again, nc = _emd(T, p, q, cost, counter=nc)
    assert rc == 0 and int(nc[0]) == 2 * count and np.array_equal(again, got)


# ---- sagen_power_map / sagen_power_map_batched ----------------------------------------------------------------------------------------
def _power_map_single(T, ambi, sh):
    """sagen_power_map with rms[P + 24 ..] poisoned: the documented tail is all the call may touch."""
    from spatialaudiogen_amd import _lib
    P = len(sh)
    rms = _nan(T, P + 24 + 40)
    _lib.check(_lib.lib().sagen_power_map(_ptr(ambi), ambi.shape[0], _ptr(sh), P, _ptr(rms), _stream(T)))
    rms = rms.cpu().numpy()
    assert np.isnan(rms[P + 24:]).all()
    return rms[:P]


@pytest.mark.parametrize('case', E.pm_cases(), ids=lambda c: '%s_T%d_n%d' % c)
def test_power_map_families(T, case):
    from spatialaudiogen_amd import ops
    mesh, Tn, nchunks = case
    sh, names, ambi = E.pm_chunks(mesh, Tn, nchunks)
    ref = np.stack([E.power_map_ref(a, sh) for a in ambi])
    bound = E.power_map_bound(ref)
    assert np.isfinite(ref).all()
    a_dev, sh_dev = _dev(T, ambi), _dev(T, sh)
    batched = ops.power_map_batched(a_dev, sh_dev).cpu().numpy()
    single = np.stack([_power_map_single(T, a_dev[c], sh_dev) for c in range(nchunks)])
    windows = ops.power_map_windows(a_dev.reshape(-1, 4), sh_dev, 1, Tn).cpu().numpy()
    assert batched.shape == single.shape == windows.shape == ref.shape
    fails = []
    for entry, got in (('batched', batched), ('single', single), ('windows', windows)):
        assert np.isfinite(got).all(), entry
        err = np.abs(got.astype(np.float64) - ref)
        for c, name in enumerate(names):
            f = _frac(err[c], bound[c])
            _report(op='power_map', entry=entry, mesh=mesh, T=Tn, family=name, frac=f, at=int(np.argmax(err[c] - bound[c])),
                    err_over_max=float(err[c].max() / max(ref[c].max(), 1e-300)))
            if name == 'silent':
                assert not got[c].any(), (entry, c)
            if name == 'omni' and mesh in ('30', '5'):                           # W only: every node decodes the same signal
                assert np.all(got[c] == got[c][0]), (entry, c)
            if f > 1:
                fails.append((entry, name, f))
    assert not fails, fails
    assert np.all(np.abs(batched.astype(np.float64) - windows) <= 2 * bound) and np.all(np.abs(single.astype(np.float64) - windows) <= 2 * bound)
