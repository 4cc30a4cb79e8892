"""--all_metrics on the host (no GPU): the fp64 restatements of eval.py's host metrics against known answers, the column list of
eval.py:125-132, the CLI flag, the new entries' argument checks, and the exact EMD solver core (csrc/emd_core.h, run by the CPU twin
on host pointers) against an LP solver."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import metric_oracle as mo  # noqa: E402


# ---- the metric definitions: known answers ----------------------------------------------------------------------------------
def test_hilbert_kernel_matches_scipy():
    from scipy.signal import hilbert
    rng = np.random.default_rng(0)
    x = rng.standard_normal(4800)
    g = mo.hilbert_kernel(4800)
    hx = np.array([np.dot(np.roll(g[::-1], n + 1), x) for n in range(0, 4800, 97)])      # sum_m g[(n - m) mod N] x[m]
    assert np.allclose(hx, np.imag(hilbert(x))[::97], atol=1e-9)
    assert np.all(g[::2] == 0)


def test_envelope_of_a_periodic_tone_is_its_amplitude():
    n = np.arange(4800)
    x = 0.7 * np.sin(2 * np.pi * 25 * n / 4800 + 0.3)
    assert np.allclose(mo.envelope(x), 0.7, atol=1e-9)
    gt = np.stack([x, 2 * x, 0 * x], 1)
    assert np.allclose(mo.env_mse(gt, gt), 0.0)
    assert np.allclose(mo.env_mse(0.5 * gt, gt), [0.35, 0.7, 0.0], atol=1e-9)


def test_mel_basis_shape_support_and_peaks():
    W = mo.mel_basis()
    assert W.shape == (128, 1025)
    assert np.all(W[:, 513:] == 0) and np.any(W[:, 512] == 0)
    edges = mo.mel_to_hz(np.linspace(0, mo.hz_to_mel(12000.0), 130))
    freqs = np.linspace(0, 24000, 1025)
    for i in range(128):
        # the triangle peaks at its centre edge: the largest weight sits at the bin nearest to edges[i + 1]
        nz = np.nonzero(W[i])[0]
        if len(nz):
            assert abs(freqs[np.argmax(W[i])] - edges[i + 1]) <= freqs[1]
        peak = 2.0 / (edges[i + 2] - edges[i])
        assert W[i].max() <= peak * (1 + 1e-12)
    assert abs(mo.hz_to_mel(1000.0) - 15.0) < 1e-12 and abs(mo.mel_to_hz(mo.hz_to_mel(7000.0)) - 7000.0) < 1e-9


def test_mel_lsd_zero_for_identical_and_positive_otherwise():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4800, 3)) * 0.1
    assert np.allclose(mo.mel_lsd(x, x), 0)
    d = mo.mel_lsd(x, 2 * x)                                  # a gain of 2 is +6.02 dB wherever the spectrum dominates the floor
    assert np.all(d > 5.5) and np.all(d < 6.1)
    assert mo.melspectrogram(x[:, 0]).shape == (128, 10)


def test_emd_known_answers():
    Cm, _, _ = mo.angular_distance_ref(30.0)
    assert Cm.shape == (84, 84) and abs(Cm.max() - np.pi) < 1e-12
    rng = np.random.default_rng(2)
    p = rng.random(84)
    assert abs(mo.emd_hat(p, p, Cm)) < 1e-12
    # a unit mass moved one mesh step along the equator (row 3 of 7): pi / 6
    a, b = np.zeros(84), np.zeros(84)
    a[3 * 12 + 4], b[3 * 12 + 5] = 1.0, 1.0
    assert abs(mo.emd_hat(a, b, Cm) - np.pi / 6) < 1e-9
    assert abs(mo.emd_hat(0.25 * a, 0.25 * b, Cm) - 0.25 * np.pi / 6) < 1e-9
    # a mass surplus delta costs delta * max C
    q = p.copy()
    q[10] += 0.125
    assert abs(mo.emd_hat(p, q, Cm) - 0.125 * np.pi) < 1e-9
    # dir2 normalises each map by its own sum + 0.01
    d1, d2 = mo.emd_pair(a.reshape(7, 12), b.reshape(7, 12), Cm)
    assert abs(d1 - np.pi / 6 / 84) < 1e-9 and abs(d2 - np.pi / 6 / 1.01) < 1e-9
    assert mo.emd_pair(np.zeros((7, 12)), np.zeros((7, 12)), Cm) == (0.0, 0.0)


def test_angular_distance_matches_the_reference_mesh():
    from spatialaudiogen_amd.ambisonics import angular_distance
    Cm, _, _ = mo.angular_distance_ref(30.0)
    got = angular_distance(30.0)
    assert got.dtype == np.float64 and got.shape == (84, 84)
    assert np.abs(got - Cm).max() < 1e-13 and np.all(np.diag(got) < 1e-15)
    assert np.array_equal(got, got.T)
    # the reference's flipud (eval.py passes flipped maps with the unflipped mesh) is an isometry of this grid
    flip = np.arange(84).reshape(7, 12)[::-1].reshape(-1)
    assert np.allclose(Cm[np.ix_(flip, flip)], Cm, atol=1e-12)


# ---- driver surface ---------------------------------------------------------------------------------------------------------
def test_all_metric_keys_are_eval_py_columns():
    from spatialaudiogen_amd.evaluate import ALL_METRIC_KEYS, METRIC_KEYS
    assert ALL_METRIC_KEYS == ['amplitude/predicted', 'amplitude/gt',
                               'mse/avg', 'mse/X', 'mse/Y', 'mse/Z',
                               'stft/avg', 'stft/X', 'stft/Y', 'stft/Z',
                               'lsd/avg', 'lsd/X', 'lsd/Y', 'lsd/Z',
                               'mel_lsd/avg', 'mel_lsd/X', 'mel_lsd/Y', 'mel_lsd/Z',
                               'snr/avg', 'snr/X', 'snr/Y', 'snr/Z',
                               'env_mse/avg', 'env_mse/X', 'env_mse/Y', 'env_mse/Z',
                               'emd/dir', 'emd/dir2']
    assert METRIC_KEYS == ['amplitude/predicted', 'amplitude/gt',
                           'mse/avg', 'mse/X', 'mse/Y', 'mse/Z', 'stft/avg', 'stft/X', 'stft/Y', 'stft/Z',
                           'lsd/avg', 'lsd/X', 'lsd/Y', 'lsd/Z', 'snr/avg', 'snr/X', 'snr/Y', 'snr/Z']
    # the reference's summary (parse_eval_results.py) reads these four
    for k in ('mse/avg', 'stft/avg', 'env_mse/avg', 'emd/dir'):
        assert k in ALL_METRIC_KEYS


def test_all_metrics_flag_parses():
    from spatialaudiogen_amd.evaluate import arg_parser
    a = arg_parser().parse_args(['m', 'd', '--all_metrics', '--power_maps'])
    assert a.all_metrics and a.power_maps
    assert not arg_parser().parse_args(['m', 'd']).all_metrics


@pytest.fixture(scope='module')
def hip():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_new_entries_check_arguments_without_a_device(hip):
    buf = (C.c_float * 64)()
    dbl = (C.c_double * 64)()
    cnt = (C.c_uint32 * 1)()
    assert hip.sagen_eval_mel_env(None, buf, 16, 3, buf, buf, buf, 1 << 20, None) == -1
    assert hip.sagen_eval_mel_env(buf, buf, 16, 9, buf, buf, buf, 1 << 20, None) == -3
    assert hip.sagen_eval_mel_env(buf, buf, 0, 3, buf, buf, buf, 1 << 20, None) == -2
    need = hip.sagen_eval_mel_env_scratch_bytes(16, 3)
    assert need > 0 and hip.sagen_eval_mel_env_scratch_bytes(16, 5) > need
    assert hip.sagen_eval_mel_env(buf, buf, 16, 3, buf, buf, buf, need - 1, None) == -5
    assert b'scratch' in hip.sagen_last_error()
    assert hip.sagen_eval_emd(buf, buf, 4, 84, None, dbl, cnt, None) == -1
    assert hip.sagen_eval_emd(buf, buf, 4, 97, dbl, dbl, cnt, None) == -3
    assert hip.sagen_eval_emd(buf, buf, 0, 84, dbl, dbl, cnt, None) == -2


# ---- the exact solver core on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    try:
        path = build.build_cpu_twin()
    except Exception as e:                  # pragma: no cover - no host compiler
        pytest.fail('the CPU twin does not build: %s' % e)
    return C.CDLL(path)


def _twin_emd(L, p, q, Cm):
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    n = p.shape[0]
    out = np.zeros((n, 2))
    nc = C.c_uint32(0)
    Cm = np.ascontiguousarray(Cm, np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.sagen_eval_emd(vp(p), vp(q), C.c_int(n), C.c_int(p.shape[1]), vp(Cm), vp(out), C.byref(nc), None)
    assert rc == 0
    return out, nc.value


def map_pairs(count, seed):
    """random and degenerate [84] map pairs (RMS maps are >= 0)"""
    rng = np.random.default_rng(seed)
    P, Q = [], []
    for k in range(count):
        kind = k % 8
        p = (rng.random(84) * rng.choice([1e-3, 1.0, 30.0])).astype(np.float32)
        q = (rng.random(84) * rng.choice([1e-3, 1.0, 30.0])).astype(np.float32)
        if kind == 1:
            q = (p * (1 + 1e-3 * rng.standard_normal(84))).astype(np.float32)              # near-identical
        elif kind == 2:
            q = p.copy()                                                                     # identical
        elif kind == 3:
            q = np.zeros(84, np.float32)                                                     # one silent map: penalty only
        elif kind == 4:
            p, q = np.zeros(84, np.float32), np.zeros(84, np.float32)                        # both silent
        elif kind == 5:
            p = np.zeros(84, np.float32); p[rng.integers(84)] = 1.0                          # point masses
            q = np.zeros(84, np.float32); q[rng.integers(84)] = 1.0
        elif kind == 6:
            p = np.where(rng.random(84) < 0.2, p, 0).astype(np.float32)                      # sparse support
            q = np.where(rng.random(84) < 0.2, q, 0).astype(np.float32)
        elif kind == 7:
            p = np.full(84, 0.5, np.float32); q = np.full(84, 0.5, np.float32); q[0] = 0.6    # ties everywhere
        P.append(p); Q.append(q)
    return np.stack(P), np.stack(Q)


def test_emd_solver_core_matches_the_lp(twin):
    Cm, _, _ = mo.angular_distance_ref(30.0)
    P, Q = map_pairs(200, seed=5)
    got, nc = _twin_emd(twin, P, Q, Cm)
    assert nc == 0
    for k in range(len(P)):
        ref = mo.emd_pair(P[k], Q[k], Cm)
        for v in range(2):
            assert abs(got[k, v] - ref[v]) <= 1e-7 * abs(ref[v]) + 1e-12, (k, v, got[k, v], ref[v])


def test_emd_solver_core_non_finite_and_symmetry(twin):
    Cm, _, _ = mo.angular_distance_ref(30.0)
    P, Q = map_pairs(16, seed=6)
    P[3, 7] = np.nan
    Q[5, 0] = np.inf
    got, nc = _twin_emd(twin, P, Q, Cm)
    assert nc == 0 and np.isnan(got[3]).all() and np.isnan(got[5]).all()
    ok = [k for k in range(16) if k not in (3, 5)]
    back, _ = _twin_emd(twin, Q[ok], P[ok], Cm)          # EMD-hat is symmetric in its two maps
    assert np.allclose(back, got[ok], rtol=1e-12, atol=1e-15)
    flip = np.arange(84).reshape(7, 12)[::-1].reshape(-1)
    fl, _ = _twin_emd(twin, P[ok][:, flip], Q[ok][:, flip], Cm)
    assert np.allclose(fl, got[ok], rtol=1e-9, atol=1e-15)
    assert math.isfinite(float(got[ok].sum()))
