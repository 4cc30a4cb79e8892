"""eval_oracle.py proven on the host (no GPU), before a kernel is involved: its references against known answers and against the
older oracles where they overlap, its case lists against what they claim, and its bounds against restatements with one thing wrong -
a Hermitian weight of 2 on bins 0 / 600, a reflect pad that repeats the edge sample, a Hilbert ring read one sample late, and the
power map's ten moments summed in float32 (the order power_moments_kernel had: per lane, a wave tree, fp64 across the waves) - each
outside the bound on the inputs named for it, while the float32 restatement of the LSD's DFT and the fp64-moment power map are inside."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_oracle as E  # noqa: E402
import metric_oracle as mo  # noqa: E402
from oracle import np_oracle as O  # noqa: E402
from test_eval_metrics_host import twin, _twin_emd  # noqa: E402,F401  (the CPU twin as a ctypes library)

U = E.U


# ---- per-sample metrics --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def batch16():
    pred, gt, names = E.metric_batch(16, 3, E.METRIC_STARTS[16])
    return pred, gt, names


def test_metric_references_agree_with_the_older_oracle(batch16):
    pred, gt, _ = batch16
    m, stft, lsd, mse, snr = O.evaluation_ops(pred, gt)
    tm = E.time_metrics_ref(pred, gt)
    assert np.allclose(tm['stft'], stft, rtol=1e-12, atol=1e-18) and np.allclose(tm['mse'], mse, rtol=1e-13, atol=0)
    assert np.allclose(tm['snr'], snr, rtol=0, atol=1e-12)
    assert np.allclose(E.lsd_ref(pred, gt), lsd, rtol=0, atol=1e-11)                    # the Hermitian weights = the mean over 1200 bins
    assert abs(tm['pw'][0] / 48 - m['pow/pred']) <= 1e-12 * m['pow/pred'] and abs(tm['pw'][1] / 48 - m['pow/gt']) <= 1e-12 * m['pow/gt']
    # any channel count: a five-channel batch is its channels one by one
    p5, g5, _ = E.metric_batch(2, 5, 11)
    t5, l5 = E.time_metrics_ref(p5, g5), E.lsd_ref(p5, g5)
    for c in range(5):
        one = E.time_metrics_ref(p5[:, :, c:c + 1], g5[:, :, c:c + 1])
        assert np.allclose(one['stft'][:, 0], t5['stft'][:, c], rtol=1e-13, atol=0) and np.allclose(one['snr'][:, 0], t5['snr'][:, c], rtol=0, atol=1e-12)
        assert np.allclose(E.lsd_ref(p5[:, :, c:c + 1], g5[:, :, c:c + 1])[:, 0], l5[:, c], rtol=1e-12, atol=1e-13)


def test_impulse_pins_the_three_loss_windows():
    """An impulse of height a at n in the difference: stft distance = a^2 / 3 * sum over the windows that hold n of hann[n - start]^2
    (Parseval), 0 from 4096 on, with an MSE of a^2 / 4800 everywhere."""
    a = 0.25
    for n in E.IMPULSES:
        gt = np.zeros((1, 4800, 1), np.float32)
        pred = gt.copy()
        pred[0, n, 0] = a
        tm = E.time_metrics_ref(pred, gt)
        want = sum(E.HANN_SL[n - lo] ** 2 for lo, hi in E.SL_WINDOWS if lo <= n < hi) * a * a / 3
        assert abs(tm['stft'][0, 0] - want) <= 1e-15, n
        assert (want == 0) == (n >= 4096 or n == 0), n            # hann[0] = 0; 2048 starts one window and is the centre of [1024, 3072)
        assert abs(tm['mse'][0, 0] - a * a / 4800) <= 1e-18
    names = [s[0] for s in E.metric_slots()]
    assert all('imp_%s_%d' % (k, n) in names for n in E.IMPULSES for k in ('pred', 'gt', 'diff'))


def test_dc_and_nyquist_frames_in_closed_form_and_the_wrong_weight_is_seen(batch16):
    """A constant c under the periodic Hann: |X[0]| = 600 c, |X[1]| = |X[1199]| = 300 c, nothing else; (-1)^n c: the same around bin
    600.  The frame's LSD is sqrt((d0^2 + 2 d1^2) / 1200) - and sqrt((2 d0^2 + 2 d1^2) / 1200) with the Hermitian weight wrong, which
    the bound must see."""
    pred, gt, names = batch16
    ref, bound = E.lsd_ref(pred, gt, with_bound=True)
    wrong = E.lsd_ref(pred, gt, weights=np.full(601, 2.0))
    P = lambda m: E.K10 * np.log(m + 0.01)
    d0, d1 = P(600 * 0.004) - P(600 * 0.002), P(300 * 0.004) - P(300 * 0.002)
    want = np.sqrt((d0 ** 2 + 2 * d1 ** 2) / 1200)
    for name in ('dc_only', 'dc_only_swapped', 'nyquist_only'):
        b, c = divmod(names.index(name), 3)
        assert abs(ref[b, c] - want) <= 1e-9, name
        assert abs(wrong[b, c] - ref[b, c]) > 3 * bound[b, c], (name, wrong[b, c] - ref[b, c], bound[b, c])
    # ... and nowhere does the wrong weight hide in a case whose bins 0 / 600 differ by more than a bound's worth
    assert np.isfinite(ref).all() and np.isfinite(bound).all() and np.all(bound <= 2e-3 * np.maximum(1.0, ref))
    # the frame list: samples 4200.. are in no frame, 3600..4199 in frame 5 only
    for name, frames in (('beyond_lsd_frames', []), ('lsd_frame5_only', [5])):
        b, c = divmod(names.index(name), 3)
        live = np.nonzero(np.abs(E.lsd_frames(gt)[b, c]).sum(-1))[0].tolist()
        assert live == frames, (name, live)


def test_float32_restatement_of_the_dft_is_inside_the_bound(batch16):
    """The contraction as igemm_kernel does it, with every rounding made explicit: frames and matrix in float32, each product rounded,
    1200 sequential float32 additions.  Its magnitudes stay inside dm = LSD_DFT_C u A1 + 3 u m on every frame of the list."""
    pred, gt, _ = batch16
    f64 = np.concatenate([E.lsd_frames(gt), E.lsd_frames(pred)]).reshape(-1, 1200)
    f32 = (np.concatenate([gt, pred]).transpose(0, 2, 1)[:, :, None, :].astype(np.float32))
    f32 = np.stack([f32[:, :, 0, 600 * t:600 * t + 1200] for t in range(6)], 2).reshape(-1, 1200) * E.HANN_LSD.astype(np.float32)
    assert f32.dtype == np.float32
    k, n = np.arange(601)[None, :], np.arange(1200)[:, None]
    ang = 2 * np.pi * ((k * n) % 1200) / 1200
    W = np.concatenate([np.cos(ang), -np.sin(ang)], 1).astype(np.float32)
    acc = np.zeros((len(f32), 1202), np.float32)
    for j in range(1200):
        acc += f32[:, j, None] * W[None, j, :]
    m32 = np.sqrt(acc[:, :601].astype(np.float64) ** 2 + acc[:, 601:].astype(np.float64) ** 2)
    m64 = np.abs(np.fft.rfft(f64, axis=-1))
    A1 = np.abs(f64).sum(-1, keepdims=True)
    frac = np.abs(m32 - m64) / np.maximum(E.LSD_DFT_C * U * A1 + 3 * U * m64, 1e-300)
    assert frac.max() < 1.0, frac.max()
    print('LSD DFT float32 restatement: worst %.3f of dm' % frac.max())


def test_snr_and_sum_bounds_are_tighter_than_the_older_ones(batch16):
    pred, gt, _ = batch16
    tm = E.time_metrics_ref(pred, gt)
    assert E.SUM_C * U < 1e-5 and np.all(E.snr_bound(tm['snr']) < 1e-4) and E.SNR_DB < 3e-5
    assert np.isfinite(tm['stft']).all() and np.isfinite(tm['snr']).all() and np.isfinite(tm['pw']).all()


# ---- mel-LSD and envelope --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mel_table():
    """name -> (pred, gt, impulse, mel ref, mel bound, env ref, env bound)"""
    return {name: (p, g, imp) + E.mel_lsd_ref(p, g, with_bound=True) + E.env_ref(p, g, imp) for name, p, g, imp in E.mel_slots()}


def test_mel_and_envelope_references_agree_with_metric_oracle(mel_table):
    for name, (p, g, imp, mel, mb, env, eb) in mel_table.items():
        assert abs(mel - mo.mel_lsd(p[:, None].astype(np.float64), g[:, None].astype(np.float64))[0]) <= 1e-10, name
        assert abs(env - mo.env_mse(p[:, None], g[:, None])[0]) <= 1e-15, name
        assert np.isfinite([mel, mb, env, eb]).all() and mb <= 1e-4 * max(1.0, mel) and eb <= 1e-4 * env + 1e-6 + 1e-12, name
    # the circulant form the kernel walks is scipy's analytic signal
    x = mel_table['ramp'][0]
    assert np.allclose(np.sqrt(x.astype(np.float64) ** 2 + E.hilbert_circulant(x) ** 2), mo.envelope(x), atol=1e-12)


def test_known_answers_of_the_mel_and_envelope_cases(mel_table):
    p, g, _, mel, _, env, _ = mel_table['periodic_tone']                 # whole periods: the envelope is the amplitude
    assert np.allclose(E.envelope_ref(p), 0.7, atol=1e-6) and abs(env - 0.35) < 1e-6
    assert mel_table['nyquist'][3] == 0.0                                  # bin 1024 lies above every band: both sides sit on the floor
    # 13 kHz reaches no band either (the last triangle ends at 12 kHz = bin 512) - up to the Hann window's skirt, which the 1e-2 floor hides
    p, g = mel_table['tone_13000'][:2]
    Sp = np.abs(np.fft.rfft(E.mel_frames(p)[4])[:513]) ** 2
    assert (Sp @ E.MEL_W.T).max() < 1e-2 * 1e-3 and E.MEL_W[127, 511] > 0 and E.MEL_W[127, 512] == 0
    assert (np.abs(np.fft.rfft(E.mel_frames(mel_table['tone_11900'][0])[4])[:513]) ** 2 @ E.MEL_W.T)[127] > 1.0
    # an impulse against silence: the Hilbert transform is unitary off DC and Nyquist, env_mse = a sqrt((2 - 2 / N) / N) wherever it sits
    for m in E.MEL_IMPULSES:
        assert abs(mel_table['imp_%d_vs_silence' % m][5] - 0.3 * np.sqrt((2 - 2 / 4800) / 4800)) < 1e-8
    assert mel_table['silent_both'][3] == 0 and mel_table['silent_both'][5] == 0 and mel_table['identical'][3] == 0


def test_an_edge_repeating_pad_is_outside_the_mel_bound(mel_table):
    for m in (0, 1, 2, 4797, 4798, 4799):
        for name in ('imp_%d' % m, 'imp_%d_vs_silence' % m):
            p, g, _, mel, mb = mel_table[name][:5]
            mutant = E.mel_lsd_ref(p, g, pad_mode='symmetric')
            assert abs(mutant - mel) > 100 * mb, (name, mutant - mel, mb)
    for m in (2400, 2401):                                                  # inside, the pad is never reached
        p, g = mel_table['imp_%d' % m][:2]
        assert E.mel_lsd_ref(p, g, pad_mode='symmetric') == mel_table['imp_%d' % m][3]


def test_a_ring_read_one_sample_late_is_outside_the_impulse_bound(mel_table):
    for m in E.MEL_IMPULSES:
        p, g, imp, _, _, env, eb = mel_table['imp_%d' % m]
        assert imp and eb < 1e-5 * env
        mutant = E.env_ref(p, g, True, ring_shift=1)[0]
        assert abs(mutant - env) > 1000 * eb, (m, mutant - env, eb)


def test_mel_shapes_cover_the_channel_counts_and_the_second_finish_block():
    assert sorted(c for _, c, _ in E.MEL_SHAPES) == [1, 2, 3, 4, 5, 8] and any(b * c > 64 for b, c, _ in E.MEL_SHAPES)
    assert any(b == 1 for b, _, _ in E.MEL_SHAPES)
    seen = set()
    for b, c, s in E.MEL_SHAPES:
        meta = E.mel_batch(b, c, s)[2]
        seen |= {name for name, _ in meta}
        if c > 1:
            assert len({name for name, _ in meta[:c]}) == c                # neighbouring channels carry different families
    assert seen == {s[0] for s in E.mel_slots()}


# ---- EMD -------------------------------------------------------------------------------------------------------------------------
def test_emd_metrics_are_metrics():
    for n in E.EMD_NODES:
        C = E.emd_metric(n)
        assert C.shape == (n, n) and np.array_equal(C, C.T) and np.all(np.diag(C) == 0) and np.all(C >= 0)
        assert np.all(C[:, None, :] <= C[:, :, None] + C[None, :, :] + 1e-12)          # the min(P, Q) shortcut needs the triangle inequality
        if n >= 3 and n != 84:
            assert C[0, 1] == 0 and np.array_equal(C[0], C[1])                          # duplicate vectors: ties in every row
    from spatialaudiogen_amd.ambisonics import angular_distance
    assert np.array_equal(E.emd_metric(84), angular_distance(30.0)) and (E.emd_metric(84)[:12, :12] < 1e-12).all()   # the pole nodes coincide


def test_emd_case_lists_hold_what_they_claim():
    """More than one pass of WIDTH = 64 over the sources WITH sinks to reach, and the reverse; the rerouting branch; ties."""
    for n in E.EMD_NODES:
        C = E.emd_metric(n)
        cases = {name: (p, q) for name, p, q in E.emd_cases(n)}
        assert len(cases) == len(E.emd_cases(n)) and all(np.isfinite(p).all() and np.isfinite(q).all() and (p >= 0).all() and (q >= 0).all()
                                                         for p, q in cases.values())
        split = lambda name, v: tuple(len(x) for x in E.emd_split(*E.emd_masses(*cases[name], v)))
        if n >= 66:
            for nd in sorted({1, 4, n - 65}):
                assert split('src65_snk%d' % nd, 0) == (65, nd) and split('src65_snk%d_swapped' % nd, 0) == (nd, 65)
            for v in (0, 1):
                assert split('diffuse_vs_plane', v) == (n - 3, 3) and split('diffuse_vs_plane_swapped', v) == (3, n - 3)
        if n >= 4:
            for name in ('reroute', 'reroute_swapped'):
                for v in (0, 1):
                    assert E.emd_serial(*E.emd_masses(*cases[name], v), C)[2]['reroutes'] > 0, (n, name, v)
        if n >= 3:
            p, q = cases['ties']
            assert p[0] == p[1] and q[0] == q[1] and len(np.unique(p)) < n // 2 + 2
    assert {n for n in E.EMD_NODES if n >= 66} == {84, 96}


def test_emd_serial_restatement_equals_the_twin_and_the_lp(twin):
    for n in E.EMD_NODES:
        C = E.emd_metric(n)
        cases = E.emd_cases(n)
        P, Q = np.stack([p for _, p, _ in cases]), np.stack([q for _, _, q in cases])
        got, nc = _twin_emd(twin, P, Q, C)
        lp = E.emd_lp_refs(n)
        assert nc == 0 and np.isfinite(lp).all()
        for k, (name, p, q) in enumerate(cases):
            for v in range(2):
                val, ok, _ = E.emd_serial(*E.emd_masses(p, q, v), C)
                assert ok and abs(val - got[k, v]) <= 1e-12 * abs(got[k, v]), (n, name, v, val, got[k, v])
                assert abs(got[k, v] - lp[k, v]) <= 1e-7 * abs(lp[k, v]) + 1e-12, (n, name, v, got[k, v], lp[k, v])
    # point masses: mass x distance, in both normalisations
    C = E.emd_metric(96)
    p, q = dict((name, (p, q)) for name, p, q in E.emd_cases(96))['point_masses']
    assert abs(E.emd_serial(*E.emd_masses(p, q, 0), C)[0] - 2.0 / 96 * C[0, 95]) < 1e-15
    assert abs(E.emd_serial(*E.emd_masses(p, q, 1), C)[0] - 2.0 / 2.01 * C[0, 95]) < 1e-15


def test_blocked_costs_raise_the_counter_on_the_twin(twin):
    p, q, C, exp, count = E.emd_blocked_case()
    assert count == 4 and np.isfinite(exp).all() and np.all(exp[[0, 4]] == 0)
    got, nc = _twin_emd(twin, p, q, C)
    assert nc == count and np.allclose(got, exp, rtol=1e-12, atol=0)


# ---- power maps ------------------------------------------------------------------------------------------------------------------
def test_power_map_reference_against_the_older_oracle_and_a_plane_wave_in_closed_form():
    r = np.random.default_rng(3)
    a = (r.standard_normal((4800, 4)) * np.array([1.0, 0.3, 0.1, 0.6])).astype(np.float32)
    sh = E.pm_mesh('30')
    ref = E.power_map_ref(a, sh)
    old = np.flipud(O.power_map(a, 30.0)).reshape(-1)                      # O.power_map's fp64 matrix against the float32 one of the call
    assert np.abs(ref - old).max() <= 2e-7 * old.max()
    assert np.abs(E.power_map_ref(a, sh, block=1000) - ref).max() <= 1e-14
    # a plane wave s(t) Y(u) decoded at v: s (1 + u . v), so rms = rms(s) (1 + cos gamma): twice rms(s) at the source, 0 at the antipode
    sh64 = sh.astype(np.float64)
    for node in E.pm_nodes('30', sh):
        s = r.standard_normal(4800)
        got = E.power_map_ref(s[:, None] * sh64[node], sh64)
        cosg = sh64[:, 1:] @ sh64[node, 1:]
        assert np.abs(got - np.sqrt(np.mean(s ** 2)) * (1 + cosg)).max() <= 1e-6 * got.max()
        q, exact = E.pm_antipode(sh, node)
        assert abs(cosg[q] + 1) < 1e-6 and got[q] < 1e-6 * got.max()
    sh, names, ambi = E.pm_chunks('r83', 4800, 13)
    assert E.pm_antipode(sh, 0) == (1, True) and names[1] == 'silent' and names[5] == 'silent' and not ambi[1].any()
    assert set(names) == {x[0] for x in E.pm_signals(sh, (0, 1, 2), 8, 0)}
    k = names.index('plane_pow2')
    assert np.array_equal(ambi[k][:, 0], ambi[k][:, 2]) and not ambi[k][:, 1].any()     # exact in float32: the node (1, 0, -1, 0) is an exact null


def test_power_map_cases_cover_the_issue():
    cases = E.pm_cases()
    assert {m for m, _, _ in cases} == {'30', '5'} | {'r%d' % p for p in E.PM_RANDOM_P}
    assert {T for _, T, _ in cases} == set(E.PM_T) and {n for _, _, n in cases} == {1, 2, 13}
    assert max(E.PM_T) > 1024 * 256                                         # the grid-stride loop of power_moments_kernel takes a second trip
    assert {len(E.pm_mesh('r%d' % p)) % 2 for p in E.PM_RANDOM_P} == {0, 1}  # the moments' offset rms + ((P + 1) / 2) * 2 both ways


def test_float32_moments_leave_a_floor_at_the_null_and_fp64_moments_do_not():
    """The reason power_moments_kernel and power_moments_batched_kernel sum in fp64.  A plane wave toward node 40 of the 30 degree mesh
    (seed 0) and node 1337 of the 5 degree mesh (seed 1), T = 4800, the float32 matrix: the quadratic form cancels at the antipode, and
    the float32 sums leave up to 1e-4 of the map's maximum there."""
    worst64 = 0.0
    for mesh, node, seed, least in (('30', 40, 0, 100.0), ('5', 1337, 1, 2.0), ('30', 19, 2, 100.0)):
        sh = E.pm_mesh(mesh)
        s = np.random.default_rng(seed).standard_normal(4800)
        a = (s[:, None] * sh[node].astype(np.float64)).astype(np.float32)
        ref = E.power_map_ref(a, sh)
        bound = E.power_map_bound(ref)
        e32 = np.abs(E.power_map_moments(a, sh, 'f32') - ref) / bound
        e64 = np.abs(E.power_map_moments(a, sh, 'f64') - ref) / bound
        q, _ = E.pm_antipode(sh, node)
        print('power map %s node %d: float32 moments %.1f bounds (%.2e of max) at node %d (antipode %d), fp64 moments %.4f'
              % (mesh, node, e32.max(), e32.max() * bound[np.argmax(e32)] / ref.max(), int(np.argmax(e32)), q, e64.max()))
        assert e32.max() > least and e64.max() < 0.2
        worst64 = max(worst64, e64.max())
    # every family of the case list: fp64 moments 5x inside
    for mesh in ('30', 'r83', 'r2'):
        sh, names, ambi = E.pm_chunks(mesh, 4800, 13)
        for name, a in zip(names, ambi):
            ref = E.power_map_ref(a, sh)
            assert np.isfinite(ref).all()
            err = np.abs(E.power_map_moments(a, sh, 'f64') - ref)
            assert np.all(err <= 0.2 * E.power_map_bound(ref)), (mesh, name)
