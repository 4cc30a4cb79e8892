"""fp64 references, derived bounds and case lists for the kernels that produce the numbers `evaluate --all_metrics` reports:
csrc/eval.hip (sagen_eval_metrics / sagen_eval_metrics_c: stft distance, LSD, temporal MSE, SNR, power sums), csrc/evalx.hip
(sagen_eval_mel_env: mel-LSD, envelope distance; sagen_eval_emd: EMD-hat) and the two power-map kernel pairs of csrc/elementwise.hip
(sagen_power_map, sagen_power_map_batched).  The companion of spectral_oracle.py: plain numpy in float64, no kernel, no library;
what oracle.np_oracle and metric_oracle.py already state is reused, not restated.  test_eval_oracle_host.py proves the references,
the case lists and the bounds (each against a restatement with one thing wrong) before a kernel is involved;
test_gpu_eval_ops.py holds the kernels - and, through test_cpu_twin_ops.py, the CPU twin's power maps and EMD - to them.

References take the float32 inputs the kernel gets, widened to float64.  u = 2^-24.  Every bound is a formula of the reference and of
float32 / float64 rounding; none is tuned to what a kernel gives, and none is looser than the bound the older test of the same
quantity uses (where both exist the smaller one holds: min(derived, old)).

Sums (stft distance, MSE, the two power sums; eval_time_kernel).  Non-negative sums of 4800 terms: 19 serial additions per lane, a
6-level wave tree, 3 additions across the four waves = 28 roundings, each relative to a partial sum that is at most the total.  A
term carries: d = g - p (1, twice in d^2), the square (1) = 3 for the MSE and the powers; for the stft distance also the Hann value
rounded to float32 (1, twice in h^2), h h (1), the sum of the two overlapping windows (1) and the two products with d (2) = 8.
The closing division: 1.  8 + 28 + 1 = 37 -> SUM_C = 40:  |got - ref| <= 40 u ref = 2.4e-6 ref (the older test: 1e-5 of the RMS).
A window whose difference is zero gives exactly 0, and an impulse at 4096..4799 gives a stft distance of exactly 0: no
stft_for_loss window ([0,2048), [2048,4096), [1024,3072)) covers it.

SNR = 10 log10((G + 0.1) / (D + 0.1)), G and D two such sums: (10 / ln 10) (2 x 40 u + 2 u for the two additions of 0.1 + 1 u for
the quotient) = 4.343 x 83 u = 2.2e-5 dB, plus logf (2 ulp), the product with 10 and the division by logf(10) (one rounding each, logf(10)
itself 2 ulp): 8 u |snr|.  At 60 dB that is 2.9e-5: together under 6e-5 dB, against the 1e-3 of the older test.

LSD (eval_lsd_frames_kernel, the [1200 x 1202] DFT on igemm_kernel - exact fp32 products, fp32 accumulation - and
eval_lsd_reduce_kernel).  Per frame f = x hann (float32) and bin k, with A1 = sum_n |f[n]| (<= sqrt(1200) ||f||_2):
    dm[k] = LSD_DFT_C u A1 + 3 u m[k]                                       (m = |X[k]| of the fp64 transform)
    1       the window product, one rounding per sample, |w| <= 1
    1       the DFT matrix entry rounded to float32, |dw| <= u
    2 sqrt(1200) = 70   the 1200 sequential fp32 additions of the contraction: each rounds a partial sum of magnitude <= A1, so the
            worst case is 1200; independent roundings add in quadrature, sqrt(1200) = 35, taken twice.  This one count is a model,
            not a worst case: the host test holds a float32 restatement (float32 matrix, sequential float32 sums) inside it on every
            case of the list, and DESIGN.md records what the device measures.
    3 u m   two squares, their sum and sqrtf
LSD_DFT_C = 72.  In dB, P = 10 log10(m + 0.01):  dP <= (10 / ln 10) dm / (max(m - dm, 0) + 0.01) + (10 / ln 10) 4 u (|ln(m + 0.01)| + 1)
(logf 2 ulp, the addition of the floor, the two closing roundings), for gt and for pred.  A frame's value is a 2-norm over the bins,
||a| - |b|| <= |a - b|:  d frame <= sqrt(sum_k w_k (dP_gt + dP_pred)^2 / 1200) with the Hermitian weights w = 1, 2, .., 2, 1, and
the mean over the six frames and the closing roundings (a 601-term fp32 sum: 3 + 6 + 3 additions, sqrtf, the division): + 16 u ref.
The floor 0.01 decides how tight this is: the DC-only and Nyquist-only cases use amplitudes 0.002 / 0.004, where A1 <= 2.4,
dm <= 1.1e-5 and an empty bin moves by at most 0.007 dB (a derived bound of 6.7e-3 on the frame), while bins 0 / 600 sit 3 dB apart
at weight 1: a weight of 2 there moves the frame by 0.023 dB, three derived bounds out.  The older bound, 2e-3 max(1, ref), caps the
derived one wherever it is smaller - on these frames it is, so the wrong weight is eleven bounds out (test_eval_oracle_host.py).

mel-LSD (evalx_mel_kernel).  pred and gt of a frame are the real and imaginary part of ONE complex radix-2 transform, so every
rounding is relative to both: A = sum_n (|p[n]| + |g[n]|) hann[n] over the reflect-padded frame.  Per bin, in units of u A:
1 (window product) + 11 x 7 (per stage: the float32 twiddle 1, the complex product 3, on magnitudes x sqrt 2 <= 6, one addition 1)
+ 1 (the Hermitian split) = MEL_C = 79, as spectral_oracle.py counts its radix-4 stages.  dm = 79 u A; the power S = m^2 moves by
dS = 2 m dm + dm^2 + 4 u S; the band energy M = W S is summed in fp64: dM = W dS; dL = (10 / ln 10) dM / (max(M - dM, 0) + 0.01);
d mel_lsd <= sqrt(mean over 128 x 10 of (dL_gt + dL_pred)^2) + 8 u ref.  The older bound 1e-4 max(1, ref) caps it.

Envelope (evalx_env_kernel).  The older form 1e-4 ref + 1e-6 sig (sig = RMS of both signals) stays for dense signals: the 2400-tap
fp32 sum has no tighter derived bound here.  An impulse is different: every Hilbert sum has ONE non-zero term, so an output element is
a tap rounded to float32 (1) times the sample (1), squared and added (2) under sqrtf (1): 5 u e.  With e_g, e_p the two envelopes
    |got - ref| <= 5 u sqrt(mean (e_g + e_p)^2) + 40 u ref          (the 4800-term sum of squares as above)
which is 1e-6 of the impulse's amplitude: a ring index off by one (the wrapped half of the ring read one sample late) moves the
value by 1e-2 of it.

EMD.  fp64 throughout and deterministic: 1e-7 |ref| + 1e-12 against the LP (the LP solver's own tolerances: 1e-10 on O(1) masses),
and 1e-12 relative against the serial core (EmdSerial, the CPU twin): the lane-parallel walk differs from it only in the order of
the closing cost sum, n <= 48 terms of fp64.

Power maps (power_moments[_batched]_kernel + power_map[_batched]_kernel).  |got - ref| <= 2^-23 ref[p] + 2^-22 max(ref), elementwise,
nulls included.  2^-23 ref: the float32 result (2^-24) and one more for sqrt and the scaling.  2^-22 max(ref) is the floor of the
quadratic form: e = sh S sh^T cancels where a plane wave has its null, to the rounding of the ten moments.  With fp64 moments of
float32 inputs (products exact; 19 serial additions per lane, then 8 tree levels: about five roundings in quadrature, 5e-16 |S|) the
sixteen terms of the form leave e off by about 1e-14 |S|, and the square root makes 1e-7 sqrt(|S| / T) of it: at most 5e-8 max(ref)
in the restatement of test_eval_oracle_host.py, 5x inside.  With float32 moments the same count starts from 2^-24 and the square root
makes 1e-4 max(ref) of it (restated there too, same inputs: 6e-5 .. 1e-4).  The reference evaluates the definition,
sqrt(mean_t (ambi . sh[p])^2), which has no cancellation.
"""
import numpy as np

import metric_oracle as mo

U = 2.0 ** -24
K10 = 10.0 / np.log(10.0)
EV_N, EPS = 4800, 1e-2
SL_W = 2048
SL_WINDOWS = ((0, 2048), (2048, 4096), (1024, 3072))                    # myutils.stft_for_loss at window 1200 -> 2048, overlap 2
LSD_W, LSD_HOP, LSD_T = 1200, 600, 6
HANN_SL = (0.5 - 0.5 * np.cos(2 * np.pi / SL_W * np.arange(SL_W))).astype(np.float32).astype(np.float64)
HANN_LSD = (0.5 - 0.5 * np.cos(2 * np.pi / LSD_W * np.arange(LSD_W))).astype(np.float32).astype(np.float64)
HERMITIAN = np.concatenate([[1.0], np.full(599, 2.0), [1.0]])
SUM_C, LSD_DFT_C, MEL_C = 40, 72, 79
SNR_DB = K10 * (2 * SUM_C + 3) * U


# ------------------------------------------------------------------------------------------------------------------------
# sagen_eval_metrics[_c]
# ------------------------------------------------------------------------------------------------------------------------
def time_metrics_ref(pred, gt):
    """pred / gt [B, 4800, C] -> dict(stft, mse, snr [B, C]; pw [2] = sum pred^2, sum gt^2).  The stft distance in its FFT form
    (model.py:62-76): the kernel's Parseval form is what is under test."""
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    d = g - p
    stft = np.zeros(p.shape[::2])
    for lo, hi in SL_WINDOWS:
        X = np.fft.fft(d[:, lo:hi, :] * HANN_SL[None, :, None], axis=1)
        stft += (np.abs(X) ** 2).mean(1)
    D, G = (d ** 2).sum(1), (g ** 2).sum(1)
    return dict(stft=stft / 3.0, mse=D / EV_N, snr=K10 * np.log((G + 0.1) / (D + 0.1)), pw=np.array([(p ** 2).sum(), G.sum()]))


def snr_bound(snr_ref):
    return SNR_DB + 8 * U * np.abs(snr_ref)


def lsd_frames(x):
    """[B, 4800, C] -> [B, C, 6, 1200]: frame t = samples [600 t, 600 t + 1200) times the float32-rounded periodic Hann (myutils.stft
    with wind_size 1200, n_overlap 2: samples 4200..4799 belong to no frame)."""
    x = np.asarray(x, np.float64).transpose(0, 2, 1)
    return np.stack([x[:, :, LSD_HOP * t:LSD_HOP * t + LSD_W] for t in range(LSD_T)], 2) * HANN_LSD


def lsd_ref(pred, gt, weights=HERMITIAN, with_bound=False):
    """model.py:78-94 -> [B, C]: mean over the frames of sqrt(mean over the 1200 bins of (P_gt - P_pred)^2), P = 10 log10(|X| + 0.01),
    on the 601 bins of the real transform with their Hermitian multiplicities (`weights`: what a mutant gets wrong)."""
    fg, fp = lsd_frames(gt), lsd_frames(pred)
    mg, mp = np.abs(np.fft.rfft(fg, axis=-1)), np.abs(np.fft.rfft(fp, axis=-1))
    d = K10 * (np.log(mg + EPS) - np.log(mp + EPS))
    ref = np.sqrt((weights * d ** 2).sum(-1) / LSD_W).mean(-1)
    if not with_bound:
        return ref

    def dP(f, m):
        dm = LSD_DFT_C * U * np.abs(f).sum(-1, keepdims=True) + 3 * U * m
        return K10 * (dm / (np.maximum(m - dm, 0) + EPS) + 4 * U * (np.abs(np.log(m + EPS)) + 1))
    e = dP(fg, mg) + dP(fp, mp)
    derived = np.sqrt((HERMITIAN * e ** 2).sum(-1) / LSD_W).mean(-1) + 16 * U * ref
    return ref, np.minimum(derived, 2e-3 * np.maximum(1.0, ref))


# ------------------------------------------------------------------------------------------------------------------------
# sagen_eval_mel_env
# ------------------------------------------------------------------------------------------------------------------------
MEL_W = mo.mel_basis()[:, :513]
HANN_MEL = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(mo.N_FFT) / mo.N_FFT)


def mel_frames(x, pad_mode='reflect'):
    """[4800] -> [10, 2048] windowed frames of the centred transform (librosa 0.6.0: np.pad reflect; 'symmetric' is the mutant that
    repeats the edge sample)."""
    xp = np.pad(np.asarray(x, np.float64), mo.N_FFT // 2, mode=pad_mode)
    return np.stack([xp[t * mo.HOP:t * mo.HOP + mo.N_FFT] for t in range(10)]) * HANN_MEL


def mel_lsd_ref(pred, gt, pad_mode='reflect', with_bound=False):
    """pred / gt [4800] of one channel -> mel_lsd (and its bound)."""
    fp, fg = mel_frames(pred, pad_mode), mel_frames(gt, pad_mode)
    Sp, Sg = np.abs(np.fft.rfft(fp, axis=-1)[:, :513]) ** 2, np.abs(np.fft.rfft(fg, axis=-1)[:, :513]) ** 2
    Mp, Mg = Sp @ MEL_W.T, Sg @ MEL_W.T                                   # [10, 128]
    ref = np.sqrt(np.mean((10 * np.log10(Mg + EPS) - 10 * np.log10(Mp + EPS)) ** 2))
    if not with_bound:
        return ref
    dm = MEL_C * U * (np.abs(fp) + np.abs(fg)).sum(-1, keepdims=True)

    def dL(S, M):
        dS = 2 * np.sqrt(S) * dm + dm ** 2 + 4 * U * S
        dM = dS @ MEL_W.T
        return K10 * dM / (np.maximum(M - dM, 0) + EPS)
    derived = np.sqrt(np.mean((dL(Sp, Mp) + dL(Sg, Mg)) ** 2)) + 8 * U * ref
    return ref, min(derived, 1e-4 * max(1.0, ref))


def hilbert_circulant(x, ring_shift=0):
    """(Hx)[n] = sum over the odd k of g[k] x[(n - k) mod N], as evalx_env_kernel walks it.  ring_shift = 1 is the mutant: indices
    below zero (the wrapped half of the ring) read one sample late."""
    x = np.asarray(x, np.float64)
    N = len(x)
    g = mo.hilbert_kernel(N)
    n = np.arange(N)[:, None]
    k = np.arange(1, N, 2)[None, :]
    i = n - k
    src = np.where(i < 0, (i + ring_shift) % N, i)
    return (g[k] * x[src]).sum(1)


def envelope_ref(x, ring_shift=0):
    x = np.asarray(x, np.float64)
    if ring_shift == 0:
        return mo.envelope(x)
    return np.sqrt(x ** 2 + hilbert_circulant(x, ring_shift) ** 2)


def env_ref(pred, gt, impulse=False, ring_shift=0):
    """pred / gt [4800] -> (env_mse, bound)."""
    ep, eg = envelope_ref(pred, ring_shift), envelope_ref(gt, ring_shift)
    ref = np.sqrt(np.mean((eg - ep) ** 2))
    sig = np.sqrt(np.mean(np.asarray(gt, np.float64) ** 2 + np.asarray(pred, np.float64) ** 2))
    bound = 1e-4 * ref + 1e-6 * sig + 1e-12
    if impulse:
        bound = min(bound, 5 * U * np.sqrt(np.mean((eg + ep) ** 2)) + 40 * U * ref)
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------------
# signal families
# ------------------------------------------------------------------------------------------------------------------------
IMPULSES = (0, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, 4799)
MEL_IMPULSES = (0, 1, 2, 4797, 4798, 4799, 2400, 2401)


def _imp(n, a=1.0):
    x = np.zeros(EV_N)
    x[n] = a
    return x


def metric_slots():
    """The (name, pred [4800], gt [4800]) families of the per-sample metrics, float32.  A batch [B, 4800, C] is filled slot by slot."""
    r = np.random.default_rng(20241021)
    n = np.arange(EV_N)
    noise = lambda a: a * r.standard_normal(EV_N)
    z = np.zeros(EV_N)
    s = [('silent_both', z, z), ('silent_pred', z, noise(0.3)), ('silent_gt', noise(0.3), z)]
    x = noise(0.2)
    s += [('identical', x, x), ('amp_1e-4', noise(1e-4), noise(1e-4)), ('amp_1', noise(1.0), noise(1.0)),
          ('dc_offset', noise(0.1) + 0.5, noise(0.1)), ('dc_offset_both', noise(0.1) + 0.5, noise(0.1) + 0.25)]
    for m in IMPULSES:
        base = noise(0.05)
        s += [('imp_pred_%d' % m, _imp(m), z), ('imp_gt_%d' % m, z, _imp(m, 0.5)), ('imp_diff_%d' % m, base + _imp(m, 0.25), base)]
    alt = np.where(n % 2 == 0, 1.0, -1.0)
    s += [('dc_only', np.full(EV_N, 0.002), np.full(EV_N, 0.004)), ('dc_only_swapped', np.full(EV_N, 0.004), np.full(EV_N, 0.002)),
          ('nyquist_only', 0.002 * alt, 0.004 * alt), ('nyquist_vs_dc', 0.004 * alt, np.full(EV_N, 0.002)),
          ('tone_on_bin', 0.2 * np.sin(2 * np.pi * 37 * n / LSD_W + 0.3), 0.3 * np.sin(2 * np.pi * 37 * n / LSD_W)),
          ('tone_between_bins', 0.2 * np.sin(2 * np.pi * 37.5 * n / LSD_W), 0.3 * np.sin(2 * np.pi * 37.5 * n / LSD_W + 1.0))]
    last = np.where((n >= 3600) & (n < 4200), 1.0, 0.0)                   # LSD frame 5 = [3000, 4200) alone reaches these
    tail = np.where(n >= 4200, 1.0, 0.0)                                  # beyond every LSD frame
    s += [('lsd_frame5_only', last * noise(0.3), last * noise(0.3)), ('beyond_lsd_frames', tail * noise(0.3), tail * noise(0.3))]
    return [(name, p.astype(np.float32), g.astype(np.float32)) for name, p, g in s]


def metric_batch(B, C, start=0):
    """[B, 4800, C] pred / gt and the slot names [B][C]: slot (start + b C + c) mod len(slots) in entry (b, c), so neighbouring
    channels carry different families."""
    slots = metric_slots()
    pred, gt = np.zeros((B, EV_N, C), np.float32), np.zeros((B, EV_N, C), np.float32)
    names = []
    for b in range(B):
        for c in range(C):
            name, p, g = slots[(start + b * C + c) % len(slots)]
            pred[b, :, c], gt[b, :, c] = p, g
            names.append(name)
    return pred, gt, names


METRIC_STARTS = {1: 38, 2: 8, 5: 23, 16: 0}                             # B = 1: dc_only, dc_only_swapped, nyquist_only, ...


def mel_slots():
    """(name, pred, gt, impulse) for sagen_eval_mel_env."""
    r = np.random.default_rng(20241022)
    n = np.arange(EV_N)
    z = np.zeros(EV_N)
    noise = lambda a: a * r.standard_normal(EV_N)
    s = []
    for i, m in enumerate(MEL_IMPULSES):
        s.append(('imp_%d' % m, _imp(m), _imp((m + 7) % EV_N, 0.5), True))
        s.append(('imp_%d_vs_silence' % m, z, _imp(m, 0.3), True))
    tone = lambda f, a, ph=0.0: a * np.sin(2 * np.pi * f * n / 48000.0 + ph)
    s += [('periodic_tone', tone(250.0, 0.7, 0.3), tone(250.0, 0.35, 0.3), False),             # 25 periods in 4800 samples
          ('tone_11900', tone(11900.0, 0.5), tone(11900.0, 0.25, 0.5), False),
          ('tone_13000', tone(13000.0, 0.5), tone(13000.0, 0.05), False),                       # above every mel band
          ('nyquist', 0.5 * np.where(n % 2 == 0, 1.0, -1.0), 0.1 * np.where(n % 2 == 0, 1.0, -1.0), False),
          ('ramp', n / 4800.0 - 0.5, 0.5 * (n / 4800.0), False),
          ('amp_1e-4', noise(1e-4), noise(1e-4), False), ('noise', noise(0.1), noise(0.3), False),
          ('identical', s[0][1], s[0][1], True), ('silent_both', z, z, False), ('silent_pred', z, noise(0.2), False)]
    return [(name, p.astype(np.float32), g.astype(np.float32), imp) for name, p, g, imp in s]


def mel_batch(B, C, start=0):
    slots = mel_slots()
    pred, gt = np.zeros((B, EV_N, C), np.float32), np.zeros((B, EV_N, C), np.float32)
    meta = []
    for b in range(B):
        for c in range(C):
            name, p, g, imp = slots[(start + b * C + c) % len(slots)]
            pred[b, :, c], gt[b, :, c] = p, g
            meta.append((name, imp))
    return pred, gt, meta


MEL_SHAPES = ((1, 1, 0), (1, 2, 3), (1, 3, 16), (2, 4, 18), (13, 5, 0), (1, 8, 5))     # (B, C, first slot); 13 x 5 = 65 crosses one finish block


# ------------------------------------------------------------------------------------------------------------------------
# sagen_eval_emd
# ------------------------------------------------------------------------------------------------------------------------
EMD_NODES = (1, 2, 63, 64, 65, 84, 96)
WAVE = 64


def emd_metric(n):
    """[n, n] fp64 metric: the product's 30 degree mesh for 84 (coincident nodes at the poles), great-circle distances of n seeded
    unit vectors otherwise - with vector 1 a duplicate of vector 0 (a zero distance and ties in every row) where n >= 3."""
    if n == 84:
        from spatialaudiogen_amd.ambisonics import angular_distance
        return np.ascontiguousarray(angular_distance(30.0), np.float64)
    r = np.random.default_rng(1000 + n)
    v = r.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if n >= 3:
        v[1] = v[0]
    cross = np.linalg.norm(np.cross(v[:, None, :], v[None, :, :]), axis=-1)
    d = np.arctan2(cross, v @ v.T)
    d = 0.5 * (d + d.T)
    np.fill_diagonal(d, 0.0)
    if n >= 3:
        d[0, 1] = d[1, 0] = 0.0
        d[1, :] = d[0, :]
        d[:, 1] = d[:, 0]
    return np.ascontiguousarray(d)


def emd_masses(p, q, var):
    """The kernel's normalisation (distance.py:128-129): var 0 = / nodes, 1 = / (sum + 0.01), in fp64 from the float32 maps."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    if var == 0:
        return p / p.size, q / q.size
    return p / (p.sum() + 0.01), q / (q.sum() + 0.01)


def emd_split(P, Q):
    """(sources, sinks) after the min(P, Q) shortcut, as emd_core.h lists them."""
    m = np.minimum(P, Q)
    return np.nonzero(P - m > 0)[0], np.nonzero((Q - m > 0) & ~(P - m > 0))[0]


def emd_serial(P, Q, C, inf=1e300, cap=4096):
    """csrc/emd_core.h step by step with one lane (EmdSerial), in Python: (EMD-hat, converged, stats).  stats counts what the case
    lists promise: 'reroutes' = sources reached back through a settled sink without demand, 'augment' = augmentations."""
    P, Q, C = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(C, np.float64)
    stats = dict(reroutes=0, augment=0, ns=0, nd=0)
    if not (np.isfinite(P).all() and np.isfinite(Q).all()):
        return float('nan'), 1, stats
    sp = sq = 0.0
    for v in range(len(P)):
        sp += P[v]; sq += Q[v]
    pen = (sp - sq if sp > sq else sq - sp) * max(C.max(), 0.0)
    src, snk = emd_split(P, Q)
    ns, nd = len(src), len(snk)
    stats['ns'], stats['nd'] = ns, nd
    m = np.minimum(P, Q)
    sup, dem = (P - m)[src].copy(), (Q - m)[snk].copy()
    cst = C[np.ix_(src, snk)].copy() if ns and nd else np.zeros((ns, nd))
    flw = np.zeros((ns, nd))
    ps, pt = np.zeros(ns), np.zeros(nd)
    ok = 1
    it = 0
    while (sup > 0).any() and (dem > 0).any():
        if it == cap:
            ok = 0
            break
        it += 1
        roots = sup > 0
        ds = np.where(roots, 0.0, inf)
        pred_s = np.full(ns, -1)
        done_s = roots.copy()
        lst = list(np.nonzero(roots)[0])
        dt, pred_t, done_t = np.full(nd, inf), np.full(nd, -1), np.zeros(nd, bool)
        jstar, D = -1, 0.0
        while True:
            for i in lst:
                v = (ds[i] + ps[i]) + cst[i] - pt
                upd = ~done_t & (v < dt)
                dt[upd] = v[upd]
                pred_t[upd] = i
            cand = np.where(done_t, np.inf, dt)
            bj = int(np.argmin(cand))                                     # the first minimum: the smaller index wins a tie
            bd = cand[bj]
            if not bd < inf:
                break
            done_t[bj] = True
            if dem[bj] > 0:
                jstar, D = bj, bd
                break
            reach = ~done_s & (flw[:, bj] > 0)
            ds[reach], pred_s[reach], done_s[reach] = bd, bj, True
            lst = list(np.nonzero(reach)[0])
            stats['reroutes'] += len(lst)
        if jstar < 0:
            ok = 0
            break
        ps += np.minimum(ds, D)
        pt += np.minimum(dt, D)
        delta, j = dem[jstar], jstar
        while True:
            i = pred_t[j]
            if pred_s[i] < 0:
                delta = min(delta, sup[i])
                break
            delta = min(delta, flw[i, pred_s[i]])
            j = pred_s[i]
        j = jstar
        dem[j] -= delta
        while True:
            i = pred_t[j]
            flw[i, j] += delta
            if pred_s[i] < 0:
                sup[i] -= delta
                break
            flw[i, pred_s[i]] -= delta
            j = pred_s[i]
        stats['augment'] += 1
    c = 0.0
    for j in range(nd):
        cj = 0.0
        for i in range(ns):
            cj += flw[i, j] * cst[i, j]
        c += cj
    return c + pen, ok, stats


def _emd_family(n, r):
    """(name, p [n], q [n]) float32 map pairs on n nodes; every one also runs with its maps swapped."""
    out = []
    u = lambda: r.random(n) + 0.05
    if n >= 65 + 1:
        for nd in sorted({1, 4, n - 65}):                                  # many sources: p above q on 65 nodes, below on nd others
            if nd < 1 or 65 + nd > n:
                continue
            q = u()
            p = q.copy()
            idx = r.permutation(n)
            p[idx[:65]] += 0.1 + r.random(65)
            p[idx[65:65 + nd]] *= 0.25
            out.append(('src65_snk%d' % nd, p, q))
    flat = np.full(n, 0.5)
    peak = np.full(n, 0.0)
    peak[r.permutation(n)[:max(1, min(3, n - 1))]] = (np.array([20.0, 12.0, 9.0])[:max(1, min(3, n - 1))])
    out.append(('diffuse_vs_plane', flat, peak))
    out.append(('diffuse_vs_plane_floor', flat, peak + 0.01))
    out.append(('random', u() * 3, u()))
    if n >= 3:
        p, q = u(), u()
        p[1], q[1] = p[0], q[0]                                            # equal masses on the duplicated node: ties in cost and mass
        p[2:] = np.round(p[2:] * 4) / 4 + 0.25
        q[2:] = np.round(q[2:] * 4) / 4 + 0.25
        out.append(('ties', p, q))
    out.append(('point_masses', np.eye(n)[0] * 2.0, np.eye(n)[n - 1] * 2.0))
    return [(name, p.astype(np.float32), q.astype(np.float32)) for name, p, q in out]


def emd_reroute_pair(n, C, tries=400):
    """A pair on which the serial core reaches a source back through a settled sink without demand (the flow of an earlier
    augmentation is rerouted) in BOTH normalisations - searched with emd_serial over seeded sparse pairs, so the list proves itself."""
    r = np.random.default_rng(7000 + n)
    for _ in range(tries):
        k = max(2, min(n // 2, 6))
        idx = r.permutation(n)
        p, q = np.zeros(n), np.zeros(n)
        p[idx[:k]] = np.round(r.random(k) * 8 + 1) / 4
        q[idx[k:2 * k]] = np.round(r.random(k) * 8 + 1) / 4
        p, q = p.astype(np.float32), q.astype(np.float32)
        if all(emd_serial(*emd_masses(p, q, v), C)[2]['reroutes'] > 0 for v in (0, 1)):
            return p, q
    return None


_EMD_CACHE = {}


def emd_cases(n):
    """[(name, p, q)] for n nodes: the families, the reroute pair where one exists (n >= 4), each also swapped."""
    if n not in _EMD_CACHE:
        C = emd_metric(n)
        fam = _emd_family(n, np.random.default_rng(500 + n))
        if n >= 4:
            rr = emd_reroute_pair(n, C)
            if rr is not None:
                fam.append(('reroute', rr[0], rr[1]))
        _EMD_CACHE[n] = fam + [(name + '_swapped', q, p) for name, p, q in fam]
    return _EMD_CACHE[n]


def emd_blocked_case(n=5):
    """A cost matrix whose off-diagonal entries are 1e300 (the solver's "no path" value): the first Dijkstra step of every problem
    that has mass to move finds no sink below it and returns through `not converged` - an ordinary return path.  Rows: identical maps,
    two pairs that differ both ways, q = 2 p (nothing to move in either normalisation), both silent.
    -> (p, q [5, n] float32, cost, expected [5, 2] by emd_serial, expected rise of the counter)."""
    r = np.random.default_rng(77)
    C = np.full((n, n), 1e300)
    np.fill_diagonal(C, 0.0)
    a, b, c = (r.random(n) * 1e-3 + 1e-4).astype(np.float32), (r.random(n) * 1e-3 + 1e-4).astype(np.float32), (r.random(n) * 1e-3).astype(np.float32)
    p = np.stack([a, a, b, c, np.zeros(n, np.float32)])
    q = np.stack([a, b, a[::-1].copy(), 2 * c, np.zeros(n, np.float32)])
    exp, count = np.zeros((len(p), 2)), 0
    for k in range(len(p)):
        for v in range(2):
            exp[k, v], ok, _ = emd_serial(*emd_masses(p[k], q[k], v), C)
            count += 1 - ok
    return p, q, C, exp, count


_EMD_REF = {}


def emd_lp_refs(n):
    """[cases, 2] LP values of emd_cases(n) (computed once per process; EMD-hat is symmetric on a symmetric metric, so a swapped pair
    shares its partner's LP)."""
    if n not in _EMD_REF:
        C = emd_metric(n)
        cases = emd_cases(n)
        half = len(cases) // 2
        ref = np.array([mo.emd_pair(p, q, C) for _, p, q in cases[:half]])
        _EMD_REF[n] = np.concatenate([ref, ref], 0)
    return _EMD_REF[n]


# ------------------------------------------------------------------------------------------------------------------------
# power maps
# ------------------------------------------------------------------------------------------------------------------------
def power_map_ref(ambi, sh, block=32768):
    """ambi [T, 4] float32, sh [P, 4] float32 -> [P] fp64: sqrt(mean_t (ambi[t] . sh[p])^2), the definition (no moments)."""
    a, s = np.asarray(ambi, np.float64), np.asarray(sh, np.float64)
    acc = np.zeros(len(s))
    for t0 in range(0, len(a), block):
        acc += ((a[t0:t0 + block] @ s.T) ** 2).sum(0)
    return np.sqrt(acc / len(a))


def power_map_bound(ref):
    ref = np.asarray(ref, np.float64)
    return 2.0 ** -23 * ref + 2.0 ** -22 * ref.max(axis=-1, keepdims=True)


def power_map_moments(ambi, sh, moments='f64'):
    """The kernels' route restated on the CPU: ten second moments, then sh S sh^T in fp64.  moments = 'f32': per-lane float32 sums
    (stride 256), a float32 tree over the 64 lanes of a wave, fp64 across the four waves - power_moments_kernel as it was;
    'f64': every sum in fp64 (products of float32 values are exact there)."""
    a = np.asarray(ambi, np.float32)
    T = len(a)
    iu = np.triu_indices(4)
    if moments == 'f64':
        a64 = a.astype(np.float64)
        S10 = np.array([(a64[:, i] * a64[:, j]).sum() for i, j in zip(*iu)])
    else:
        pad = (-T) % 256
        ap = np.concatenate([a, np.zeros((pad, 4), np.float32)])
        S10 = np.zeros(10)
        for k, (i, j) in enumerate(zip(*iu)):
            prod = (ap[:, i] * ap[:, j]).astype(np.float32).reshape(-1, 256)
            lane = np.zeros(256, np.float32)
            for row in prod:
                lane = (lane + row).astype(np.float32)
            w = lane.reshape(4, 64)
            for m in (1, 2, 4, 8, 16, 32):
                w = (w + w[:, np.arange(64) ^ m]).astype(np.float32)
            S10[k] = w[:, 0].astype(np.float64).sum()
    S = np.zeros((4, 4))
    S[iu] = S10
    S = S + S.T - np.diag(np.diag(S))
    y = np.asarray(sh, np.float32).astype(np.float64)
    e = np.einsum('pi,ij,pj->p', y, S, y)
    return np.sqrt(np.maximum(e, 0.0) / T)


PM_RANDOM_P = (1, 2, 83, 255, 256, 257)
PM_T = (1, 3, 255, 256, 257, 4800, 262144 + 513)


def pm_mesh(name):
    """'30' / '5' -> the product's SH matrix of that mesh; 'r<P>' -> a seeded random [P, 4] whose row 0 is a unit direction (1, v) and,
    for P >= 2, whose row 1 is its antipode (1, -v) bit for bit.  float32."""
    if name in ('30', '5'):
        from spatialaudiogen_amd.ambisonics import sh_matrix
        return np.ascontiguousarray(sh_matrix(float(name)), np.float32)
    P = int(name[1:])
    r = np.random.default_rng(3000 + P)
    sh = r.standard_normal((P, 4)).astype(np.float32)
    v = r.standard_normal(3)
    sh[0] = np.concatenate([[1.0], v / np.linalg.norm(v)]).astype(np.float32)
    if P >= 2:
        sh[1] = sh[0] * np.array([1, -1, -1, -1], np.float32)
    return sh


def pm_nodes(name, sh):
    """(pole, equator, generic) node indices of a mesh - or what a random matrix has of them."""
    P = len(sh)
    if name == '30':
        return (0, 40, 19)                                                # nu = -90; nu = 0 (row 3, column 4); nu = -60
    if name == '5':
        return (3, 1337, 7 * 72 + 30)                                     # nu = -90; nu = 0 (row 18, column 41); nu = -55
    return (0, min(1, P - 1), P // 2)


def pm_antipode(sh, p):
    """Index of the row closest to (1, -v) of row p, and whether it is an exact null (bit for bit the negated direction)."""
    want = sh[p].astype(np.float64) * np.array([1, -1, -1, -1])
    q = int(np.argmin(np.abs(sh.astype(np.float64) - want).sum(1)))
    return q, bool(np.array_equal(sh[q].astype(np.float64), want))


def pm_signals(sh, nodes, T, seed):
    """[(name, ambi [T, 4] float32)]: the families of the issue on a given matrix."""
    r = np.random.default_rng(seed)
    s = r.standard_normal(T)
    out = []
    for tag, p in zip(('pole', 'equator', 'generic'), nodes):
        out.append(('plane_' + tag, s[:, None] * sh[p].astype(np.float64)[None, :]))
    s2 = r.standard_normal(T)
    out.append(('two_planes', s[:, None] * sh[nodes[1]].astype(np.float64) + 0.5 * s2[:, None] * sh[nodes[2]].astype(np.float64)))
    a = 0.1 * r.standard_normal((T, 4))
    a[:, 0] += 0.75
    out.append(('dc_on_w', a))
    omni = np.zeros((T, 4))
    omni[:, 0] = s
    out.append(('omni', omni))
    out.append(('silent', np.zeros((T, 4))))
    out.append(('noise_1e-4', 1e-4 * r.standard_normal((T, 4))))
    out.append(('noise_30', 30.0 * r.standard_normal((T, 4)) * np.array([1.0, 0.3, 0.1, 0.6])))
    out.append(('plane_pow2', np.where(r.random(T) < 0.5, -1.0, 1.0)[:, None] * 2.0 ** r.integers(-3, 4, T)[:, None]
                * np.array([1.0, 0.0, 1.0, 0.0])))                        # exact in float32: toward (0, 0, 1)
    return [(name, np.ascontiguousarray(x, np.float32)) for name, x in out]


def pm_cases():
    """[(mesh name, T, nchunks)]: every mesh at T = 4800 with 13 chunks (all families, silent chunks between loud ones), every T on the
    30 degree mesh and on an odd random matrix with 1 and 2 chunks."""
    cases = [(m, 4800, 13) for m in ('30', '5') + tuple('r%d' % p for p in PM_RANDOM_P)]
    for T in PM_T:
        if T != 4800:
            cases += [('30', T, 2), ('r83', T, 1)]
    return cases


def pm_chunks(mesh, T, nchunks):
    """(sh, [names], ambi [nchunks, T, 4]) of one case: the families in order, a silent chunk between loud ones (index 1 and, from 6
    chunks on, index 5), cycled to nchunks."""
    sh = pm_mesh(mesh)
    sig = pm_signals(sh, pm_nodes(mesh, sh), T, seed=(sum(map(ord, mesh)) * 7919 + T) % 100003)
    silent = [x for x in sig if x[0] == 'silent'][0]
    loud = [x for x in sig if x[0] != 'silent']
    order = []
    k = 0
    for c in range(nchunks):
        if nchunks > 1 and c in (1, 5):
            order.append(silent)
        else:
            order.append(loud[k % len(loud)])
            k += 1
    return sh, [o[0] for o in order], np.stack([o[1] for o in order])
