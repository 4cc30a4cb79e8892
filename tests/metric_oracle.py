"""fp64 numpy / scipy restatements of the three metric families the reference's eval.py computes on the host (eval.py:172-193):
mel-LSD (myutils.py:96-106, librosa 0.6.0 written out from its formulas - librosa is not a dependency), envelope distance
(myutils.py:109-116, scipy.signal.hilbert) and EMD-hat between directional RMS maps (distance.py:100-130, pyemd 0.5.1 restated as
the partial-transport LP on scipy.optimize.linprog).  Test infrastructure: the product never imports this."""
import numpy as np

SR, N_FFT, HOP, N_MELS, FMAX = 48000, 2048, 512, 128, 12000.0


# ---- envelope ---------------------------------------------------------------------------------------------------------------
def hilbert_kernel(n):
    """g with (Hx)[k] = sum_m g[(k - m) mod n] x[m] for even n: (2/n) cot(pi k / n) at odd k, 0 at even k."""
    k = np.arange(n)
    g = np.zeros(n)
    odd = k % 2 == 1
    g[odd] = 2.0 / n / np.tan(np.pi * k[odd] / n)
    return g


def envelope(x):
    from scipy.signal import hilbert
    return np.abs(hilbert(np.asarray(x, np.float64)))


def env_mse(pred, gt):
    """myutils.compute_envelope_dist: pred / gt [T, C] -> [C]."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    return np.array([np.sqrt(np.mean((envelope(gt[:, c]) - envelope(pred[:, c])) ** 2)) for c in range(gt.shape[1])])


# ---- mel-LSD ----------------------------------------------------------------------------------------------------------------
def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f < 1000.0, f * 3.0 / 200.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m < 15.0, m * 200.0 / 3.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)))


def mel_basis(sr=SR, n_fft=N_FFT, n_mels=N_MELS, fmax=FMAX):
    """librosa 0.6.0 filters.mel(sr, n_fft, n_mels, fmin=0, fmax, htk=False, norm=1): [n_mels, 1 + n_fft // 2]."""
    freqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    edges = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    w = np.zeros((n_mels, len(freqs)))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w * (2.0 / (edges[2:n_mels + 2] - edges[:n_mels]))[:, None]


def melspectrogram(x, sr=SR):
    """librosa 0.6.0 feature.melspectrogram(y=x, sr, n_mels=128, fmax=12000): centred reflect-padded STFT (periodic Hann 2048,
    hop 512), power 2, mel basis -> [128, frames]."""
    x = np.pad(np.asarray(x, np.float64), N_FFT // 2, mode='reflect')
    nfr = 1 + (len(x) - N_FFT) // HOP
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
    frames = np.stack([x[t * HOP:t * HOP + N_FFT] * win for t in range(nfr)], 1)
    S = np.abs(np.fft.rfft(frames, axis=0)) ** 2
    return mel_basis(sr) @ S


def mel_lsd(pred, gt, sr=SR):
    """myutils.compute_lsd_dist: pred / gt [T, C] -> [C]."""
    ps = lambda s: 10 * np.log10(np.abs(s) + 1e-2)
    return np.array([np.sqrt(np.mean((ps(melspectrogram(gt[:, c], sr)) - ps(melspectrogram(pred[:, c], sr))) ** 2))
                     for c in range(np.asarray(gt).shape[1])])


# ---- EMD --------------------------------------------------------------------------------------------------------------------
def angular_distance_ref(angular_res=30.0):
    """distance.py:101-110 on the reference's mesh (distance.py:9-13)."""
    phi = np.flip(np.arange(-180., 180., angular_res)) / 180. * np.pi
    nu = np.arange(-90., 90.1, angular_res) / 180. * np.pi
    phi, nu = np.meshgrid(phi, nu)
    p = np.stack((np.cos(nu) * np.cos(phi), np.cos(nu) * np.sin(phi), np.sin(nu)), 0).reshape((3, -1))
    d = p.T @ p
    C = np.arccos(np.clip(d, -1, 1))
    # pyemd quantises the costs to 1e6 levels of max C before it solves: the 1.5e-8 rad that arccos makes of a rounded dot product
    # of 1 (the diagonal, the coincident pole nodes) become 0 there.  No other entry of a 30 degree mesh is below 0.2 rad.
    C[C < 1e-6 * C.max()] = 0.0
    return C, phi, nu


def emd_hat(P, Q, C):
    """pyemd.emd(P, Q, C) with the default extra-mass penalty, solved exactly: min sum f C over f >= 0 with row sums <= P,
    column sums <= Q, total min(sum P, sum Q); + |sum P - sum Q| max C."""
    from scipy.optimize import linprog
    from scipy.sparse import coo_matrix
    P, Q, C = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(C, np.float64)
    if not (np.isfinite(P).all() and np.isfinite(Q).all()):
        return float('nan')
    sp, sq = P.sum(), Q.sum()
    pen = abs(sp - sq) * C.max()
    tot = min(sp, sq)
    if tot <= 0:
        return pen
    s = 1.0 / max(sp, sq)                        # masses rescaled to O(1)
    n = len(P)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    rows = np.concatenate([i.ravel(), n + j.ravel()])
    A = coo_matrix((np.ones(2 * n * n), (rows, np.concatenate([np.arange(n * n)] * 2))), shape=(2 * n, n * n)).tocsr()
    r = linprog(C.ravel(), A_ub=A, b_ub=np.concatenate([P, Q]) * s, A_eq=np.ones((1, n * n)), b_eq=[tot * s], bounds=(0, None),
                method='highs-ds', options={'primal_feasibility_tolerance': 1e-10, 'dual_feasibility_tolerance': 1e-10})
    assert r.status == 0, r.message
    return r.fun / s + pen


def emd_pair(map1, map2, C):
    """distance.emd for one frame (distance.py:100-130): maps [7, 12] as eval.py passes them (flipud of the device map order) with
    the unflipped mesh -> (dir, dir2)."""
    m1, m2 = np.asarray(map1, np.float64).reshape(-1), np.asarray(map2, np.float64).reshape(-1)
    n = m1.size
    return emd_hat(m1 / n, m2 / n, C), emd_hat(m1 / (m1.sum() + 0.01), m2 / (m2.sum() + 0.01), C)
