"""The rational polyphase FIR resampler restated for the tests, in fp64 numpy, from the definition alone (it imports nothing of the
package and knows nothing of the phase table's layout):

    g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, q = max(L, M)
    quality (Z, beta, rolloff): 'best' = (64, 14.8, 0.9476), 'fast' = (16, 8.6, 0.85)
    H = Z q, w = rolloff / q, h[k] = L w sinc(w k) I0(beta sqrt(1 - (k / H)^2)) / I0(beta), k = -H .. H
    y[n][o] = sum_m h[n M - m L] (sum_c mix[o][c] x[m][c]) over |n M - m L| <= H and 0 <= m < N_in, n < ceil(N_in L / M)

Three paths to y:
    direct_loop   the literal double loop over (n, m), channels ascending inside, m ascending outside; every product rounded, then added
    direct        the same sums in the same order with the loop over n turned into whole-array arithmetic (slot t = m - m_first(n)):
                  bit-equal to direct_loop (tests/test_resample_host.py), and fast enough for a few seconds of audio
    poly          scipy.signal.resample_poly(z, L, M, window=h / L) (scipy multiplies the window by `up`)
"""
import math

import numpy as np

PRESETS = {'best': (64, 14.8, 0.9476), 'fast': (16, 8.6, 0.85)}


def filt(rate_in, rate_out, quality='best'):
    """(L, M, H, h [2 H + 1])."""
    zeros, beta, rolloff = PRESETS[quality] if isinstance(quality, str) else quality
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    q = max(L, M)
    H, w = zeros * q, rolloff / q
    k = np.arange(-H, H + 1, dtype=np.float64)
    h = L * w * np.sinc(w * k) * np.i0(beta * np.sqrt(1. - (k / H) ** 2)) / np.i0(beta)
    return L, M, H, h


def table(rate_in, rate_out, quality='best'):
    """(L, M, H, [L][T]) built tap by tap: phase p, slot t holds h[k] for the t-th LARGEST k <= H with k = p (mod L), zero below -H."""
    L, M, H, h = filt(rate_in, rate_out, quality)
    T = (2 * H + 1 + L - 1) // L
    out = np.zeros((L, T), np.float64)
    for p in range(L):
        ks = list(range(H - (H - p) % L, -H - 1, -L))           # H - ((H - p) mod L) is the largest k <= H congruent to p
        assert len(ks) <= T and all((k - p) % L == 0 for k in ks)
        for t, k in enumerate(ks):
            out[p, t] = h[k + H]
    return L, M, H, out


def mixed(x, mix):
    """z[m][o] = sum_c mix[o][c] x[m][c], c ascending, fp64, each product rounded before it is added (from 0)."""
    x = np.asarray(x, np.float64)
    if mix is None:
        return x
    mix = np.asarray(mix, np.float64)
    z = np.zeros((x.shape[0], mix.shape[0]), np.float64)
    for c in range(x.shape[1]):
        z = z + mix[None, :, c] * x[:, c:c + 1]
    return z


def n_out(n_in, L, M):
    return -(-n_in * L // M)


def direct_loop(x, rate_in, rate_out, quality='best', mix=None):
    L, M, H, h = filt(rate_in, rate_out, quality)
    z = mixed(x, mix)
    N = z.shape[0]
    y = np.zeros((n_out(N, L, M), z.shape[1]), np.float64)
    for n in range(y.shape[0]):
        acc = np.zeros(z.shape[1], np.float64)
        for m in range(max(0, -((H - n * M) // L)), min(N - 1, (n * M + H) // L) + 1):       # ceil((n M - H) / L) .. floor((n M + H) / L)
            acc = acc + h[n * M - m * L + H] * z[m]
        y[n] = acc
    return y


def direct(x, rate_in, rate_out, quality='best', mix=None, n0=0, n=None, x0=0, rows=None):
    """The outputs n0 .. n0 + n - 1 (default: all) of the stream x; with (x0, rows) only the stream's rows x0 .. x0 + rows - 1 are
    seen and every other row counts as zero."""
    L, M, H, h = filt(rate_in, rate_out, quality)
    z = mixed(x, mix)
    N = z.shape[0]
    if rows is not None:
        seen = np.zeros(N, bool)
        seen[max(x0, 0):max(x0 + rows, 0)] = True
        z = np.where(seen[:, None], z, 0.)
    if n is None:
        n = n_out(N, L, M) - n0
    ns = np.arange(n0, n0 + n, dtype=np.int64)
    m_first = -((H - ns * M) // L)
    acc = np.zeros((n, z.shape[1]), np.float64)
    for t in range(2 * H // L + 1):
        m = m_first + t
        k = ns * M - m * L
        ok = (k >= -H) & (m >= 0) & (m < N)
        term = h[np.clip(k + H, 0, 2 * H)][:, None] * z[np.clip(m, 0, max(N - 1, 0))] if N else np.zeros_like(acc)
        acc = np.where(ok[:, None], acc + term, acc)
    return acc


def poly(x, rate_in, rate_out, quality='best', mix=None):
    from scipy.signal import resample_poly
    L, M, H, h = filt(rate_in, rate_out, quality)
    return resample_poly(mixed(x, mix), L, M, axis=0, window=h / L)


def tie_distance(v):
    """|v - nearest fp32 rounding tie| relative to |v|, per element of the fp64 array v (inf where v == 0)."""
    v = np.asarray(v, np.float64)
    f = v.astype(np.float32)
    other = np.where(f.astype(np.float64) <= v, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf)))
    tie = (f.astype(np.float64) + other.astype(np.float64)) / 2.
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(v != 0, np.abs(v - tie) / np.abs(v), np.inf)


def fuma_to_ambix():
    """First-order Furse-Malham (W X Y Z, W scaled by 1 / sqrt 2) to ACN / SN3D (W Y Z X, all factors 1)."""
    return np.array([[np.sqrt(2.), 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0]], np.float64)
