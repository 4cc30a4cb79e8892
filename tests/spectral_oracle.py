"""fp64 references, derived elementwise bounds and case lists for the spectral ops and the elementwise passes: sagen_stft_mag
(csrc/fft.hip: stft_kernel), sagen_mask_istft_mix / sagen_mask_istft_mix_hoa (mask_istft_kernel + ola_mix_kernel, mask_istft_hoa_kernel
+ ola_mix_hoa_kernel), sagen_bn_finalize, sagen_bn_apply_relu and sagen_maxpool3x3s2 (csrc/elementwise.hip).  The companion of
forward_oracle.py and trunk_oracle.py: plain numpy in float64 only, no kernel, no library.  test_spectral_oracle_host.py proves the
references against the oracle's own restatements and the bounds against a float32 emulation and against mutants before a kernel is
involved; test_gpu_spectral_ops.py holds the kernels (and, through test_cpu_twin_ops.py, the CPU twin) to them.

Bounds have the form c * 2^-24 * A, elementwise.  c counts the roundings of the kernel AS WRITTEN on the way to one output element, A is
the sum of the magnitudes those roundings are relative to.  Nothing here is tuned to what a kernel gives.

STFT (stft_kernel).  Two real frames a, b share one complex 1024-point transform: z[n] = xa[n] h[n] + i xb[n] h[n], and the Hermitian
split Xa = (Z[k] + conj Z[-k]) / 2, Xb = -i (Z[k] - conj Z[-k]) / 2 separates them.  The partner of frame t of a call [f0, f1) is
f0 + ((t - f0) ^ 1), or nothing (zeros) for an odd last frame.
    A[t] = sum_n (|xa[n]| + |xb[n]|) h[n]
Both frames enter: every rounding of the shared transform is relative to |z|, and the split hands each frame the other's rounding
errors.  A SILENT FRAME BESIDE A LOUD ONE IS THEREFORE NOT EXACTLY ZERO: it carries the loud partner's rounding noise, up to the
bound below with the partner's A (about 1e-7 of the partner's spectrum).  All-zero audio gives exact zeros.
Count, per bin, of the complex error in units of 2^-24 * A:
    1      the window product x * h (one rounding per sample; the twiddles have magnitude 1, so it reaches every bin at most once)
    5 * 7  five radix-4 stages, each: the twiddle rounded to float32 (|dw| <= 2^-24), the complex product (two products and one
           addition per component: 2 roundings on the path of each term, both components: 2 sqrt(2) <= 3) - together at most
           (1 + 3) sqrt(2) <= 5 on magnitudes - and two levels of additions (2).  The first stage has no twiddle and is counted the same.
    1      the split (one addition per component; the halving is exact)
STFT_C_SPEC = 37 holds re and im of spec separately (a component's error is at most the complex error).  The magnitude adds the two
squares, their sum and sqrtf, each at most one rounding of a quantity bounded by |X| <= A: STFT_C_MAG = 37 + 4 = 41, and
||Xa + e| - |Xa|| <= |e|.  A float32 restatement of the kernel's five Stockham stages measures at most 1.3 of 2^-24 * A (test_spectral_oracle_host.py: DC beside an alternating partner), so the
reference lies far inside and an index error (of the order of A itself: 1e5 bounds) far outside.

Tail (mask_istft_kernel / mask_istft_hoa_kernel, then the overlap-add).  With s(n) = n / 1600, frames 1..23 live (sample n of the
cropped window is offset p = n + 1216 - 256 f of frame f, four frames cover every n),
    out[b, n, o] = 1/4 sum_f real(ifft(Y_f^{o, s(n)}))[p] + bias[s(n), o],     Y^{o,s}[k] = sum_i X_i[k] sum_j w[s, o, i, j] sigmoid(m_ij[k])
    A[b, n, o]   = 1/4 sum_f 1/1024 sum_k sum_{(s', o') of frame f} sum_i |X_i,f[k]| sum_j |w[s', o', i, j]| sigmoid(m_ij,f[k])  +  |bias|
over the covering frames f, where (s', o') runs over ALL spectra the frame's workgroup transforms (the one or two steps the frame
touches x every output channel): a superset of the spectra packed with (o, s(n)) into one complex transform ((0,1) (2,5) (3,4) of
mask_istft_kernel, (ca, ca + 1) of the hoa kernel), which is what leaks into an output through the shared roundings.
Count with K = tracks (first order) or tracks per input channel (hoa):
    4      sigmoid: expf (2), 1 + e (1), the division (1); d sigmoid / sigmoid <= d e / e
    K + 6  K fused multiply-adds, the cross-lane sums (at most 6 levels: 4 over tracks, 2 over input channels) - and in the hoa kernel
           the product with X_i before the last of them, counted below
    1 + 3  the Hermitian half-sum (one addition) and the product with X (two roundings per term, both components: 3)
    35     the inverse transform, as above
    4 + 1  up to four additions of the overlap and the final fmaf(acc, 1/4, bias)
TAIL_C(K) = K + 54.  The fused epilogue (igemm_epilogue_maskmix) forms the sigmoid from v_exp_f32 and v_rcp_f32, 1 ulp each: + 2.
Where A is |bias| alone (zero weights, or no live frame below a sample) the output is the bias bit for bit: fmaf(0, 1/4, bias).

The CPU twin accumulates in double and rounds once: TWIN_C = 2 (the final rounding, and one more for whatever its own double
arithmetic leaves) in place of every count above, as test_gpu_forward_ops._bound does with n = 1.

Elementwise passes.  bn_apply_relu: fmaf(x, scale, shift) rounds once, the residual's addition once more:
|y - relu(v)| <= 2 * 2^-24 * (|x scale + shift| + |residual|), and ReLU is 1-Lipschitz; where v < -bound the result is exactly 0.
Without scale the product is fmaf(x, 1, 0) = x: one rounding (the addition) at most.  maxpool3x3s2 with scale: rounding is monotone, so
the max of the rounded values is the rounded max: one rounding, 2^-24 * |v|; without scale bit for bit.  bn_finalize: the kernel
evaluates the formula in fp64 from the accumulators and rounds scale and shift once each; 4 * 2^-24 relative leaves room for the
sqrt and the division of another fp64 library.
"""
import collections

import numpy as np

U = 2.0 ** -24
N = 1024
HOP = 256
HANN = (0.5 - 0.5 * np.cos(2 * np.pi / N * np.arange(N))).astype(np.float32).astype(np.float64)      # myutils.py:134: rounded to float32
STFT_C_SPEC, STFT_C_MAG, TWIN_C = 37, 41, 2
F_LO, F_HI, OUT_SHIFT, N_OUT, STEP, NF = 1, 24, 1216, 4800, 1600, 28     # live frames [1, 24), 768 + 448, the cropped window, 28 masked frames


def tail_c(K, fused=False):
    return K + 54 + (2 if fused else 0)


def frame_count(n_samples):
    """myutils.stft: 4 * (n_samples / 1024 - 1) frames (include/sagen.h: what sagen_stft_mag accepts)."""
    return max(4 * (n_samples // N - 1), 0)


# ------------------------------------------------------------------------------------------------------------------------
# STFT
# ------------------------------------------------------------------------------------------------------------------------
def windows(audio, f0, f1):
    """[B, f1 - f0, 1024]: frame t = samples [256 t, 256 t + 1024), unwindowed."""
    a = np.asarray(audio, np.float64)
    return np.stack([a[:, HOP * t:HOP * t + N] for t in range(f0, f1)], 1)


def stft_ref(audio, f0, f1):
    """Complex [B, f1 - f0, 1024]: np.fft.fft of the frames times the float32-rounded periodic Hann."""
    return np.fft.fft(windows(audio, f0, f1) * HANN, axis=-1)


def partner(t, f0, f1):
    """The frame that shares frame t's complex transform in a call [f0, f1), or None for the odd last one."""
    p = f0 + ((t - f0) ^ 1)
    return p if p < f1 else None


def stft_A(audio, f0, f1):
    """[B, f1 - f0]: sum_n (|xa| + |xb|) h of every frame and its partner."""
    own = (np.abs(windows(audio, f0, f1)) * HANN).sum(-1)
    A = own.copy()
    for t in range(f0, f1):
        p = partner(t, f0, f1)
        if p is not None:
            A[:, t - f0] += own[:, p - f0]
    return A


def stft_bounds(audio, f0, f1, twin=False):
    """(bound of each component of spec, bound of mag), both [B, f1 - f0, 1]."""
    A = stft_A(audio, f0, f1)[..., None]
    return (TWIN_C if twin else STFT_C_SPEC) * U * A, (TWIN_C if twin else STFT_C_MAG) * U * A


StftCase = collections.namedtuple('StftCase', 'name B n f0 f1 c0 c1 outs')      # outs: 'both' | 'mag' | 'spec'


def stft_cases():
    """The smallest calls that reach every path of stft_kernel: one frame, a pair, an odd tail, a non-zero start; spec windows at
    every alignment against the packed pairs; each output alone; slack behind the last frame; and the workload's own call."""
    cases, k = [], [0]

    def add(n, f0, f1, c0, c1, outs='both', B=None):
        B = B or (1, 3)[k[0] % 2]
        k[0] += 1
        assert 0 <= f0 < f1 <= frame_count(n) and (outs == 'mag' or f0 <= c0 < c1 <= f1)
        name = 'b%d_n%d_f%d-%d' % (B, n, f0, f1) + ('' if outs == 'mag' else '_c%d-%d' % (c0, c1)) + ('' if outs == 'both' else '_' + outs + 'only')
        cases.append(StftCase(name, B, n, f0, f1, c0, c1, outs))

    for i, (f0, f1) in enumerate([(0, 1), (0, 2), (0, 3), (1, 4), (3, 8), (0, 8), (2, 7)]):
        n = 2048 if f1 <= 4 else (3072, 3072 + 700)[i % 2]
        nf = f1 - f0
        add(n, f0, f1, f0, f1)
        add(n, f0, f1, 0, 0, 'mag')
        add(n, f0, f1, f0, f1, 'spec')
        if nf >= 2:
            add(n, f0, f1, f0, f0 + 1)                     # one frame, the first half of a pair
            add(n, f0, f1, f0 + 1, f0 + 2)                 # one frame, the second half of a pair
        if nf % 2 and nf > 1:
            add(n, f0, f1, f1 - 1, f1)                     # the odd last frame alone
        if nf >= 4:                                        # (c0 - f0, c1 - f0): odd/odd, odd/even, even/odd, even/even
            add(n, f0, f1, f0 + 1, f0 + 3)
            add(n, f0, f1, f0 + 1, f0 + 4, 'spec')
            add(n, f0, f1, f0 + 2, f0 + 3)
            add(n, f0, f1, f0 + 2, f0 + 4)
    add(3072 + 700, 0, 8, 3, 8, B=3)
    add(52799, 46, 173, 89, 117, B=2)                      # the model's own call
    return cases


def stft_audio(c, seed=0):
    return np.random.RandomState(1000 + seed).normal(size=(c.B, c.n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# mask -> iSTFT -> overlap-add -> mix
# ------------------------------------------------------------------------------------------------------------------------
def frame_steps(f):
    """The localisation steps the cropped samples of frame f fall into: (s_lo, s_hi)."""
    n_lo, n_hi = max(HOP * f - OUT_SHIFT, 0), min(HOP * f - OUT_SHIFT + N - 1, N_OUT - 1)
    return n_lo // STEP, n_hi // STEP


def _full_spectrum(spec):
    """[.., 513, 2] half spectrum -> complex [.., 1024] with the Hermitian mirror."""
    s = np.asarray(spec, np.float64)
    half = s[..., 0] + 1j * s[..., 1]
    return np.concatenate([half, np.conj(half[..., 511:0:-1])], -1)


def _canon(dmask, spec, coeffs, nin, nout):
    """The first-order and the second-order layout of include/sagen.h as one: m [B,28,1024,nin,K], X [B,nin,28,1024], w [B,3,nout,nin,K+1]."""
    dmask, coeffs = np.asarray(dmask, np.float64), np.asarray(coeffs, np.float64)
    B = dmask.shape[0]
    K = dmask.shape[3] // nin
    X = _full_spectrum(spec).reshape(B, nin, NF, N)
    return dmask.reshape(B, NF, N, nin, K), X, coeffs.reshape(B, 3, nout, nin, K + 1), B, K


def _sigmoid(m):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-m))


def tail_frames(dmask, spec, coeffs, nin=1, nout=3):
    """(y [B, 3, nout, 28, 1024], bias [B, 3, nout]): y[b, s, o, f] = real(ifft(sum_i X_i,f sum_j w[s,o,i,j] sigmoid(m_ij,f))), the
    time frame of every (step, output) spectrum of every one of the 28 frames, and the bias of input channel 0 (model.py:430)."""
    m, X, w, B, K = _canon(dmask, spec, coeffs, nin, nout)
    y = np.empty((B, 3, nout, NF, N))
    for f in range(NF):
        E = np.einsum('bkij,bsoij->bsoik', _sigmoid(m[:, f]), w[..., :K])                # [B,3,nout,nin,1024]
        y[:, :, :, f] = np.fft.ifft((E * X[:, None, None, :, f]).sum(3), axis=-1).real
    return y, w[:, :, :, 0, K]


def tail_ref(dmask, spec, coeffs, nin=1, nout=3):
    """model.py:326-347 + myutils.istft + crop + model.py:421-434 restated per (step, output) spectrum: [B, 4800, nout] in fp64.
    dmask [B,28,1024,nin*K], spec [B,(nin,)28,513,2], coeffs [B,3,nout,(nin,)K+1] as sagen_mask_istft_mix(_hoa) take them.  Every one of
    the 28 frames is transformed, as the reference does; those that reach no cropped sample are then simply never added."""
    y, bias = tail_frames(dmask, spec, coeffs, nin, nout)
    out = np.zeros((y.shape[0], N_OUT, nout))
    n = np.arange(N_OUT)
    step = n // STEP
    for f in range(NF):
        p = n + OUT_SHIFT - HOP * f
        ok = (p >= 0) & (p < N)
        if ok.any():
            out[:, n[ok]] += 0.25 * np.moveaxis(y[:, step[ok], :, f, p[ok]], 0, 1)       # (the two index arrays come first: [n, B, nout])
    return out + bias[:, step]


def tail_A(dmask, spec, coeffs, nin=1, nout=3):
    """[B, 4800, nout]: the magnitude sum of the module docstring (all spectra of each covering live frame, plus |bias|)."""
    m, X, w, B, K = _canon(dmask, spec, coeffs, nin, nout)
    G = np.zeros((B, NF))
    for f in range(F_LO, F_HI):
        steps = sorted(set(frame_steps(f)))
        aw = np.abs(w[:, steps][..., :K]).sum((1, 2))                                    # [B,nin,K]: summed over the frame's (s', o')
        G[:, f] = (np.einsum('bkij,bij->bki', _sigmoid(m[:, f]), aw) * np.abs(X[:, :, f]).transpose(0, 2, 1)).sum((1, 2)) / N
    n = np.arange(N_OUT)
    A = np.zeros((B, N_OUT))
    for f in range(F_LO, F_HI):
        p = n + OUT_SHIFT - HOP * f
        ok = (p >= 0) & (p < N)
        A[:, ok] += 0.25 * G[:, f, None]
    out = A[..., None] + np.abs(w[:, :, :, 0, K])[:, n // STEP]
    assert out.shape == (B, N_OUT, nout)
    return out


def tail_bound(dmask, spec, coeffs, nin=1, nout=3, twin=False, fused=False):
    K = np.asarray(dmask).shape[3] // nin
    return (TWIN_C if twin else tail_c(K, fused)) * U * tail_A(dmask, spec, coeffs, nin, nout)


TailCase = collections.namedtuple('TailCase', 'name K B nin nout')


def tail_cases():
    first = [TailCase('k%d_b%d' % (K, B), K, B, 1, 3) for K in (16, 32, 64) for B in (1, 3)]
    hoa = [TailCase('hoa_k%d_b%d' % (K, B), K, B, 4, 5) for K, B in ((16, 1), (32, 1), (64, 1), (16, 2))]
    return first + hoa


def tail_operands(c, seed=0):
    """(dmask, spec, coeffs) in float32 and the layouts of include/sagen.h: logits 2 * normal, coefficients normal / sqrt(K), spec =
    stft_ref of random audio rounded to float32."""
    r = np.random.RandomState(2000 + 97 * seed + c.K + 7 * c.B + c.nin)
    audio = r.normal(size=(c.B * c.nin, HOP * (NF - 1) + N))
    X = stft_ref(audio, 0, NF)[..., :513]
    spec = np.stack([X.real, X.imag], -1).astype(np.float32)
    dmask = (2.0 * r.normal(size=(c.B, NF, N, c.nin * c.K))).astype(np.float32)
    if c.nin == 1:
        return dmask, spec.reshape(c.B, NF, 513, 2), (r.normal(size=(c.B, 3, c.nout, c.K + 1)) / np.sqrt(c.K)).astype(np.float32)
    return dmask, spec.reshape(c.B, c.nin, NF, 513, 2), (r.normal(size=(c.B, 3, c.nout, c.nin, c.K + 1)) / np.sqrt(c.K)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# the elementwise passes
# ------------------------------------------------------------------------------------------------------------------------
def bn_finalize_ref(acc, count, gamma, beta, eps):
    """(scale, shift) in fp64 from the fp64 accumulators acc = [sum | sum of squares] per channel, by the kernel's own formula: biased
    variance, clamped at 0, eps as given."""
    acc = np.asarray(acc, np.float64)
    C = acc.size // 2
    inv = 1.0 / float(count)
    mean = acc[:C] * inv
    var = np.maximum(acc[C:] * inv - mean * mean, 0.0)
    scale = np.asarray(gamma, np.float64) / np.sqrt(var + float(np.float32(eps)))
    return scale, np.asarray(beta, np.float64) - mean * scale


def bn_apply_relu_ref(x, scale=None, shift=None, residual=None):
    """(relu(v), bound, v) with v = x * scale + shift (+ residual) in fp64 and the bound of the module docstring: one rounding for the
    fused multiply-add where there is a scale, one for the residual's addition where there is a residual - two at most."""
    x = np.asarray(x, np.float64)
    v = x if scale is None else x * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    r = np.zeros_like(v) if residual is None else np.asarray(residual, np.float64)
    roundings = (scale is not None) + (residual is not None)
    bound = roundings * U * (np.abs(v) + np.abs(r))
    v = v + r
    return np.maximum(v, 0.0), bound, v
