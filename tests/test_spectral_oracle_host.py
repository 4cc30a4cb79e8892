"""spectral_oracle.py proven without a GPU, before a kernel is involved:

  * CROSS-CHECKS: stft_ref equals oracle.np_oracle.stft on the frames both define; tail_ref equals the oracle-op restatement
    test_gpu_ops._mask_ref (first order) and the torch restatement test_gpu_backward._mix_ref in fp64; at nin = 4 it equals the sum of
    four first-order tails with the bias of input channel 0;
  * THE FLOAT32 EMULATION: the five radix-4 Stockham stages of csrc/fft.hip restated in np.complex64 (same indexing, same float32
    twiddle table), the packing of two frames and the Hermitian split, on every STFT case's data and on loud/silent pairs, impulses
    and DC beside an alternating partner; and the whole tail for one case with the sigmoid, the mask sums, the packed inverse
    transforms and the overlap-add in float32.  Every element stays inside its derived bound; the worst fraction is printed;
  * MUTANTS: restatements of the kernels' structure in fp64 with one index or constant wrong.  Each is outside the bound (or leaves
    an element unwritten or not finite) on at least one element of EVERY case it can touch - so the bounds are not only wide enough
    for float32 but narrow enough to see each of these;
  * REFUSALS: the table of include/sagen.h for sagen_stft_mag against libsagen_hip.so (which loads without a GPU; these calls return
    before any launch) and against the CPU twin: the same codes and the same messages.  The audio pointer is an offset into a larger
    live buffer, so a check that were missing could not read outside an allocation.
"""
import ctypes as C

import numpy as np
import pytest

import spectral_oracle as S
from oracle import np_oracle as O

STFT_CASES, TAIL_CASES = S.stft_cases(), S.tail_cases()
F32, C64 = np.float32, np.complex64


# ------------------------------------------------------------------------------------------------------------------------
# cross-checks
# ------------------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_path():
    names = [c.name for c in STFT_CASES]
    assert len(set(names)) == len(names)
    assert {(c.f0, c.f1) for c in STFT_CASES} >= {(0, 1), (0, 2), (0, 3), (1, 4), (3, 8), (0, 8), (2, 7), (46, 173)}
    assert {c.n for c in STFT_CASES} == {2048, 3072, 3772, 52799} and {c.B for c in STFT_CASES} == {1, 2, 3}
    assert {c.outs for c in STFT_CASES} == {'both', 'mag', 'spec'}
    sp = [c for c in STFT_CASES if c.outs != 'mag']
    assert {((c.c0 - c.f0) % 2, (c.c1 - c.f0) % 2) for c in sp if c.c1 - c.c0 > 1} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    single = [c for c in sp if c.c1 - c.c0 == 1 and c.f1 - c.f0 > 1]
    assert any((c.c0 - c.f0) % 2 == 0 and c.c0 + 1 < c.f1 for c in single), 'a single frame that is the first half of a pair'
    assert any((c.c0 - c.f0) % 2 == 1 for c in single), 'a single frame that is the second half of a pair'
    assert any((c.c0 - c.f0) % 2 == 0 and c.c0 + 1 == c.f1 for c in single), 'the odd last frame'
    assert all(c.f1 <= S.frame_count(c.n) for c in STFT_CASES)
    assert {(c.K, c.B) for c in TAIL_CASES if c.nin == 1} == {(K, B) for K in (16, 32, 64) for B in (1, 3)}
    assert {(c.K, c.B) for c in TAIL_CASES if c.nin == 4} == {(16, 1), (32, 1), (64, 1), (16, 2)}


def test_stft_ref_equals_the_oracle_on_the_frames_both_define():
    audio = np.random.RandomState(3).normal(size=(2, 52799)).astype(np.float32)
    ref = O.stft(audio.astype(np.float64)[:, None, :], 1024, 4)[:, 0]                      # [B,200,1024]
    assert ref.shape[1] == S.frame_count(52799) == 200
    got = S.stft_ref(audio, 0, 200)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(S.stft_ref(audio, 46, 173), got[:, 46:173])
    for n, want in ((1023, 0), (1024, 0), (2047, 0), (2048, 4), (3072, 8), (3772, 8), (52799, 200)):
        assert S.frame_count(n) == want
        if want:
            assert O.stft(np.zeros((1, 1, n)), 1024, 4).shape[2] == want


def _tail_inputs(c, seed=0):
    dmask, spec, coeffs = S.tail_operands(c, seed)
    return dmask, spec, coeffs


def test_tail_ref_equals_the_oracle_restatements():
    from test_gpu_ops import _mask_ref
    import torch as T
    from test_gpu_backward import _mix_ref
    c = S.TailCase('x', 16, 2, 1, 3)
    dmask, spec, coeffs = _tail_inputs(c)
    got = S.tail_ref(dmask, spec, coeffs)
    full = S._full_spectrum(spec)                                                         # [B,28,1024]
    ref = _mask_ref(dmask.astype(np.float64), full[:, None], coeffs.astype(np.float64))
    assert got.shape == ref.shape == (2, 4800, 3)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    ref2 = _mix_ref(T, T.as_tensor(dmask).double(), T.as_tensor(full), T.as_tensor(coeffs).double()).numpy()
    assert np.abs(got - ref2).max() <= 1e-12 * np.abs(ref2).max()


def test_tail_ref_second_order_is_the_sum_of_first_order_tails():
    c = S.TailCase('x', 16, 1, 4, 5)
    dmask, spec, coeffs = _tail_inputs(c)
    got = S.tail_ref(dmask, spec, coeffs, 4, 5)
    want = np.zeros_like(got)
    for o0 in (0, 3):                                       # output channels three at a time through the first-order reference
        for i in range(4):
            cf = np.zeros((1, 3, 3, 17))
            no = min(3, 5 - o0)
            cf[:, :, :no] = coeffs[:, :, o0:o0 + no, i]
            if i:
                cf[..., 16] = 0.                            # the biases of input channels 1..3 are dropped (model.py:430)
            want[:, :, o0:o0 + no] += S.tail_ref(dmask[..., 16 * i:16 * i + 16], spec[:, i], cf)[:, :, :no]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_elementwise_refs():
    r = np.random.RandomState(5)
    x = r.normal(size=(2, 9, 8, 12)).astype(np.float32)
    assert np.array_equal(O.max_pool_3x3_s2_same(x)[0, 0, 0], x[0, :2, :3].max((0, 1)))          # H odd: one row of padding; W even: none before
    y = r.normal(size=(50, 4)) * 3 + 100.
    acc = np.concatenate([y.sum(0), (y * y).sum(0)])
    g, b = r.normal(size=4), r.normal(size=4)
    sc, sh = S.bn_finalize_ref(acc, 50, g, b, 1e-3)
    want = O.batch_norm_train(y, g, b, eps=float(np.float32(1e-3)))
    assert np.abs(y * sc + sh - want).max() < 1e-9
    acc0 = np.array([50 * 0.1, 50 * 0.1 * 0.1 * (1 - 1e-15)])                                   # a variance that cancels to below zero
    sc0, _ = S.bn_finalize_ref(acc0, 50, [2.0], [0.0], 1e-3)
    assert sc0[0] == 2.0 / np.sqrt(float(np.float32(1e-3)))
    v, bound, raw = S.bn_apply_relu_ref(np.array([1.0, -3.0]), np.array([2.0, 2.0]), np.array([0.5, 0.5]), np.array([1.0, 1.0]))
    assert np.array_equal(v, [3.5, 0.0]) and np.array_equal(raw, [3.5, -4.5]) and np.allclose(bound, 2 * S.U * np.array([3.5, 6.5]))
    assert np.array_equal(S.bn_apply_relu_ref(np.array([1.0]))[1], [0.0])


# ------------------------------------------------------------------------------------------------------------------------
# the float32 emulation of fft1024 (csrc/fft.hip): Stockham radix-4 autosort, 5 stages, 256 "threads", float32 twiddle table
# ------------------------------------------------------------------------------------------------------------------------
_TW = np.exp(-2j * np.pi * np.arange(1024) / 1024.)
TW32 = (_TW.real.astype(F32) + 1j * _TW.imag.astype(F32)).astype(C64)


def fft1024_f32(z, inverse=False):
    src = np.ascontiguousarray(z, dtype=C64)
    tid = np.arange(256)
    for s in range(5):
        Ns = 4 ** s
        k = tid & (Ns - 1)
        u = [src[..., tid + 256 * q] for q in range(4)]
        if s > 0:
            step = k * (256 // Ns)
            for q in (1, 2, 3):
                w = TW32[q * step]
                u[q] = (u[q] * (np.conj(w) if inverse else w)).astype(C64)
        v0, v1, v2, d = u[0] + u[2], u[0] - u[2], u[1] + u[3], u[1] - u[3]
        v3 = (d.imag - 1j * d.real).astype(C64) if not inverse else (-d.imag + 1j * d.real).astype(C64)
        j0 = ((tid - k) << 2) + k
        dst = np.empty_like(src)
        dst[..., j0], dst[..., j0 + Ns], dst[..., j0 + 2 * Ns], dst[..., j0 + 3 * Ns] = v0 + v2, v1 + v3, v0 - v2, v1 - v3
        src = dst
    return src


def stft_f32(audio, f0, f1):
    """stft_kernel in float32: (mag [B,nf,1024] float32, X [B,nf,1024] complex64)."""
    w = S.windows(audio, f0, f1).astype(F32) * S.HANN.astype(F32)
    B, nf = w.shape[:2]
    if nf % 2:
        w = np.concatenate([w, np.zeros((B, 1, 1024), F32)], 1)
    Z = fft1024_f32(w[:, 0::2] + 1j * w[:, 1::2])
    zn = np.conj(Z[..., (1024 - np.arange(1024)) & 1023])
    xa = (F32(0.5) * (Z + zn)).astype(C64)
    d = Z - zn
    xb = (F32(0.5) * d.imag - 1j * (F32(0.5) * d.real)).astype(C64)
    X = np.stack([xa, xb], 2).reshape(B, -1, 1024)[:, :nf]
    mag = np.sqrt(X.real * X.real + X.imag * X.imag)
    assert mag.dtype == F32
    return mag, X


def _stft_fraction(audio, f0, f1):
    mag, X = stft_f32(audio, f0, f1)
    ref = S.stft_ref(audio, f0, f1)
    bs, bm = S.stft_bounds(audio, f0, f1)
    tiny = 1e-300
    frac = max((np.abs(X.real - ref.real) / np.maximum(bs, tiny)).max(), (np.abs(X.imag - ref.imag) / np.maximum(bs, tiny)).max(),
               (np.abs(mag - np.abs(ref)) / np.maximum(bm, tiny)).max())
    unit = max((np.abs(X - ref) / np.maximum(bs / S.STFT_C_SPEC, tiny)).max(), 0.)
    return frac, unit


def test_the_emulation_is_a_1024_point_transform():
    z = np.random.RandomState(1).normal(size=(3, 1024)) + 1j * np.random.RandomState(2).normal(size=(3, 1024))
    assert np.abs(fft1024_f32(z) - np.fft.fft(z)).max() < 1e-4
    assert np.abs(fft1024_f32(z, True) - np.fft.ifft(z) * 1024).max() < 1e-4
    e = np.zeros(1024); e[5] = 1.
    assert np.abs(fft1024_f32(e) - _TW[(5 * np.arange(1024)) % 1024]).max() < 1e-6


def test_float32_stft_stays_inside_the_bound_on_every_case_and_on_directed_pairs():
    worst = 0., 0.
    for c in STFT_CASES:
        frac, unit = _stft_fraction(S.stft_audio(c), c.f0, c.f1)
        assert frac <= 1.0, (c.name, frac)
        worst = max(worst[0], frac), max(worst[1], unit)
    r = np.random.RandomState(9)
    directed = []
    a = r.normal(size=(1, 3072)).astype(F32); a[:, 1024 + 256:] *= 0; a[:, :1024] *= 1e3; directed.append(('loud|silent', a, 0, 2))
    a = r.normal(size=(1, 2048)).astype(F32); a[:, :256] = 0; a[:, 256:] *= 0; a[0, 100] = 1.; directed.append(('impulse', a, 0, 2))
    a = np.ones((1, 2048), F32); a[0, 1024:] = 0; a[0, 1024:1280] = (-1.) ** np.arange(256); directed.append(('dc|alternating', a, 0, 2))
    a = np.zeros((1, 2048), F32); a[0, :1280] = 1.; a[0, 256:1280] = (-1.) ** np.arange(1024); directed.append(('dc-ish|alternating', a, 0, 2))
    for name, a, f0, f1 in directed:
        frac, unit = _stft_fraction(a, f0, f1)
        assert frac <= 1.0, (name, frac)
        worst = max(worst[0], frac), max(worst[1], unit)
    print('float32 STFT emulation: at most %.3g of the bound, %.3g of 2^-24 * A' % worst)
    assert worst[1] < 4.0, 'the emulation itself is further off than a handful of roundings: something other than rounding'


def tail_f32(dmask, spec, coeffs):
    """mask_istft_kernel<K> + ola_mix_kernel in float32 (first order): sigmoid, K sequential multiply-adds, the packing
    (0,1) (2,5) (3,4), the inverse transform, the step selection per sample, the overlap-add and the bias."""
    B, _, _, K = dmask.shape
    X = S._full_spectrum(spec).astype(C64)
    frames = np.zeros((B, 28, 3, 1024), F32)
    n_all = np.arange(4800)
    for f in range(S.F_LO, S.F_HI):
        s_lo, s_hi = S.frame_steps(f)
        with np.errstate(over='ignore'):
            sg = (F32(1) / (F32(1) + np.exp(-dmask[:, f].astype(F32)))).astype(F32)              # [B,1024,K]
        E = np.zeros((B, 6, 1024), F32)
        for si, st in enumerate((s_lo, s_hi)):
            for o in range(3):
                acc = np.zeros((B, 1024), F32)
                for j in range(K):
                    acc = (acc + coeffs[:, st, o, j, None].astype(F32) * sg[:, :, j]).astype(F32)
                E[:, si * 3 + o] = acc
        km = (1024 - np.arange(1024)) & 1023
        two = s_hi != s_lo
        p = np.arange(1024)
        n = 256 * f + p - S.OUT_SHIFT
        inside = (n >= 0) & (n < 4800)
        st_n = np.where(inside, n // 1600, -1)
        for ca, cb in ((0, 1), (2, 5 if two else -1)) + (((3, 4),) if two else ()):
            ma = F32(0.5) * (E[:, ca] + E[:, ca][:, km])
            mb = F32(0.5) * (E[:, cb] + E[:, cb][:, km]) if cb >= 0 else np.zeros_like(ma)
            z = ((ma * X[:, f].real - mb * X[:, f].imag) + 1j * (ma * X[:, f].imag + mb * X[:, f].real)).astype(C64)
            Y = fft1024_f32(z, True)
            for cc, part in ((ca, Y.real), (cb, Y.imag)):
                if cc < 0:
                    continue
                sel = st_n == (s_hi if cc // 3 else s_lo)
                frames[:, f, cc % 3, sel] = (part[:, sel] * F32(1. / 1024)).astype(F32)
    out = np.zeros((B, 4800, 3), F32)
    for f in range(S.F_LO, S.F_HI):                       # ascending frames, as the kernel's loop
        p = n_all + S.OUT_SHIFT - 256 * f
        ok = (p >= 0) & (p < 1024)
        out[:, ok] = (out[:, ok] + frames[:, f][:, :, p[ok]].transpose(0, 2, 1)).astype(F32)
    bias = coeffs[..., K][:, n_all // 1600].astype(F32)                                  # [B,4800,3]
    res = (out.astype(np.float64) * 0.25 + bias).astype(F32)
    assert res.shape == (B, 4800, 3)
    return res


def test_float32_tail_stays_inside_the_bound():
    c = S.TailCase('x', 16, 1, 1, 3)
    dmask, spec, coeffs = _tail_inputs(c)
    got = tail_f32(dmask, spec, coeffs)
    ref, bound = S.tail_ref(dmask, spec, coeffs), S.tail_bound(dmask, spec, coeffs)
    frac = (np.abs(got - ref) / bound).max()
    print('float32 tail emulation: at most %.3g of the bound (%.3g of 2^-24 * A)' % (frac, frac * S.tail_c(16)))
    assert frac <= 1.0


# ------------------------------------------------------------------------------------------------------------------------
# STFT mutants: stft_kernel's structure in fp64 with one thing wrong
# ------------------------------------------------------------------------------------------------------------------------
STFT_MUTANTS = ('partner_swapped', 'has_b_ignored', 'bin_shifted', 'symmetric_hann', 'mirror_1023', 'row_unwritten')


def stft_packed(c, audio, mutant=None):
    """(mag [B,nf,1024], spec [B,nc,513] complex) as stft_kernel forms them, NaN where nothing is written.  audio: padded with NaN
    behind the buffer, so a read outside it is seen."""
    a = np.concatenate([np.asarray(audio, np.float64), np.full((c.B, 2048), np.nan)], 1)
    h = S.HANN if mutant != 'symmetric_hann' else 0.5 - 0.5 * np.cos(2 * np.pi / 1023 * np.arange(1024))
    nf, nc = c.f1 - c.f0, c.c1 - c.c0
    mag, spec = np.full((c.B, nf, 1024), np.nan), np.full((c.B, max(nc, 0), 513), np.nan + 0j)
    k = np.arange(1024)
    km = 1023 - k if mutant == 'mirror_1023' else (1024 - k) & 1023
    for fa in range(c.f0, c.f1, 2):
        fb = fa + 1
        has_b = fb < c.f1
        xa = a[:, 256 * fa:256 * fa + 1024] * h
        xb = a[:, 256 * fb:256 * fb + 1024] * h if (has_b or mutant == 'has_b_ignored') else np.zeros_like(xa)
        Z = np.fft.fft(xa + 1j * xb, axis=-1)
        zn = np.conj(Z[:, km])
        XA, XB = 0.5 * (Z + zn), -0.5j * (Z - zn)
        if mutant == 'partner_swapped' and has_b:
            XA, XB = XB, XA
        for t, X in ((fa, XA), (fb, XB)):
            if t >= c.f1:
                continue
            if mutant == 'bin_shifted' and t == c.f0:
                X = X.copy(); X[:, 100] = X[:, 101]
            if mutant == 'row_unwritten' and t == c.f1 - 1:
                continue
            mag[:, t - c.f0] = np.abs(X)
            if c.c0 <= t < c.c1:
                spec[:, t - c.c0] = X[:, :513]
    return mag, spec


def stft_verdict(c, audio, mag, spec, twin=False):
    """None if every asked-for element is finite and inside its bound, else what is wrong.  The checker the GPU tests use."""
    ref = S.stft_ref(np.nan_to_num(audio), c.f0, c.f1)
    bs, bm = S.stft_bounds(np.nan_to_num(audio), c.f0, c.f1, twin)
    if c.outs != 'spec':
        if not np.isfinite(mag).all():
            return 'mag: %d elements not finite' % (~np.isfinite(mag)).sum()
        bad = np.argwhere(np.abs(mag - np.abs(ref)) > bm)
        if bad.size:
            return 'mag: %d elements outside the bound, first %s' % (len(bad), bad[0])
    if c.outs != 'mag':
        r = ref[:, c.c0 - c.f0:c.c1 - c.f0, :513]
        b = bs[:, c.c0 - c.f0:c.c1 - c.f0]
        if not (np.isfinite(spec.real).all() and np.isfinite(spec.imag).all()):
            return 'spec: elements not finite'
        bad = np.argwhere((np.abs(spec.real - r.real) > b) | (np.abs(spec.imag - r.imag) > b))
        if bad.size:
            return 'spec: %d elements outside the bound, first %s' % (len(bad), bad[0])
    return None


def poisoned(c, audio):
    """NaN wherever the call [f0, f1) must not read: before 256 f0 and from 256 (f1 - 1) + 1024 on."""
    a = np.array(audio, np.float32)
    a[:, :256 * c.f0] = np.nan
    a[:, 256 * (c.f1 - 1) + 1024:] = np.nan
    return a


def _touches(c, mutant):
    nf = c.f1 - c.f0
    if mutant == 'partner_swapped':
        return nf >= 2
    if mutant == 'has_b_ignored':                          # the odd last frame: in mag, or in a spec window that ends with it
        return nf % 2 == 1 and (c.outs != 'spec' or c.c1 == c.f1)
    if mutant == 'bin_shifted':                            # bin 100 of the first frame: in mag, or in a spec window that holds that frame
        return c.outs != 'spec' or c.c0 == c.f0
    if mutant == 'row_unwritten':                          # the last frame's row of mag, or of a spec window that ends with it
        return c.outs != 'spec' or c.c1 == c.f1
    return True


def test_the_fp64_restatement_of_the_packed_transform_is_inside_every_bound_with_poisoned_surroundings():
    for c in STFT_CASES:
        a = poisoned(c, S.stft_audio(c))
        mag, spec = stft_packed(c, a)
        assert stft_verdict(c, a, mag, spec, twin=True) is None, c.name


@pytest.mark.parametrize('mutant', STFT_MUTANTS)
def test_stft_mutants_are_caught_on_every_case_they_touch(mutant):
    touched = 0
    for c in STFT_CASES:
        if not _touches(c, mutant):
            continue
        touched += 1
        a = poisoned(c, S.stft_audio(c))
        mag, spec = stft_packed(c, a, mutant)
        assert stft_verdict(c, a, mag, spec) is not None, '%s passes on %s' % (mutant, c.name)
    assert touched >= 5, (mutant, touched)


# ------------------------------------------------------------------------------------------------------------------------
# tail mutants: the overlap-add geometry, the step of a sample, the bias and the weights' order
# ------------------------------------------------------------------------------------------------------------------------
TAIL_MUTANTS = ('f_lo_2', 'f_lo_0', 'f_hi_23', 'f_hi_25', 'shift_1215', 'shift_1217', 'seam_from_s_lo', 'bias_wrong_step', 'hoa_bias_channel_1',
                'three_frames', 'tracks_swapped')


def tail_assemble(y, bias, f_lo=S.F_LO, f_hi=S.F_HI, shift=S.OUT_SHIFT, seam_from_s_lo=False, bias_step=0, three=False):
    """The kernels' overlap-add over live frames [f_lo, f_hi) of the time frames y [B,3,nout,28,1024] (spectral_oracle.tail_frames)."""
    B, _, nout = y.shape[:3]
    out = np.zeros((B, 4800, nout))
    n = np.arange(4800)
    for f in range(f_lo, f_hi):
        p = n + shift - 256 * f
        ok = (p >= 0) & (p < 1024)
        if three:
            ok &= p >= 256                                 # the newest of the four covering frames is dropped
        if not ok.any():
            continue
        step = np.full(4800, S.frame_steps(f)[0]) if seam_from_s_lo else n // 1600
        out[:, n[ok]] += 0.25 * np.moveaxis(y[:, step[ok], :, f, p[ok]], 0, 1)
    return out + bias[:, (n // 1600 + bias_step) % 3]


def _tail_mutant(mutant, c, ops, frames):
    dmask, spec, coeffs = ops
    y, bias = frames
    if mutant == 'tracks_swapped':
        j = np.arange(c.K) ^ 1
        y, bias = S.tail_frames(dmask, spec, np.concatenate([coeffs[..., j], coeffs[..., c.K:]], -1), c.nin, c.nout)
    if mutant == 'hoa_bias_channel_1':
        bias = coeffs.astype(np.float64)[:, :, :, 1, c.K]
    kw = {'f_lo_2': dict(f_lo=2), 'f_lo_0': dict(f_lo=0), 'f_hi_23': dict(f_hi=23), 'f_hi_25': dict(f_hi=25), 'shift_1215': dict(shift=1215),
          'shift_1217': dict(shift=1217), 'seam_from_s_lo': dict(seam_from_s_lo=True), 'bias_wrong_step': dict(bias_step=1),
          'three_frames': dict(three=True)}.get(mutant, {})
    return tail_assemble(y, bias, **kw)


@pytest.fixture(scope='module')
def tail_data():
    """Per case, once: operands, the time frames, the reference and the bound."""
    data = {}
    for c in TAIL_CASES:
        ops = _tail_inputs(c)
        data[c.name] = (c, ops, S.tail_frames(*ops, c.nin, c.nout), S.tail_ref(*ops, c.nin, c.nout), S.tail_bound(*ops, c.nin, c.nout))
    return data


def test_the_overlap_add_restatement_equals_tail_ref(tail_data):
    for c, ops, frames, ref, bound in tail_data.values():
        assert np.array_equal(tail_assemble(*frames), ref), c.name
        # frames 0 and 24..27 reach no cropped sample: widening the live range changes nothing ...
        assert np.array_equal(tail_assemble(*frames, f_lo=0, f_hi=28), ref), c.name


@pytest.mark.parametrize('mutant', TAIL_MUTANTS)
def test_tail_mutants_are_caught_on_every_case_they_touch(tail_data, mutant):
    """MASK_F_LO, MASK_F_HI and OUT_SHIFT off by one in either direction, and the rest of the list.  Two of them can touch no case:
    a live range widened to frame 0 or to frame 24 adds a frame that has no sample in the cropped window, so the VALUES cannot
    change - asserted here as harmless.  What such a kernel would do is READ rows the model does not allocate; the GPU test holds
    that with NaN rows and bit-identical outputs."""
    touched = 0
    for c, ops, frames, ref, bound in tail_data.values():
        if mutant == 'hoa_bias_channel_1' and c.nin == 1:
            continue
        touched += 1
        got = _tail_mutant(mutant, c, ops, frames)
        caught = (not np.isfinite(got).all()) or bool((np.abs(got - ref) > bound).any())
        if mutant in ('f_lo_0', 'f_hi_25'):
            assert not caught, 'frames 0 and 24 cannot reach the cropped window'
        else:
            assert caught, '%s passes on %s' % (mutant, c.name)
    assert touched >= 2


# ------------------------------------------------------------------------------------------------------------------------
# refusals of sagen_stft_mag, both libraries (include/sagen.h; csrc/stft_frames.h)
# ------------------------------------------------------------------------------------------------------------------------
_POOL = np.zeros(8192 + 52799 + 4096, np.float32)          # the audio pointer: 8192 floats into a live buffer
AUDIO = _POOL.ctypes.data + 4 * 8192
_OUT = np.zeros(4096, np.float32)
OUT = _OUT.ctypes.data
SHAPE, NULL = -2, -1

#             case                         audio  batch n      f0   f1   mag   c0  c1  spec  code
REFUSALS = [('f0_-1',                      AUDIO, 1,    52799, -1,  10,  OUT,  0,  0,  None, SHAPE),
            ('f0_-1_with_spec',            AUDIO, 1,    52799, -1,  10,  OUT,  0,  4,  OUT,  SHAPE),
            ('f1_equals_f0',               AUDIO, 1,    52799, 5,   5,   OUT,  0,  0,  None, SHAPE),
            ('f1_below_f0',                AUDIO, 1,    52799, 6,   5,   OUT,  0,  0,  None, SHAPE),
            ('f1_201_of_200',              AUDIO, 1,    52799, 46,  201, OUT,  0,  0,  None, SHAPE),
            ('f1_203_fits_no_more',        AUDIO, 1,    52799, 0,   203, OUT,  0,  0,  None, SHAPE),
            ('lone_frame_of_1024',         AUDIO, 1,    1024,  0,   1,   OUT,  0,  0,  None, SHAPE),
            ('n_2047',                     AUDIO, 1,    2047,  0,   1,   OUT,  0,  0,  None, SHAPE),
            ('f1_5_of_4',                  AUDIO, 1,    2048,  0,   5,   OUT,  0,  0,  None, SHAPE),
            ('n_0',                        AUDIO, 1,    0,     0,   1,   OUT,  0,  0,  None, SHAPE),
            ('n_negative',                 AUDIO, 1,    -4096, 0,   1,   OUT,  0,  0,  None, SHAPE),
            ('spec_c0_below_f0',           AUDIO, 1,    52799, 46,  173, OUT,  45, 117, OUT, SHAPE),
            ('spec_c1_above_f1',           AUDIO, 1,    52799, 46,  173, OUT,  89, 174, OUT, SHAPE),
            ('spec_c1_equals_c0',          AUDIO, 1,    52799, 46,  173, OUT,  89, 89, OUT,  SHAPE),
            ('spec_c1_below_c0',           AUDIO, 1,    52799, 46,  173, None, 90, 89, OUT,  SHAPE),
            ('spec_window_outside',        AUDIO, 1,    52799, 46,  100, None, 120, 130, OUT, SHAPE),
            ('batch_0',                    AUDIO, 0,    52799, 46,  173, OUT,  89, 117, OUT, SHAPE),
            ('batch_-1',                   AUDIO, -1,   52799, 46,  173, OUT,  89, 117, OUT, SHAPE),
            ('null_audio',                 None,  1,    52799, 46,  173, OUT,  89, 117, OUT, NULL),
            ('null_mag_and_spec',          AUDIO, 1,    52799, 46,  173, None, 89, 117, None, NULL)]


def stft_refusal_lines(lib):
    lines = []
    for case, audio, batch, n, f0, f1, mag, c0, c1, spec, code in REFUSALS:
        rc = lib.sagen_stft_mag(audio, batch, n, f0, f1, mag, c0, c1, spec, None)
        assert rc == code, (case, rc, lib.sagen_last_error())
        lines.append('%s %d %s' % (case, rc, lib.sagen_last_error().decode()))
    return lines


@pytest.fixture(scope='module')
def device_lib():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope='module')
def twin_lib():
    from test_op_refusals_host import _bind
    from spatialaudiogen_amd import build
    return _bind(C.CDLL(build.build_cpu_twin()))


def test_both_libraries_refuse_the_same_stft_calls_with_the_same_words(device_lib, twin_lib):
    dev, twin = stft_refusal_lines(device_lib), stft_refusal_lines(twin_lib)
    assert dev == twin
    assert not _OUT.any() and not _POOL.any(), 'a refused call wrote'
    by_case = dict(l.split(' ', 1) for l in dev)
    assert by_case['f0_-1'] == '-2 stft: frames [-1,10) are not among the 200 frames of 52799 samples'
    assert by_case['f1_201_of_200'] == '-2 stft: frames [46,201) are not among the 200 frames of 52799 samples'
    assert by_case['lone_frame_of_1024'] == '-2 stft: frames [0,1) are not among the 0 frames of 1024 samples'
    assert by_case['spec_c0_below_f0'] == '-2 stft: spec frames [45,117) must lie in [46,173)'
    assert by_case['batch_0'] == '-2 sagen_stft_mag: batch=0' and by_case['null_audio'] == '-1 sagen_stft_mag: null argument'


def test_the_twin_runs_the_legal_calls_next_to_the_refused_ones(twin_lib):
    """The model's own call, and the last legal frame of each length, are accepted (the twin runs them on the host) and equal the
    reference; mag alone and spec alone are both served."""
    audio = np.random.RandomState(0).normal(size=(1, 52799)).astype(np.float32)
    for n, f0, f1, c0, c1 in ((52799, 46, 173, 89, 117), (52799, 199, 200, 199, 200), (2048, 3, 4, 3, 4), (3772, 0, 8, 7, 8)):
        a = np.ascontiguousarray(audio[:, :n])
        mag, spec = np.full((1, f1 - f0, 1024), np.nan, np.float32), np.full((1, c1 - c0, 513, 2), np.nan, np.float32)
        assert twin_lib.sagen_stft_mag(a.ctypes.data, 1, n, f0, f1, mag.ctypes.data, c0, c1, spec.ctypes.data, None) == 0
        c = S.StftCase('x', 1, n, f0, f1, c0, c1, 'both')
        assert stft_verdict(c, a, mag.astype(np.float64), spec[..., 0] + 1j * spec[..., 1].astype(np.float64), twin=True) is None
        m2, s2 = np.full_like(mag, np.nan), np.full_like(spec, np.nan)
        assert twin_lib.sagen_stft_mag(a.ctypes.data, 1, n, f0, f1, m2.ctypes.data, -7, -9, None, None) == 0      # c0, c1 ignored without spec
        assert twin_lib.sagen_stft_mag(a.ctypes.data, 1, n, f0, f1, None, c0, c1, s2.ctypes.data, None) == 0
        assert np.array_equal(m2, mag) and np.array_equal(s2, spec)
