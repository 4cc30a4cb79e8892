"""The audio side of the network and the elementwise passes, op by op through the C ABI, against the plain fp64 references and the DERIVED
elementwise bounds of spectral_oracle.py (its docstring holds the derivations; test_spectral_oracle_host.py proves the references, the
bounds against a float32 emulation, and that each bound sees every mutant).  The companion of test_gpu_forward_ops.py for
csrc/fft.hip (stft_kernel, mask_istft_kernel<16|32|64> + ola_mix_kernel, mask_istft_hoa_kernel + ola_mix_hoa_kernel) and
csrc/elementwise.hip (bn_finalize, bn_apply_relu, maxpool3x3s2).  With SAGEN_LIB naming the CPU twin the same tests run on host tensors
(test_cpu_twin_ops.py), with the twin's own count of roundings (spectral_oracle.TWIN_C).

Every output is prefilled with NaN and has a NaN guard slice behind it: an element no kernel writes fails, a write past the end fails.
Every input that must not be read is NaN inside an allocation the test owns: nothing here reads or writes outside live memory, and
no test provokes a fault.  Each test prints, per case, the worst element's fraction of its bound as 'SPECTRAL {json}' (the source of
profiles/spectral_ops.jsonl: measurements, not bars).

sagen_stft_mag, per case of spectral_oracle.stft_cases() (one frame, a pair, an odd tail, a non-zero start, spec windows at every
alignment against the packed pairs, mag only / spec only / both, slack behind the last frame, B 1 and 3, and the model's own call):
  * random audio: mag within STFT_C_MAG * 2^-24 * A and both components of spec within STFT_C_SPEC * 2^-24 * A of the fp64 transform,
    A = sum (|xa| + |xb|) hann over the frame and the partner that shares its complex transform; the 2e-5 RMS bar beside it;
  * reads only its frames: NaN in every sample before 256 f0 and from 256 (f1 - 1) + 1024 on (slack included) and in the rows of
    the allocation before and behind the audio; the outputs are bit for bit those of the clean call;
  * partial outputs: mag alone and spec alone give bit for bit what the call with both gives;
  * directed signals under the same bound: an impulse at sample m in {0, 1, 255, 256, 511, 1023} of the first and of the second frame
    of a pair (every bin hann[m], the phase pins the bin), a constant (bins 0, +-1: 512 c, 256 c), the alternating sequence (bins
    511, 512, 513), and all-zero audio, whose mag and spec are exactly 0;
  * a loud frame (1e3) beside a silent one, in either half of the pair: the silent frame is NOT exactly zero - it holds the partner's
    rounding noise - and is under its bound, which contains the loud partner's A.  The measured size is printed.

sagen_mask_istft_mix and sagen_mask_istft_mix_hoa, per case of spectral_oracle.tail_cases() (K 16, 32, 64 x B 1, 3; second order
nsep 16, 32, 64 at B 1 and 16 at B 2):
  * random operands (logits 2 * normal, coefficients normal / sqrt(K), spec = stft_ref of random audio): within TAIL_C(K) * 2^-24 * A
    elementwise, A = the magnitude sum of the spectra that share the output's frames (spectral_oracle.tail_A), and RMS < 2e-5;
  * dead frames are never read: rows 0 and 24..27 of dmask and of spec (every input channel) NaN - the output is finite and bit for
    bit that of the call with zeros there (the model hands the kernel a 23-row buffer);
  * zero weights: the output is the bias of its step bit for bit;
  * one live frame at a time (K 16, the 28 frames as B = 7 x 4 calls; second order frames 0, 1, 23, 24 in one call): all-pass mask,
    spec non-zero in frame f only - outside [256 f - 1216, 256 f - 193] the output is the step's bias bit for bit, inside within the
    bound, and for f in {0, 24..27} the whole output is the bias;
  * step seams: one-hot coefficients per step, step s passes the s-th third of the bins of track s: n = 1599, 1600, 3199, 3200 and
    their neighbours (all samples, in fact) inside the bound;
  * packed partners: output 0 = 1e3 x output 1, output 2 zero - output 2 is the bias bit for bit wherever its spectrum shares its
    transform with nothing or with another zero spectrum (first order: everywhere), under the bound elsewhere, and so is output 1;
  * saturated logits +-88, +-100, +-1e4: finite and inside the bound; all logits >= 88 give bit for bit the all-pass output (float32
    expf(-88) vanishes beside 1) and all logits <= -100 the bias bit for bit (expf overflows to inf, 1 / inf = 0);
  * refusals: K = 24, a scratch one byte short, batch 0 and (nin, nout) != (4, 5) return a negative status and leave the output NaN.

The elementwise passes:
  * bn_apply_relu: C in {4, 12, 20, 64, 100, 512} x 1, 3, 257 pixels x with / without scale+shift x with / without residual, scales of
    both signs and one 0, and C 12 and 64 with more than 4096 x 256 float4 (the grid-stride loop's second pass; C / 4 = 3 on the gcd
    branch of channel_aligned_grid).  Bound: one rounding per operation present, 2 * 2^-24 * (|x scale + shift| + |residual|) at
    most; results the reference puts below -bound are exactly 0;
  * maxpool3x3s2: H, W in {1, 2, 3, 8, 9}, C in {4, 12, 64}, and one shape beyond one grid pass; without scale bit for bit the oracle,
    with scale within one rounding of the fp64 value and exactly 0 where the window's maximum is negative;
  * bn_finalize: C in {4, 12, 100, 512}, a channel of variance 0 and large mean (the accumulators cancel, the clamp decides), gamma 0
    (scale exactly 0, shift exactly beta), within 4 * 2^-24 relative of the fp64 formula, the slice behind scale[C] / shift[C] untouched.

The tail inside the network (audio-only networks, B = 2 and 5):
  * the two-kernel form on the device's own inputs, nsep 16, 32 (materialize_mask = 1), 64: the logits (deconv1 rows 44..66 = frames
    1..23), the STFT and the localisation coefficients are read back through net.intermediate, and the network's output holds the tail's
    bound against tail_ref of those three tensors; `mag` and `stft` hold the STFT's bound against stft_ref of the input audio;
  * the fused epilogue (igemm_epilogue_maskmix; nsep 32, default switches) on EXACT logits: deconv2 with zero weights and integer biases
    0..3, deconv1 with zero weights on the encoder half of cat1 and integers -2..2 on the decoder half, integer biases, everything else
    random.  The logits are then exact integers (forward_oracle.deconv_ref in fp64); under materialize_mask = 1 the device's logits equal
    them bit for bit, and the default forward holds TAIL_C(32) + 2 (v_exp_f32, v_rcp_f32: 1 ulp each) against tail_ref(integer logits,
    device stft, device coeffs); fp16x2_saturations is 0; the profiler rows name the fused tile (conv3g_kernel<..,true,1>, or an
    igemm3_kernel tile where the planes are switched off) and mask_istft_kernel, and the logits cannot be asked for after it.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import spectral_oracle as S
from oracle import np_oracle as O
from test_spectral_oracle_host import stft_verdict, poisoned
from util import ensure_lib, rel_rms_err

pytestmark = pytest.mark.gpu

TWIN = os.path.basename(os.environ.get('SAGEN_LIB', '')) == 'libsagen_cpu.so'
TOL = 2e-5
U = S.U
STFT_CASES, TAIL_CASES = S.stft_cases(), S.tail_cases()


@pytest.fixture(scope='module')
def T():
    import torch
    if not TWIN:
        assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    ensure_lib()
    return torch


def _dev(T, a, dtype=np.float32):
    if a is None:
        return None
    t = T.as_tensor(np.ascontiguousarray(a, dtype=dtype))
    return t if TWIN else t.cuda()


def _guarded(T, shape, dtype=None):
    """A NaN-filled output with one more leading slice behind it, which must still be all NaN after the call."""
    big = T.full((shape[0] + 1,) + tuple(shape[1:]), float('nan'), dtype=dtype or T.float32, device='cpu' if TWIN else 'cuda')
    return big[:shape[0]], big[shape[0]:]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(T):
    return None if TWIN else C.c_void_p(T.cuda.current_stream().cuda_stream)


def _sync(T):
    if not TWIN:
        T.cuda.synchronize()


def _lib():
    from spatialaudiogen_amd import _lib as L
    return L.lib(), L


def _record(op, case, what, fraction, **more):
    print('SPECTRAL ' + json.dumps(dict(dict(op=op, case=case, what=what, worst_fraction_of_bound=float('%.4g' % fraction)), **more), sort_keys=True))


def _frac(diff, bound):
    return float((diff / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# sagen_stft_mag
# ------------------------------------------------------------------------------------------------------------------------
def run_stft(T, c, audio, outs=None, expect=0):
    """The call of case c on `audio` [B, n], which lies between two NaN rows of one allocation.  (mag [B,nf,1024] float32 or None,
    spec [B,nc,513] complex64-as-pairs or None) as numpy; guards checked."""
    outs = outs or c.outs
    lib, L = _lib()
    big = np.full((c.B + 2, c.n), np.nan, np.float32)
    big[1:c.B + 1] = audio
    big = _dev(T, big)
    mag, mguard = _guarded(T, (c.B, c.f1 - c.f0, 1024)) if outs != 'spec' else (None, None)
    spec, sguard = _guarded(T, (c.B, c.c1 - c.c0, 513, 2)) if outs != 'mag' else (None, None)
    rc = lib.sagen_stft_mag(_ptr(big[1]), c.B, c.n, c.f0, c.f1, _ptr(mag), c.c0, c.c1, _ptr(spec), _stream(T))
    _sync(T)
    assert rc == expect, (rc, lib.sagen_last_error())
    for g in (mguard, sguard):
        assert g is None or bool(T.isnan(g).all()), 'written past an output'
    return (None if mag is None else mag.cpu().numpy()), (None if spec is None else spec.cpu().numpy())


def _cplx(spec):
    return None if spec is None else spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64)


def _stft_fraction(c, audio, mag, spec):
    ref = S.stft_ref(audio, c.f0, c.f1)
    bs, bm = S.stft_bounds(audio, c.f0, c.f1, TWIN)
    fr = 0.0
    if mag is not None:
        fr = max(fr, _frac(np.abs(mag - np.abs(ref)), np.broadcast_to(bm, mag.shape)))
    if spec is not None:
        r, b = ref[:, c.c0 - c.f0:c.c1 - c.f0, :513], np.broadcast_to(bs[:, c.c0 - c.f0:c.c1 - c.f0], spec.shape)
        fr = max(fr, _frac(np.abs(spec.real - r.real), b), _frac(np.abs(spec.imag - r.imag), b))
    return fr, ref


def _check_stft(c, audio, mag, spec, what):
    """Finite, inside the elementwise bound (the host test's checker), the RMS bar; records the worst fraction."""
    clean = np.nan_to_num(audio)
    v = stft_verdict(c._replace(outs='both' if mag is not None and spec is not None else 'mag' if spec is None else 'spec'), clean,
                     None if mag is None else mag.astype(np.float64), _cplx(spec), twin=TWIN)
    fr, ref = _stft_fraction(c, clean, mag, _cplx(spec))
    _record('stft_mag', c.name, what, fr)
    assert v is None, (c.name, what, v)
    return ref


@pytest.mark.parametrize('case', STFT_CASES, ids=lambda c: c.name)
def test_stft_sweep(T, case):
    c = case
    audio = S.stft_audio(c)
    mag, spec = run_stft(T, c, audio)
    ref = _check_stft(c, audio, mag, spec, 'random')
    if mag is not None and np.abs(ref).max() > 0:
        assert rel_rms_err(mag, np.abs(ref)) < TOL
    if spec is not None:
        r = ref[:, c.c0 - c.f0:c.c1 - c.f0, :513]
        assert rel_rms_err(np.stack([spec[..., 0], spec[..., 1]]), np.stack([r.real, r.imag])) < TOL
    # reads only its frames: NaN everywhere else - bit for bit the clean call
    mag_p, spec_p = run_stft(T, c, poisoned(c, audio))
    for got, want in ((mag_p, mag), (spec_p, spec)):
        assert got is None or (np.isfinite(got).all() and np.array_equal(got, want)), 'the call read outside its frames'
    # partial outputs: bit for bit the call with both
    if c.outs == 'both':
        mag_only, none = run_stft(T, c, audio, 'mag')
        none2, spec_only = run_stft(T, c, audio, 'spec')
        assert none is None and none2 is None and np.array_equal(mag_only, mag) and np.array_equal(spec_only, spec)


PAIR = S.StftCase('pair', 1, 2048, 0, 2, 0, 2, 'both')


@pytest.mark.parametrize('half', [0, 1])
@pytest.mark.parametrize('m', [0, 1, 255, 256, 511, 1023])
def test_stft_impulse_pins_every_bin(T, m, half):
    """An impulse at sample m of frame `half` of the pair [0, 2), random samples where only the other frame sees them: every bin of
    the impulse's frame is hann[m] exp(-2 pi i k m / 1024)."""
    audio = np.zeros((1, 2048), np.float32)
    r = np.random.RandomState(m + 7 * half)
    if half == 0:
        audio[0, 1024:1280] = r.normal(size=256)
    else:
        audio[0, :256] = r.normal(size=256)
    audio[0, 256 * half + m] = 1.0
    mag, spec = run_stft(T, PAIR, audio)
    ref = _check_stft(PAIR._replace(name='impulse_m%d_half%d' % (m, half)), audio, mag, spec, 'impulse')
    want = S.HANN[m] * np.exp(-2j * np.pi * np.arange(1024) * m / 1024.)
    assert np.abs(ref[0, half] - want).max() < 1e-12, 'the directed signal is not what the docstring says'
    assert np.abs(np.abs(ref[0, half]) - S.HANN[m]).max() < 1e-12


def test_stft_constant_alternating_and_zero(T):
    c0 = 0.75
    audio = np.full((1, 2048), c0, np.float32)
    mag, spec = run_stft(T, PAIR, audio)
    ref = _check_stft(PAIR._replace(name='constant'), audio, mag, spec, 'constant')
    assert abs(ref[0, 0, 0] - 512 * c0) < 1e-3 and abs(ref[0, 0, 1] + 256 * c0) < 1e-3 and abs(ref[0, 0, 1023] + 256 * c0) < 1e-3
    assert np.abs(ref[0, :, 2:1023]).max() < 1e-3, 'every other bin is zero up to the rounding of the window'
    bm = S.stft_bounds(audio, 0, 2, TWIN)[1]
    assert (np.abs(mag[:, :, 2:1023]) <= bm + 1e-3).all()
    audio = ((-1.0) ** np.arange(2048))[None].astype(np.float32)
    mag, spec = run_stft(T, PAIR, audio)
    ref = _check_stft(PAIR._replace(name='alternating'), audio, mag, spec, 'alternating')
    assert abs(abs(ref[0, 0, 512]) - 512) < 1e-3 and abs(abs(ref[0, 0, 511]) - 256) < 1e-3 and abs(abs(ref[0, 0, 513]) - 256) < 1e-3
    for c in (PAIR, S.StftCase('zero3', 3, 2048, 0, 3, 1, 3, 'both')):
        mag, spec = run_stft(T, c, np.zeros((c.B, c.n), np.float32))
        assert not mag.any() and not spec.any(), 'all-zero audio gives exact zeros'


@pytest.mark.parametrize('loud', [0, 1])
def test_stft_silent_frame_beside_a_loud_one(T, loud):
    """Frames 0 and 1 overlap in samples 256..1023, so one of them is silent only if the audio lives in the 256 samples the other
    does not see.  The silent frame's reference is exactly zero; what the kernel gives is the partner's rounding noise."""
    audio = np.zeros((1, 2048), np.float32)
    lo = 0 if loud == 0 else 1024
    audio[0, lo:lo + 256] = 1e3 * np.random.RandomState(loud).normal(size=256)
    mag, spec = run_stft(T, PAIR, audio)
    ref = _check_stft(PAIR._replace(name='loud%d_silent%d' % (loud, 1 - loud)), audio, mag, spec, 'loud|silent')
    silent = 1 - loud
    assert not ref[0, silent].any() and np.abs(ref[0, loud]).max() > 1e3
    bm = float(S.stft_bounds(audio, 0, 2, TWIN)[1][0, silent, 0])
    size = float(np.abs(mag[0, silent]).max())
    _record('stft_mag', 'loud%d_silent%d' % (loud, 1 - loud), 'silent frame: max |mag|', size / bm, max_abs=size, bound=bm,
            loud_frame_max=float(np.abs(ref[0, loud]).max()))
    assert size <= bm


# ------------------------------------------------------------------------------------------------------------------------
# sagen_mask_istft_mix / sagen_mask_istft_mix_hoa
# ------------------------------------------------------------------------------------------------------------------------
def run_tail(T, c, dmask, spec, coeffs, expect=0, short=0, batch=None, ntracks=None, nin=None, nout=None):
    """The op of case c; out [B,4800,nout] as numpy (NaN where nothing was written); guard and scratch size checked."""
    lib, L = _lib()
    B = c.B if batch is None else batch
    out, guard = _guarded(T, (c.B, 4800, c.nout))
    d, s, w = _dev(T, dmask), _dev(T, spec), _dev(T, coeffs)
    if c.nin == 1:
        need = int(lib.sagen_mask_istft_mix_scratch_bytes(max(B, 1)))
    else:
        need = int(lib.sagen_mask_istft_mix_hoa_scratch_bytes(max(B, 1), c.nout))
    scratch = T.empty((need + 3) // 4 + 64, dtype=T.float32, device=out.device)
    K = c.K if ntracks is None else ntracks
    if c.nin == 1:
        rc = lib.sagen_mask_istft_mix(_ptr(d), _ptr(s), _ptr(w), B, K, _ptr(out), _ptr(scratch), need - short, _stream(T))
    else:
        rc = lib.sagen_mask_istft_mix_hoa(_ptr(d), _ptr(s), _ptr(w), B, K, c.nin if nin is None else nin, c.nout if nout is None else nout,
                                          _ptr(out), _ptr(scratch), need - short, _stream(T))
    _sync(T)
    if expect == 0:
        assert rc == 0, (rc, lib.sagen_last_error())
    else:
        assert rc < 0 and len(lib.sagen_last_error()) > 10, (rc, lib.sagen_last_error())
    assert bool(T.isnan(guard).all()), 'written past the output'
    return out.cpu().numpy()


def _check_tail(c, ops, got, what, rms_bar=True, fused=False):
    ref, bound = S.tail_ref(*ops, c.nin, c.nout), S.tail_bound(*ops, c.nin, c.nout, twin=TWIN, fused=fused)
    assert np.isfinite(got).all(), (c.name, what, 'elements not written or not finite', int((~np.isfinite(got)).sum()))
    diff = np.abs(got - ref)
    fr = _frac(diff, bound)
    _record('mask_istft_mix' + ('_hoa' if c.nin > 1 else ''), c.name, what, fr)
    bad = np.argwhere(diff > bound)
    assert bad.size == 0, (c.name, what, len(bad), [(tuple(b), float(got[tuple(b)]), float(ref[tuple(b)]), float(bound[tuple(b)])) for b in bad[:6]])
    if rms_bar:
        assert rel_rms_err(got, ref) < TOL
    return ref, bound


def _bias_of(c, coeffs):
    """[B,4800,nout] float32: the bias of each sample's step (input channel 0 at second order)."""
    b = coeffs[..., c.K] if c.nin == 1 else coeffs[:, :, :, 0, c.K]
    return np.ascontiguousarray(b[:, np.arange(4800) // 1600]).astype(np.float32)


DEAD = [0, 24, 25, 26, 27]


@pytest.mark.parametrize('case', TAIL_CASES, ids=lambda c: c.name)
def test_tail_sweep(T, case):
    c = case
    dmask, spec, coeffs = ops = S.tail_operands(c)
    got = run_tail(T, c, *ops)
    _check_tail(c, ops, got, 'random')
    # dead frames are never read: NaN there, against zeros there
    dn, sn, dz, sz = dmask.copy(), spec.copy(), dmask.copy(), spec.copy()
    dn[:, DEAD], dz[:, DEAD] = np.nan, 0.0
    if c.nin == 1:
        sn[:, DEAD], sz[:, DEAD] = np.nan, 0.0
    else:
        sn[:, :, DEAD], sz[:, :, DEAD] = np.nan, 0.0
    with_nan, with_zero = run_tail(T, c, dn, sn, coeffs), run_tail(T, c, dz, sz, coeffs)
    assert np.isfinite(with_nan).all(), 'a dead frame was read'
    assert np.array_equal(with_nan, with_zero) and np.array_equal(with_nan, got)
    # zero weights: the bias, bit for bit
    wz = coeffs.copy()
    wz[..., :c.K] = 0.0
    assert np.array_equal(run_tail(T, c, dmask, spec, wz), _bias_of(c, wz))


def _live_frame_ops(c, frames_of_b, seed):
    """All-pass logits, spec non-zero only in frame frames_of_b[b] of window b (every input channel)."""
    dmask, spec, coeffs = S.tail_operands(c, seed)
    dmask[:] = 40.0
    keep = np.zeros_like(spec)
    for b, f in enumerate(frames_of_b):
        if c.nin == 1:
            keep[b, f] = spec[b, f]
        else:
            keep[b, :, f] = spec[b, :, f]
    return dmask, keep, coeffs


def _check_one_live_frame(T, c, frames_of_b, seed):
    ops = _live_frame_ops(c, frames_of_b, seed)
    got = run_tail(T, c, *ops)
    _check_tail(c, ops, got, 'one live frame %s' % (frames_of_b,), rms_bar=False)
    bias, n = _bias_of(c, ops[2]), np.arange(4800)
    for b, f in enumerate(frames_of_b):
        inside = (n >= 256 * f - 1216) & (n <= 256 * f - 193) if f not in DEAD else np.zeros(4800, bool)
        assert np.array_equal(got[b, ~inside], bias[b, ~inside]), 'frame %d reaches a sample outside its 1024' % f
        if f not in DEAD:
            assert (got[b, inside] != bias[b, inside]).mean() > 0.9, 'frame %d does not reach its own samples' % f


@pytest.mark.parametrize('first', [0, 7, 14, 21])
def test_tail_one_live_frame_at_a_time(T, first):
    _check_one_live_frame(T, S.TailCase('k16_b7_f%d' % first, 16, 7, 1, 3), list(range(first, first + 7)), first)


def test_tail_one_live_frame_second_order(T):
    _check_one_live_frame(T, S.TailCase('hoa_k16_b4', 16, 4, 4, 5), [0, 1, 23, 24], 3)


@pytest.mark.parametrize('case', [S.TailCase('k16_b1', 16, 1, 1, 3), S.TailCase('hoa_k16_b1', 16, 1, 4, 5)], ids=lambda c: c.name)
def test_tail_step_seams(T, case):
    """Step s hears track s alone, and track s passes only the s-th third of the bins: a sample given the wrong step's spectrum, or
    the wrong step's bias, is off by the whole signal."""
    c = case
    dmask, spec, coeffs = S.tail_operands(c, 5)
    dmask[:] = -40.0
    k = np.arange(1024)
    third = np.minimum(k, 1024 - k) * 3 // 513                                  # the same third for a bin and its mirror
    for s in range(3):
        for i in range(c.nin):
            dmask[:, :, third == s, i * c.K + s] = 40.0
    w = np.zeros_like(coeffs)
    w[..., c.K] = coeffs[..., c.K]
    for s in range(3):
        w[:, s, ..., s] = 1.0 + 0.25 * s
    got = run_tail(T, c, dmask, spec, w)
    ref, bound = _check_tail(c, (dmask, spec, w), got, 'step seams', rms_bar=False)
    seam = np.r_[1596:1604, 3196:3204]
    _record('mask_istft_mix' + ('_hoa' if c.nin > 1 else ''), c.name, 'samples 1596..1603, 3196..3203', _frac(np.abs(got - ref)[:, seam], bound[:, seam]))
    wrong = S.tail_ref(dmask, spec, w[:, [0, 0, 1]], c.nin, c.nout)             # every step one too early: what a seam sample would get
    assert (np.abs(wrong - ref)[:, [1600, 3200]] > 100 * bound[:, [1600, 3200]]).any(-1).all(), 'the seam is not visible in this design'


@pytest.mark.parametrize('case', [S.TailCase('k16_b1', 16, 1, 1, 3), S.TailCase('k32_b3', 32, 3, 1, 3), S.TailCase('hoa_k16_b1', 16, 1, 4, 5)],
                         ids=lambda c: c.name)
def test_tail_packed_partners(T, case):
    c = case
    dmask, spec, coeffs = S.tail_operands(c, 6)
    w = coeffs.copy()
    if c.nin == 1:
        w[:, :, 0, :c.K] = 1e3 * w[:, :, 1, :c.K]
        w[:, :, 2, :c.K] = 0.0
    else:
        w[:, :, 0, :, :c.K] = 1e3 * w[:, :, 1, :, :c.K]
        w[:, :, 2:, :, :c.K] = 0.0
    got = run_tail(T, c, dmask, spec, w)
    _check_tail(c, (dmask, spec, w), got, 'packed partners: output 0 = 1e3 x output 1, output 2 zero')
    n = np.arange(4800)
    exact = np.ones(4800, bool)
    if c.nin > 1:            # spectra (s_lo, 0..4), (s_hi, 0..4) pair up in that order: (s_hi, 2) shares its transform with (s_hi, 1)
        for f in range(S.F_LO, S.F_HI):
            s_lo, s_hi = S.frame_steps(f)
            if s_hi != s_lo:
                exact &= ~((n >= 256 * f - 1216) & (n <= 256 * f - 193) & (n // 1600 == s_hi))
    assert exact.sum() > 2400
    assert np.array_equal(got[:, exact, 2], _bias_of(c, w)[:, exact, 2]), 'a zero spectrum beside nothing, or beside another zero one, is not exactly the bias'


@pytest.mark.parametrize('case', [S.TailCase('k16_b1', 16, 1, 1, 3), S.TailCase('k64_b1', 64, 1, 1, 3), S.TailCase('hoa_k32_b1', 32, 1, 4, 5)],
                         ids=lambda c: c.name)
def test_tail_saturated_logits(T, case):
    c = case
    dmask, spec, coeffs = S.tail_operands(c, 7)
    r = np.random.RandomState(8)
    mixed = r.choice(np.array([88., -88., 100., -100., 1e4, -1e4], np.float32), size=dmask.shape)
    got = run_tail(T, c, mixed, spec, coeffs)
    _check_tail(c, (mixed, spec, coeffs), got, 'logits from +-88, +-100, +-1e4')
    allpass = run_tail(T, c, np.full_like(dmask, 40.0), spec, coeffs)
    for v in (88., 100., 1e4):
        hi = run_tail(T, c, np.full_like(dmask, v), spec, coeffs)
        lo = run_tail(T, c, np.full_like(dmask, -v), spec, coeffs)
        _check_tail(c, (np.full_like(dmask, -v), spec, coeffs), lo, 'all logits %g' % -v, rms_bar=False)
        if not TWIN:         # (the twin's sigmoid is a double: 1 - 6e-39 and 4e-44 are neither 1 nor 0 there)
            assert np.array_equal(hi, allpass), 'sigmoid(%g) is 1 in float32' % v
            if v >= 100.:
                assert np.array_equal(lo, _bias_of(c, coeffs)), 'sigmoid(%g) is 0 in float32' % -v


def test_tail_refusals_leave_the_output_untouched(T):
    c, h = S.TailCase('k16_b1', 16, 1, 1, 3), S.TailCase('hoa_k16_b1', 16, 1, 4, 5)
    ops, hops = S.tail_operands(c), S.tail_operands(h)
    big = np.zeros((1, 28, 1024, 4 * 24), np.float32)          # room for 24 tracks per input channel
    big_w = np.zeros((1, 3, 5, 4, 25), np.float32)
    for out in (run_tail(T, c, big, ops[1], big_w, expect=-1, ntracks=24),
                run_tail(T, c, *ops, expect=-1, short=1),
                run_tail(T, c, *ops, expect=-1, batch=0)):
        assert np.isnan(out).all(), 'a refused call wrote to its output'
    if TWIN:
        return                                                  # the twin has no second-order op
    for out in (run_tail(T, h, big, hops[1], big_w, expect=-1, ntracks=24),
                run_tail(T, h, *hops, expect=-1, short=1),
                run_tail(T, h, *hops, expect=-1, batch=0),
                run_tail(T, h, *hops, expect=-1, nin=3),
                run_tail(T, h, *hops, expect=-1, nout=3),
                run_tail(T, h, *hops, expect=-1, nin=1, nout=3)):
        assert np.isnan(out).all(), 'a refused call wrote to its output'


# ------------------------------------------------------------------------------------------------------------------------
# the elementwise passes
# ------------------------------------------------------------------------------------------------------------------------
def _scales(r, C_):
    sc = r.uniform(0.5, 1.5, size=C_) * r.choice([-1.0, 1.0], size=C_)
    sc[0], sc[C_ - 1] = 0.0, -abs(sc[C_ - 1])
    return sc.astype(np.float32), r.normal(size=C_).astype(np.float32)


def _run_bn_apply(T, x, sc, sf, res):
    lib, L = _lib()
    y, guard = _guarded(T, x.shape)
    dx, dsc, dsf, dres = _dev(T, x), _dev(T, sc), _dev(T, sf), _dev(T, res)             # (held until the call has run)
    L.check(lib.sagen_bn_apply_relu(_ptr(dx), _ptr(dsc), _ptr(dsf), _ptr(dres), _ptr(y), x.shape[0], x.shape[1], _stream(T)))
    _sync(T)
    assert bool(T.isnan(guard).all()), 'written past y'
    return y.cpu().numpy()


def _check_bn_apply(T, name, x, sc, sf, res):
    y = _run_bn_apply(T, x, sc, sf, res)
    want, bound, v = S.bn_apply_relu_ref(x, sc, sf, res)
    assert np.isfinite(y).all(), (name, 'elements not written')
    diff = np.abs(y - want)
    bad = np.argwhere(diff > bound)
    assert bad.size == 0, (name, len(bad), [(tuple(b), float(y[tuple(b)]), float(want[tuple(b)]), float(bound[tuple(b)])) for b in bad[:6]])
    assert not y[v < -bound].any(), (name, 'a result the reference puts below zero is not exactly 0')
    return _frac(diff, bound)


@pytest.mark.parametrize('C_', [4, 12, 20, 64, 100, 512])
def test_bn_apply_relu_sweep(T, C_):
    r = np.random.RandomState(C_)
    worst = 0.0
    for npix in (1, 3, 257):
        x, res = r.normal(size=(npix, C_)).astype(np.float32), r.normal(size=(npix, C_)).astype(np.float32)
        sc, sf = _scales(r, C_)
        for with_scale in (True, False):
            for with_res in (True, False):
                worst = max(worst, _check_bn_apply(T, 'c%d_p%d_scale%d_res%d' % (C_, npix, with_scale, with_res), x, sc if with_scale else None,
                                                   sf if with_scale else None, res if with_res else None))
    _record('bn_apply_relu', 'c%d' % C_, 'pixels 1, 3, 257 x scale x residual', worst)


@pytest.mark.parametrize('C_', [12, 64])
def test_bn_apply_relu_beyond_one_grid_pass(T, C_):
    """More than 4096 x 256 float4: the grid-stride loop takes a second pass, and a thread must meet the same 4 channels there
    (C / 4 = 3 does not divide 4096 x 256: the gcd branch of channel_aligned_grid)."""
    npix = 4096 * 256 // (C_ // 4) + 1027
    assert npix * (C_ // 4) > 4096 * 256
    r = np.random.RandomState(100 + C_)
    x, res = r.normal(size=(npix, C_)).astype(np.float32), r.normal(size=(npix, C_)).astype(np.float32)
    sc, sf = _scales(r, C_)
    _record('bn_apply_relu', 'c%d_p%d' % (C_, npix), 'second grid pass, scale + residual', _check_bn_apply(T, 'big_c%d' % C_, x, sc, sf, res))


def _run_maxpool(T, x, sc, sf):
    lib, L = _lib()
    B, H, W, C_ = x.shape
    y, guard = _guarded(T, (B, (H + 1) // 2, (W + 1) // 2, C_))
    dx, dsc, dsf = _dev(T, x), _dev(T, sc), _dev(T, sf)                                  # (held until the call has run)
    L.check(lib.sagen_maxpool3x3s2(_ptr(dx), _ptr(dsc), _ptr(dsf), _ptr(y), B, H, W, C_, _stream(T)))
    _sync(T)
    assert bool(T.isnan(guard).all()), 'written past y'
    return y.cpu().numpy()


def _check_maxpool(T, x, sc, sf):
    plain = _run_maxpool(T, x, None, None)
    assert np.array_equal(plain, O.max_pool_3x3_s2_same(x)), ('maxpool without scale is not bit for bit the oracle', x.shape)
    y = _run_maxpool(T, x, sc, sf)
    v = O.max_pool_3x3_s2_same(x.astype(np.float64) * sc.astype(np.float64) + sf.astype(np.float64))      # the window's maximum before ReLU
    want, bound = np.maximum(v, 0.0), U * np.abs(v)
    assert np.isfinite(y).all()
    bad = np.argwhere(np.abs(y - want) > bound)
    assert bad.size == 0, (x.shape, len(bad), [(tuple(b), float(y[tuple(b)]), float(want[tuple(b)])) for b in bad[:6]])
    assert not y[v < -bound].any(), 'a window whose maximum is negative is not exactly 0'
    return _frac(np.abs(y - want), bound)


@pytest.mark.parametrize('C_', [4, 12, 64])
def test_maxpool_sweep(T, C_):
    r = np.random.RandomState(200 + C_)
    worst = 0.0
    for H in (1, 2, 3, 8, 9):
        for W in (1, 2, 3, 8, 9):
            x = r.normal(size=(2, H, W, C_)).astype(np.float32)
            worst = max(worst, _check_maxpool(T, x, *_scales(r, C_)))
    _record('maxpool3x3s2', 'c%d' % C_, 'H, W in 1, 2, 3, 8, 9', worst)


def test_maxpool_beyond_one_grid_pass(T):
    r = np.random.RandomState(300)
    x = r.normal(size=(1, 1183, 1183, 12)).astype(np.float32)                    # 592 x 592 x 3 float4 outputs > 4096 x 256
    assert 592 * 592 * 3 > 4096 * 256
    _record('maxpool3x3s2', 'c12_1183x1183', 'second grid pass', _check_maxpool(T, x, *_scales(r, 12)))


@pytest.mark.parametrize('C_', [4, 12, 100, 512])
def test_bn_finalize_sweep(T, C_):
    lib, L = _lib()
    r = np.random.RandomState(400 + C_)
    count, eps = 2 * 7 * 9, 1e-3
    mean, var = r.normal(size=C_) * 3, r.uniform(0.1, 4.0, size=C_)
    mean[0], var[0] = 100.1, 0.0                                                 # the accumulators cancel: the clamp decides
    mean[2], var[2] = -1e3 / 3, 0.0
    acc = np.concatenate([count * mean, count * (var + mean * mean)])
    gamma, beta = r.normal(size=C_).astype(np.float32), r.normal(size=C_).astype(np.float32)
    gamma[1] = 0.0
    pad = 8
    scale, shift = (T.full((C_ + pad,), float('nan'), dtype=T.float32, device='cpu' if TWIN else 'cuda') for _ in range(2))
    dacc, dgamma, dbeta = _dev(T, acc, np.float64), _dev(T, gamma), _dev(T, beta)        # (held until the call has run)
    L.check(lib.sagen_bn_finalize(_ptr(dacc), 2, 7, 9, C_, _ptr(dgamma), _ptr(dbeta), eps, _ptr(scale), _ptr(shift), _stream(T)))
    _sync(T)
    scale, shift = scale.cpu().numpy(), shift.cpu().numpy()
    assert np.isnan(scale[C_:]).all() and np.isnan(shift[C_:]).all(), 'written past scale[C] / shift[C]'
    want_sc, want_sh = S.bn_finalize_ref(acc, count, gamma, beta, eps)
    worst = 0.0
    for got, want, what in ((scale[:C_], want_sc, 'scale'), (shift[:C_], want_sh, 'shift')):
        assert np.isfinite(got).all()
        bound = 4 * U * np.abs(want)
        bad = np.argwhere(np.abs(got - want) > bound)
        assert bad.size == 0, (what, [(int(b), float(got[b]), float(want[b])) for b in bad[:6, 0]])
        worst = max(worst, _frac(np.abs(got - want), bound))
    assert scale[1] == 0.0 and shift[1] == beta[1], 'gamma = 0'
    assert abs(want_sc[0] - gamma[0] / np.sqrt(float(np.float32(eps)))) <= 1e-6 * abs(want_sc[0]), 'the variance of channel 0 is not ~0 in the reference'
    _record('bn_finalize', 'c%d' % C_, 'scale and shift, 4 * 2^-24 relative', worst)


# ------------------------------------------------------------------------------------------------------------------------
# the tail inside the network (audio-only networks): the two-kernel form on the device's own inputs, the fused epilogue on exact logits
# ------------------------------------------------------------------------------------------------------------------------
ENC = ['audio']


def _network(nsep, P):
    from spatialaudiogen_amd.model import SptAudioGen, SptAudioGenParams
    net = SptAudioGen(1, encoders=ENC, separation='unet_mask', params=SptAudioGenParams(sep_num_tracks=nsep))
    net.load_variables(P)
    return net


def _device_spec_and_coeffs(net, B, K):
    spec = net.intermediate(B, 'stft').cpu().numpy().reshape(B, 28, 513, 2)
    return spec, net.intermediate(B, 'localization/coeffs').cpu().numpy().reshape(B, 3, 3, K + 1)


def _check_network_stft(net, B, audio, name):
    c = S.StftCase(name, B, 52799, 46, 173, 89, 117, 'both')
    mag = net.intermediate(B, 'mag').cpu().numpy().reshape(B, 127, 1024)
    spec = net.intermediate(B, 'stft').cpu().numpy().reshape(B, 28, 513, 2)
    _check_stft(c, audio, mag, spec, 'network')


@pytest.mark.parametrize('B', [2, 5])
@pytest.mark.parametrize('nsep', [16, 32, 64])
def test_network_two_kernel_tail_on_the_devices_own_inputs(T, nsep, B):
    """The logits the network's own decoder produced (rows 44..66 of deconv1 = mask frames 1..23), its own STFT and its own
    localisation coefficients, read back and put through tail_ref: the network's output holds the tail's elementwise bound, and
    `mag` / `stft` hold the STFT's bound against the input audio.  nsep 32 needs materialize_mask = 1 to keep the logits."""
    from spatialaudiogen_amd.weights import variable_specs, init_weights, synth_inputs
    P = init_weights(variable_specs(ENC, 'unet_mask', nsep), seed=nsep + B, mode='test')
    audio = synth_inputs(B, ENC, seed=77 + B)['audio']
    net = _network(nsep, P)
    net.inference_ops(audio)
    net.set_option(B, 'materialize_mask', 1)
    out = net.inference_ops(audio).cpu().numpy()
    T.cuda.synchronize()
    dmask = np.zeros((B, 28, 1024, nsep), np.float32)
    dmask[:, 1:24] = net.intermediate(B, 'separation/deconv1').cpu().numpy()
    spec, coeffs = _device_spec_and_coeffs(net, B, nsep)
    name = 'net_k%d_b%d' % (nsep, B)
    _check_tail(S.TailCase(name, nsep, B, 1, 3), (dmask, spec, coeffs), out, 'network, two kernels', rms_bar=False)
    _check_network_stft(net, B, np.asarray(audio, np.float32).reshape(B, 52799), name)
    assert net.counter(B, 'fp16x2_saturations') == 0


@pytest.mark.parametrize('B', [2, 5])
def test_network_fused_tail_on_exact_integer_logits(T, B):
    """nsep 32, default switches: the logits never exist, so they are made KNOWN.  deconv2 has zero weights and integer biases 0..3: the
    decoder half of cat1 (its channels 0..31; the encoder half, conv1's output, lies behind it) is a per-channel integer constant.
    deconv1 has zero weights on the encoder half and integers -2..2 on the decoder half, integer biases: every logit is an exact integer
    that depends on the output row mod 4, the column mod 8 and the borders.  Everything else is random, so the audio encoder and the
    localisation run normally and the coefficients differ by step.  Under materialize_mask = 1 the device's logits equal the fp64
    deconvolution bit for bit; the default (fused) forward then holds the tail's bound, with two more roundings for v_exp_f32 and
    v_rcp_f32, against tail_ref(integer logits, device stft, device coeffs)."""
    import re
    import forward_oracle as FO
    from spatialaudiogen_amd.weights import variable_specs, init_weights, synth_inputs
    K = 32
    P = init_weights(variable_specs(ENC, 'unet_mask', K), seed=9 + B, mode='test')
    r = np.random.RandomState(31 + B)
    b2 = r.randint(0, 4, size=32).astype(np.float32)
    w1 = np.zeros((7, 16, K, 64), np.float32)
    w1[..., :32] = r.randint(-2, 3, size=(7, 16, K, 32))
    b1 = r.randint(-3, 4, size=K).astype(np.float32)
    P['separation/deconv2/weights'] = np.zeros_like(P['separation/deconv2/weights'])
    P['separation/deconv2/biases'] = b2
    assert P['separation/deconv1/weights'].shape == w1.shape
    P['separation/deconv1/weights'], P['separation/deconv1/biases'] = w1, b1
    cat1 = np.zeros((1, 31, 127, 64))
    cat1[..., :32] = b2
    logits = FO.deconv_ref(cat1, w1, (4, 8)) + b1                                  # [1,127,1024,32], exact integers
    assert logits.shape == (1, 127, 1024, K) and np.array_equal(logits, np.round(logits)) and np.abs(logits).max() < 2 ** 20
    assert len(np.unique(logits[0, 44:67])) > 20, 'the logits do not vary'
    audio = synth_inputs(B, ENC, seed=91 + B)['audio']
    net = _network(K, P)
    fused = net.inference_ops(audio).cpu().numpy()
    with pytest.raises(Exception, match='materialize_mask'):
        net.intermediate(B, 'separation/deconv1')                                  # the fused forward wrote sums, not logits
    net.set_option(B, 'materialize_mask', 1)
    two = net.inference_ops(audio).cpu().numpy()
    d1 = net.intermediate(B, 'separation/deconv1').cpu().numpy()
    want = np.broadcast_to(logits[:, 44:67].astype(np.float32), d1.shape)
    bad = np.argwhere(d1 != want)
    assert bad.size == 0, ('the materialised logits are not the exact integers', len(bad), [(tuple(b), float(d1[tuple(b)]), float(want[tuple(b)])) for b in bad[:6]])
    dmask = np.zeros((B, 28, 1024, K), np.float32)
    dmask[:, 1:24] = want
    spec, coeffs = _device_spec_and_coeffs(net, B, K)
    assert np.abs(coeffs[:, 0] - coeffs[:, 1]).max() > 1e-3, 'the coefficients do not differ by step'
    name = 'net_fused_k32_b%d' % B
    _check_tail(S.TailCase(name, K, B, 1, 3), (dmask, spec, coeffs), two, 'network, exact logits, two kernels', rms_bar=False)
    net.set_option(B, 'materialize_mask', 0)
    net.profile_enable(B, True)
    again = net.inference_ops(audio).cpu().numpy()
    rows = net.profile_report(B)
    net.profile_enable(B, False)
    assert np.array_equal(again, fused)
    _check_tail(S.TailCase(name, K, B, 1, 3), (dmask, spec, coeffs), fused, 'network, exact logits, fused epilogue', rms_bar=False, fused=True)
    assert net.counter(B, 'fp16x2_saturations') == 0
    d1_kernels = [k for k, layer, _, _ in rows if layer == 'separation/deconv1']
    assert d1_kernels and all(re.fullmatch(r'conv3g_kernel<.*,true,1>|igemm3_kernel<.*>', k) for k in d1_kernels), d1_kernels
    assert [k for k, layer, _, _ in rows if layer == 'separation/mask-istft-mix'] == ['mask_istft_kernel+ola_mix_kernel'], rows
    with pytest.raises(Exception, match='materialize_mask'):                       # the last forward fused the mask: mask_istft_kernel read the sums
        net.intermediate(B, 'separation/deconv1')
    print('SPECTRAL ' + json.dumps(dict(op='network', case=name, what='deconv1 ran', kernels=d1_kernels)))
