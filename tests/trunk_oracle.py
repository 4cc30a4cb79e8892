"""Layer-local fp64 references and elementwise bounds for the ResNet trunk on fp16x2 planes (test_gpu_trunk_layers.py; proven on the
host by test_trunk_oracle_host.py).  Plain numpy, nothing of the product is imported here and torch is not needed.

LAYER-LOCAL: the reference of a layer is computed in fp64 from the DEVICE'S OWN input of that layer (the fp32 tensor the training
step retains), the weights of the test's variable dict and batch-norm coefficients formed in fp64 from the DEVICE'S OWN (sum, sumsq)
accumulators - an error never travels from one layer's check into the next one's, and the layer that is wrong is the layer that fails.
The conv itself is forward_oracle's (_correlate / conv_geometry / conv_terms / conv_abs_ref: SAME pads the smaller half before).

The elementwise bounds, u = 2^-24.  Every one is derived here; none was fitted to what a kernel returns.

  * fp16x2 contraction (conv3h_kernel, conv3hr_kernel, conv3g_kernel on fp16 planes; csrc/conv3h.hip, csrc/h2_planes.h).  Both operands
    are stored as two fp16 planes of the value times an exact power of two (sa = 1 / a_inv for the activation, sw = 1 / w_inv for the
    filter): hi = rne_f16(v*s), lo = rne_f16(v*s - hi).
      - Representation.  |v*s - hi| <= 2^-11 |v*s| and the second rounding leaves 2^-11 of THAT, unless lo falls below fp16's normal
        range, where the absolute resolution 2^-25 takes over (fp16 subnormals are honoured): with v^ = (hi + lo) / s,
        |v - v^| <= e(v) := max(2^-22 |v|, 2^-25 / s) <= 2^-22 |v| + 2^-25 / s.
      - Products.  x*w is evaluated as xh*wh + xh*wl + xl*wh = x^ w^ - xl*wl.  |xl| <= 2^-11 |x^| (half an ulp of hi), so the dropped
        term is <= 2^-22 |x w| to first order, and |x^ w^ - x w| <= |x| e(w) + |w| e(x) + e(x) e(w).  Summed over the n terms of one output:
            3 * 2^-22 * A + 2^-25 * (a_inv * sum |w| + w_inv * sum |x|)        A = sum |x * w|
        (sum |w| is taken over ALL taps of the output channel, an upper bound of the taps inside the image).  The second-order terms -
        e(x) e(w), the 2^-11 between |x^| and |x| in the dropped term, A of the rounded operands instead of A - are below 2^-9 of this
        sum plus n * 2^-49 * a_inv * w_inv: the sum is multiplied by (1 + 2^-9) and that constant is added.
      - Accumulation.  Each of the three fp16 x fp16 products is exact in fp32 (11 + 11 significant bits); 3n of them are summed in fp32 in
        some order and grouping: at most 3n roundings of a partial sum that never exceeds A to first order.  Zero-padded K tiles add exact
        zeros, the epilogue's scale 2^-(ka + kw) is exact; the + 8 is the one the forward sweeps (test_gpu_forward_ops.py) carry for
        them and for a split-K reducer (the dh-split sums three partials of n / 3 terms: n / 3 + 2 <= n + 8):  (3n + 8) * u * A.
    a_inv is read from the device ("t:h2a"); w_inv is recomputed by the rule of h2_filter_pack: the power of two that puts max |w| of the
    layer into [512, 1024).
  * bf16x3 planes (SAGEN_NO_H2=1) and fp32 operands (SAGEN_FP32_ONLY=1): the bound of the forward sweeps, (n + 8) * u * A, unchanged.
  * A prologue relu(fmaf(y, sc, sh)) with sc, sh rounded to fp32 from the fp64 coefficients: the rounding of sc moves the value by at most
    u |y sc|, that of sh by u |sh|, the fused multiply-add rounds once more (u |y sc + sh|), ReLU is 1-Lipschitz:
    <= 2u (|y sc| + |sh|) =: 2u a_pro per element, and through a conv 2u * A_pro, A_pro = sum (|y sc| + |sh|) |w| - the 2 * A_pro of the
    forward sweeps.  The device forms the coefficients from its accumulators in fp64 exactly as bn_coeffs does; two fp64 evaluations
    of the same expression differ by a few 2^-53, amplified by the cancellation in E[y^2] - E[y]^2: 2^-40 (|y sc| + |sh|) is added, which
    covers E[y^2] / var up to 2^10.
  * The merge relu(fmaf(y2, sc, sh) + res): the prologue's three roundings and the addition's own, each at most u times a partial
    result below |y2 sc| + |sh| + |res|: 4u (|y2 sc| + |sh| + |res|) (+ the 2^-40 term).  In a projection block res is the raw output
    of the 1x1 stride-2 projection, which is not retained: its fp64 reference takes its place and its conv bound is added.
  * The pool maxpool3x3s2(relu(bn0(y0))): max is 1-Lipschitz, so an output is off by at most the largest prologue bound in its window.
    (The fused stem pools the RAW output - max, or min where gamma < 0 - and normalises afterwards: the rounded prologue is monotone
    per channel, so that is the same fp32 value, bit for bit.)
  * The stem.  Float frames: (n + 8) * u * A on the float32 frames, n = 147 (at the border an upper bound).  uint8 frames (csrc/stem8.hip) are contracted as
    conv(W, u') / 255 + (0.5 / 255) sum W with u' = u - 128 exact and u' = -0.5 in the padding: EVERY tap contributes, and so does the sum
    of the filter: n = 2 * 147 + 2 (the conv's terms, the filter sum's, the scale and the final addition) and
    A8 = sum (|u'| + 0.5) |w| / 255 over all 147 taps.
  * Batch-norm accumulators against the fp64 sums of the device's own raw output y: the kernels add one tile's rows (at most 256, plus
    the 8 levels of the cross-lane reduction) in fp32 before the fp64 atomics: |d sum| <= 264 u sum |y|, and with one more rounding for each
    square |d sumsq| <= 265 u sum y^2 (the tile-row argument of test_gpu_forward_ops._check_random_stats with b = 0).  Against a REFERENCE
    output with elementwise bound b (the projection, whose output is not retained) the full form of that function applies.

The two assertions the GPU test makes per layer are `elementwise` (finite everywhere and inside the bound) and the layer-local relative
RMS error below RMS_BAR = 2e-5 (the project's op-level bar, TOL of test_gpu_ops.py); check_layer evaluates both.

emulate_h2_conv is the arithmetic of conv3h_kernel on the CPU (planes with a closing zero pixel per image row, three fp16 products per
term, float32 accumulation in K blocks of 16) with switches that plant the faults test_trunk_oracle_host.py must see caught.
"""
import numpy as np

import forward_oracle as FO

U = 2.0 ** -24
RMS_BAR = 2e-5
BN_EPS = 1e-3
STAGES = [(56, 112, 64), (28, 56, 128), (14, 28, 256), (7, 14, 512)]      # (H, W, C) of the block outputs of stage 2 .. 5
FAULTS = ('tap', 'no_lo', 'chunk_xlwh', 'closing_pixel', 'm_tail')
FAULT_TEXT = {'tap': '(a) one tap dropped at one border pixel', 'no_lo': '(b) the activation lo plane dropped',
              'chunk_xlwh': '(c) xl*wh dropped in one 16-channel chunk', 'closing_pixel': "(d) a row's closing zero pixel = the next row's first pixel",
              'm_tail': '(e) the last 37 rows of M left NaN'}
M_TAIL = 37


# ------------------------------------------------------------------------------------------------------------------------
# planes
# ------------------------------------------------------------------------------------------------------------------------
def plane_halfs(B, H, W, C):
    """fp16 elements of the planes [C/16][B*H*(W+1)][2][16]."""
    return (C // 16) * B * H * (W + 1) * 32


def split_planes(v32, sa):
    """p3h_store of csrc/h2_planes.h: hi = float16(v*sa), lo = float16(float32(v*sa) - hi), both casts round to nearest even; sa is a power
    of two, so v*sa is exact.  (The clamp at +-65000 is not restated: the test asserts max |v| * sa <= 65000 beside it.)"""
    sv = np.asarray(v32, np.float32) * np.float32(sa)
    with np.errstate(over='ignore'):
        hi = sv.astype(np.float16)
        lo = (sv - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def encode_planes(hi, lo):
    """[B,H,W,C] hi and lo -> the flat fp16 buffer, every image row closed by a zero pixel."""
    B, H, W, C = hi.shape
    buf = np.zeros((C // 16, B, H, W + 1, 2, 16), np.float16)
    for p, a in enumerate((hi, lo)):
        buf[:, :, :, :W, p, :] = np.asarray(a, np.float16).reshape(B, H, W, C // 16, 16).transpose(3, 0, 1, 2, 4)
    return buf.reshape(-1)


def decode_planes(buf, B, H, W, C):
    """(hi, lo, closing): hi and lo as fp16 [B,H,W,C]; closing [C/16,B,H,2,16] = the pixel behind every image row, both planes."""
    a = np.asarray(buf).reshape(-1)
    a = (a if a.dtype == np.float16 else a.view(np.float16))[:plane_halfs(B, H, W, C)].reshape(C // 16, B, H, W + 1, 2, 16)
    nhwc = lambda p: np.ascontiguousarray(a[:, :, :, :W, p, :].transpose(1, 2, 3, 0, 4)).reshape(B, H, W, C)
    return nhwc(0), nhwc(1), a[:, :, :, W]


def filter_inv_scale(w):
    """2^-kw of h2_filter_pack: max |w| * 2^kw in [512, 1024)."""
    m = float(np.abs(np.asarray(w, np.float32)).max())
    return 1.0 if m == 0.0 or not np.isfinite(m) else 2.0 ** -(9 - int(np.floor(np.log2(m))))


# ------------------------------------------------------------------------------------------------------------------------
# batch-norm from the accumulators; the scale rule of DESIGN.md 3.2 (csrc/p3.hip: p3_tables)
# ------------------------------------------------------------------------------------------------------------------------
def bn_coeffs(acc, C, count, gamma, beta):
    """(scale, shift, var) in fp64 from a layer's accumulators (sum [C], then sumsq [C]): training-mode batch-norm, biased variance."""
    acc = np.asarray(acc, np.float64)
    mean = acc[:C] / count
    var = np.maximum(acc[C:2 * C] / count - mean * mean, 0.0)
    a = np.asarray(gamma, np.float64) / np.sqrt(var + BN_EPS)
    return a, np.asarray(beta, np.float64) - mean * a, var


def bn_range(var, count, gamma, beta):
    """(statistical, rigorous) bound of bn(y): max_c |beta_c| + 8 std_c and max_c |beta_c| + sqrt(N) std_c, std_c = |gamma_c| sqrt(var_c / (var_c + eps))."""
    gs = np.abs(np.asarray(gamma, np.float64)) * np.sqrt(var / (var + BN_EPS))
    b = np.abs(np.asarray(beta, np.float64))
    return float((b + 8.0 * gs).max()), float((b + np.sqrt(count) * gs).max())


def acc_range(acc, C, count):
    """The same pair for a raw tensor known by its accumulators (the projection's output): |mean_c| + 8 (sqrt(N)) std_c."""
    acc = np.asarray(acc, np.float64)
    mean = acc[:C] / count
    sd = np.sqrt(np.maximum(acc[C:2 * C] / count - mean * mean, 0.0))
    return float((np.abs(mean) + 8.0 * sd).max()), float((np.abs(mean) + np.sqrt(count) * sd).max())


def rule_a_inv(stat, rig):
    """2^-ka of the rule: the statistical bound scaled into [512, 1024), capped so that the rigorous bound stays <= 64000."""
    if not (stat > 0 and np.isfinite(stat)):
        return 1.0
    k = 9 - int(np.floor(np.log2(stat)))
    if rig > 0 and np.isfinite(rig):
        k = min(k, int(np.floor(np.log2(64000.0 / rig))))
    return 2.0 ** -max(-60, min(60, k))


def is_pow2(v):
    m, _ = np.frexp(float(v))
    return v > 0 and np.isfinite(v) and m == 0.5


# ------------------------------------------------------------------------------------------------------------------------
# references and bounds
# ------------------------------------------------------------------------------------------------------------------------
def conv_layer(x, w, stride, mode, a_inv=None, pro=None):
    """(ref, bound) of a raw SAME conv output.  x: the device's fp32 input [B,H,W,Cin] - with pro = (scale, shift) the RAW tensor the
    prologue relu(x*scale + shift) is applied to; mode: 'h2' (fp16x2 planes under a_inv) | 'sweep' (bf16x3 planes / fp32 operands)."""
    geo = ((stride, stride), 'SAME')
    sc, sh = pro if pro is not None else (None, None)
    ref = FO.conv_ref(x, w, *geo, sc, sh)
    A = FO.conv_abs_ref(x, w, *geo, sc, sh)
    n = FO.conv_terms(np.shape(x), np.shape(w), *geo)
    if mode == 'h2':
        w_inv = filter_inv_scale(w)
        absw = np.abs(np.asarray(w, np.float64))
        sum_x = FO._correlate(np.abs(FO.prologue(x, sc, sh)), np.ones(absw.shape[:3] + (1,)), *geo)
        planes = 3.0 * 2.0 ** -22 * A + 2.0 ** -25 * (a_inv * absw.sum((0, 1, 2)) + w_inv * sum_x)
        bound = (3 * n + 8) * U * A + planes * (1 + 2.0 ** -9) + n * 2.0 ** -49 * a_inv * w_inv
    else:
        assert mode == 'sweep'
        bound = (n + 8) * U * A
    if pro is not None:
        A_pro = FO.conv_prologue_abs_ref(x, w, *geo, sc, sh)
        bound = bound + (2 * U + 2.0 ** -40) * A_pro
    return ref, bound


def prologue_layer(y, sc, sh):
    """(ref, bound) of relu(fmaf(y, sc, sh))."""
    y = np.asarray(y, np.float64)
    return np.maximum(y * sc + sh, 0.0), (2 * U + 2.0 ** -40) * (np.abs(y * sc) + np.abs(sh))


def merge_layer(y2, sc, sh, res, res_bound=0.0):
    """(ref, bound) of relu(fmaf(y2, sc, sh) + res); res_bound: the elementwise bound of a residual that is itself a reference."""
    y2, res = np.asarray(y2, np.float64), np.asarray(res, np.float64)
    return np.maximum(y2 * sc + sh + res, 0.0), (4 * U + 2.0 ** -40) * (np.abs(y2 * sc) + np.abs(sh) + np.abs(res)) + res_bound


def _pool(v, fill, red):
    """3x3 stride-2 SAME window reduction of [B,H,W,C] (even H, W: one pad row / column AFTER)."""
    B, H, W, C = v.shape
    Ho, Wo, pt, pb, pl, pr = FO.conv_geometry(H, W, 3, 3, 2, 2, 'SAME')
    vp = np.pad(v, ((0, 0), (pt, pb), (pl, pr), (0, 0)), constant_values=fill)
    out = None
    for p in range(3):
        for q in range(3):
            s = vp[:, p:p + (Ho - 1) * 2 + 1:2, q:q + (Wo - 1) * 2 + 1:2]
            out = s if out is None else red(out, s)
    return out


def pool_layer(y0, sc, sh):
    """(ref, bound) of maxpool3x3s2(relu(bn0(y0)))."""
    r, b = prologue_layer(y0, sc, sh)
    return _pool(r, -np.inf, np.maximum), _pool(b, 0.0, np.maximum)


def stem_correlate(x, w):
    """forward_oracle._correlate of the 7x7 stride-2 SAME stem over an even-sized [B,H,W,3] image, fed in space-to-depth form: the image padded
    as SAME pads it (2 before, 3 after) and by one more zero row / column, its four phases stacked as 12 channels, against the filter
    padded with a zero 8th row / column and rearranged alike - a 4x4 stride-1 VALID conv over K = 12 instead of 49 taps over K = 3 (the
    same products, a third of the passes over the output; test_trunk_oracle_host.py holds it against the direct form)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    (B, H, W, C), cout = x.shape, w.shape[-1]
    assert w.shape[:2] == (7, 7) and H % 2 == 0 and W % 2 == 0
    xp = np.pad(x, ((0, 0), (2, 4), (2, 4), (0, 0)))
    x2 = xp.reshape(B, H // 2 + 3, 2, W // 2 + 3, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H // 2 + 3, W // 2 + 3, 4 * C)
    w2 = np.pad(w, ((0, 1), (0, 1), (0, 0), (0, 0))).reshape(4, 2, 4, 2, C, cout).transpose(0, 2, 1, 3, 4, 5).reshape(4, 4, 4 * C, cout)
    return FO._correlate(x2, w2, (1, 1), 'VALID')


def stem_layer(frames, w, u8):
    """(ref, bound) of the raw 7x7 stride-2 SAME stem.  frames [B,224,448,3]: float32, or the uint8 the stem8 kernels contract (x = u / 255 - 0.5)."""
    absw = np.abs(np.asarray(w, np.float64))
    if not u8:         # (n = 147 everywhere: an upper bound of the taps inside the image at the border)
        x = np.asarray(frames, np.float32)
        return stem_correlate(x, w), (147 + 8) * U * stem_correlate(np.abs(x), absw)
    up = np.asarray(frames, np.float64) - 128.0
    # sum (|u'| + 0.5) |w| / 255 over ALL taps: |u'| - 0.5 vanishes in the padding (|u'| = 0.5 there), the rest is the filter's own sum
    A8 = (stem_correlate(np.abs(up) - 0.5, absw) + absw.sum((0, 1, 2))) / 255.0
    return stem_correlate((up + 0.5) / 255.0, w), (2 * 147 + 2 + 8) * U * A8


def stats_check(acc, C, y, b=None):
    """Worst fraction of the accumulator bound: device (sum [C], sumsq [C]) against the fp64 sums of y [...,C] (its own raw output, b = None,
    or a reference with elementwise bound b)."""
    acc = np.asarray(acc, np.float64)
    v = np.abs(np.asarray(y, np.float64)).reshape(-1, C)
    b = np.zeros_like(v) if b is None else np.broadcast_to(b, np.shape(y)).reshape(-1, C)
    yy = np.asarray(y, np.float64).reshape(-1, C)
    d1, d2 = np.abs(acc[:C] - yy.sum(0)), np.abs(acc[C:2 * C] - (yy * yy).sum(0))
    t1, t2 = b.sum(0) + 264 * U * (v + b).sum(0), (2 * v * b + b * b).sum(0) + 265 * U * ((v + b) ** 2).sum(0)
    ok = np.isfinite(acc[:C]).all() and np.isfinite(acc[C:2 * C]).all()
    return float(max((d1 / np.maximum(t1, 1e-300)).max(), (d2 / np.maximum(t2, 1e-300)).max())) if ok else float('inf')


def check_layer(got, ref, bound):
    """The two assertions of the GPU test on one layer: {'finite', 'elementwise' (finite and inside the bound everywhere), 'rms'
    (rel-RMS < RMS_BAR), 'rel_rms', 'worst' (largest fraction of the bound), 'at' (its index)}."""
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    finite = bool(np.isfinite(got).all())
    diff = np.abs(np.where(np.isfinite(got), got, 0.0) - ref)
    bound = np.broadcast_to(bound, diff.shape)
    frac = np.where(bound > 0, diff / np.maximum(bound, 1e-300), np.where(diff > 0, np.inf, 0.0))
    at = tuple(int(k) for k in np.unravel_index(int(np.argmax(frac)), frac.shape))
    rel = float(np.sqrt(np.mean(diff ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-300)) if finite else float('inf')
    return {'finite': finite, 'elementwise': finite and bool((diff <= bound).all()), 'rms': rel < RMS_BAR, 'rel_rms': rel,
            'worst': float(frac[at]), 'at': at}


# ------------------------------------------------------------------------------------------------------------------------
# conv3h_kernel's arithmetic on the CPU, with planted faults
# ------------------------------------------------------------------------------------------------------------------------
def emulate_h2_conv(x32, w32, sa, sw, block=16, fault=None):
    """The dense 3x3 stride-1 SAME conv of x32 [B,H,W,Cin] with w32 [3,3,Cin,Cout] as conv3h_kernel computes it: both operands as fp16
    (hi, lo) planes of the value times sa / sw; the activation planes in the device's layout - flat pixels [B*H*(W+1)], every image row
    closed by one zero pixel that serves as the right-hand padding of its row and the left-hand padding of the next; per term the three
    products xh*wh + xh*wl + xl*wh, exact in float32; float32 accumulation in K blocks of `block` channels; the exact scale 1 / (sa*sw)
    at the end.  fault: None or one of FAULTS."""
    assert fault is None or fault in FAULTS
    x32 = np.asarray(x32, np.float32)
    B, H, W, Cin = x32.shape
    Cout = w32.shape[-1]
    xh, xl = (a.astype(np.float32) for a in split_planes(x32, sa))
    wh, wl = (a.astype(np.float32) for a in split_planes(w32, sw))
    Wp = W + 1
    flat = []
    for a in (xh, xl):
        p = np.zeros((B, H, Wp, Cin), np.float32)
        p[:, :, :W] = a
        if fault == 'closing_pixel':                     # row 1 of image 0 is closed by the first pixel of row 2
            p[0, 1, W] = p[0, 2, 0]
        flat.append(np.concatenate([np.zeros((Wp + 1, Cin), np.float32), p.reshape(-1, Cin), np.zeros((Wp + 1, Cin), np.float32)]))
    if fault == 'no_lo':
        flat[1][:] = 0.0
    bb, hh, ww = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing='ij')
    pix = ((bb * H + hh) * Wp + ww).reshape(-1) + Wp + 1                 # flat index of every output pixel (behind the leading guard)
    hh = hh.reshape(-1)
    m_drop = (H - 1) * W + (W - 1)                                        # image 0, last row, last column: its left-hand tap goes
    acc = np.zeros((B * H * W, Cout), np.float32)
    for dh in (-1, 0, 1):
        inside = ((hh + dh >= 0) & (hh + dh < H)).astype(np.float32)[:, None]          # rows above / below the image read as zero
        for c0 in range(0, Cin, block):
            cs = slice(c0, c0 + block)
            for dw in (-1, 0, 1):
                src = pix + dh * Wp + dw
                ah, al = flat[0][src, cs] * inside, flat[1][src, cs] * inside
                if fault == 'tap' and (dh, dw) == (0, -1):
                    ah[m_drop] = 0.0
                    al[m_drop] = 0.0
                bh, bl = wh[dh + 1, dw + 1, cs], wl[dh + 1, dw + 1, cs]
                acc += ah @ bh
                acc += ah @ bl
                if not (fault == 'chunk_xlwh' and c0 == block):
                    acc += al @ bh
    y = acc * np.float32(1.0 / (float(sa) * float(sw)))
    if fault == 'm_tail':
        y[-M_TAIL:] = np.nan
    return y.reshape(B, H, W, Cout)
