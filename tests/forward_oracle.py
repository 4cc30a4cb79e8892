"""References, case generators and the kernel-selection restatement of the forward op-level sweeps (test_gpu_forward_ops.py; pinned on
the host by test_forward_oracle_host.py).  Plain numpy, fp64, nothing of the product is imported here and torch is not needed.

The three contractions of include/sagen.h,

    conv:    y[b,i,j,o] = sum_{p,q,c} xin[b, i*sh + p - pt, j*sw + q - pl, c] * w[p,q,c,o]      xin = relu(x*scale + shift) or x, ZERO outside
    fc:      y[m,n]     = sum_k x[m,k] * w[k,n]
    deconv:  y[b, i*sh + p, j*sw + q, o] += x[b,i,j,c] * w[p,q,o,c]                               (conv2d_transpose, VALID)

are computed directly (one strided slice and one tensordot per tap), each with its companion sums for the elementwise bound: the
absolute reference sum |xin * w|, the prologue's own sum (|x*scale| + |shift|) * |w|, and the number of contracted terms per output.

Out of scope: the fp16x2 plane families (conv3h, conv3hr, conv3g on fp16 planes, the space-to-depth tiles, stem8, stempool) are not
reachable through the op-level ABI and keep their model-level tests; NOT_AT_OP_LEVEL below names every registry tile no op-level call
launches, NOT_SWEPT the two that a forced call would launch and the sweeps leave out on purpose.
"""
import collections
import os

import numpy as np

from backward_oracle import MAC_CAP, cdiv, same_pad

# ------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------


def conv_geometry(H, W, kh, kw, sh, sw, padding):
    """(Ho, Wo, pt, pb, pl, pr) of tf.nn.convolution: SAME pads the smaller half BEFORE."""
    if padding == 'SAME':
        (Ho, pt), (Wo, pl) = same_pad(H, kh, sh), same_pad(W, kw, sw)
        th, tw = max((Ho - 1) * sh + kh - H, 0), max((Wo - 1) * sw + kw - W, 0)
        return Ho, Wo, pt, th - pt, pl, tw - pl
    assert padding == 'VALID' and H >= kh and W >= kw
    return (H - kh) // sh + 1, (W - kw) // sw + 1, 0, 0, 0, 0


def _correlate(xin, w, stride, padding):
    """fp64 NHWC / HWIO correlation of an already prologued input, zero padded."""
    xin, w = np.asarray(xin, np.float64), np.asarray(w, np.float64)
    (B, H, W, _), (kh, kw, _, cout), (sh, sw) = xin.shape, w.shape, stride
    Ho, Wo, pt, pb, pl, pr = conv_geometry(H, W, kh, kw, sh, sw, padding)
    xp = np.pad(xin, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    y = np.zeros((B, Ho, Wo, cout))
    for p in range(kh):
        for q in range(kw):
            y += np.tensordot(xp[:, p:p + (Ho - 1) * sh + 1:sh, q:q + (Wo - 1) * sw + 1:sw], w[p, q], axes=1)
    return y


def prologue(x, scale=None, shift=None):
    """relu(x*scale + shift) in fp64 (the consumer-side batch-norm of include/sagen.h), applied BEFORE the padding; x itself without one."""
    x = np.asarray(x, np.float64)
    return x if scale is None else np.maximum(x * np.asarray(scale, np.float64) + np.asarray(shift, np.float64), 0.0)


def conv_ref(x, w, stride, padding, scale=None, shift=None):
    """The RAW fp64 output (before bias and ReLU): what bn_stats sums."""
    return _correlate(prologue(x, scale, shift), w, stride, padding)


def conv_abs_ref(x, w, stride, padding, scale=None, shift=None):
    """sum |xin * w| per output."""
    return _correlate(np.abs(prologue(x, scale, shift)), np.abs(np.asarray(w, np.float64)), stride, padding)


def conv_prologue_abs_ref(x, w, stride, padding, scale, shift):
    """sum (|x*scale| + |shift|) * |w| per output: the scale of the prologue's own two fp32 roundings."""
    x = np.asarray(x, np.float64)
    return _correlate(np.abs(x * np.asarray(scale, np.float64)) + np.abs(np.asarray(shift, np.float64)), np.abs(np.asarray(w, np.float64)), stride, padding)


def conv_terms(x_shape, w_shape, stride, padding):
    """The number of contracted terms of every output [1,Ho,Wo,1]: the taps inside the image times Cin."""
    (_, H, W, cin), (kh, kw) = x_shape, w_shape[:2]
    return _correlate(np.ones((1, H, W, 1)), np.ones((kh, kw, 1, 1)), stride, padding) * cin


def deconv_ref(x, w, stride):
    """fp64 tf.nn.conv2d_transpose VALID: x [B,H,W,Cin], w [kh,kw,Cout,Cin] -> [B, (H-1)*sh + kh, (W-1)*sw + kw, Cout]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    (B, H, W, _), (kh, kw, cout, _), (sh, sw) = x.shape, w.shape, stride
    y = np.zeros((B, (H - 1) * sh + kh, (W - 1) * sw + kw, cout))
    for p in range(kh):
        for q in range(kw):
            y[:, p:p + (H - 1) * sh + 1:sh, q:q + (W - 1) * sw + 1:sw] += np.tensordot(x, w[p, q].T, axes=1)
    return y


def deconv_abs_ref(x, w, stride):
    return deconv_ref(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), stride)


def deconv_terms(x_shape, w_shape, stride):
    (_, H, W, cin), (kh, kw) = x_shape, w_shape[:2]
    return deconv_ref(np.ones((1, H, W, 1)), np.ones((kh, kw, 1, 1)), stride) * cin


def fc_ref(x, w):
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64)


def fc_abs_ref(x, w):
    return np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64))


def stats_ref(raw):
    """bn_stats of include/sagen.h: the per-channel sum and sum of squares of the RAW output, [2*cout] fp64."""
    raw = np.asarray(raw, np.float64).reshape(-1, raw.shape[-1])
    return np.concatenate([raw.sum(0), (raw * raw).sum(0)])


def integer_exact(n, x_range=2):
    """n products of an activation of magnitude <= x_range with a weight of magnitude <= 2 (the issue's n * 4 * (prologue range), the
    range being the activation's over the plain operands' 2): every fp32 partial sum, in any order, is an integer below 2^24."""
    return n * 2 * x_range < 2 ** 24


def stats_exact(raw_int):
    """The kernels sum a TILE's rows (at most 256 consecutive output pixels) in fp32 before the fp64 atomics.  Integer statistics are
    bit-exact when every such fp32 partial sum is an integer below 2^24: sufficient is that the squares of ANY 256 consecutive
    pixels of a channel sum to less than 2^24 (the squares bound the magnitudes: |v| <= v^2 for integers)."""
    sq = np.asarray(raw_int, np.float64).reshape(-1, raw_int.shape[-1]) ** 2
    c = np.concatenate([np.zeros((1, sq.shape[1])), np.cumsum(sq, 0)])
    win = c[min(256, len(sq)):] - c[:len(c) - min(256, len(sq))]
    return bool(win.max() < 2 ** 24)


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
ConvCase = collections.namedtuple('ConvCase', 'name B H W cin kh kw cout sh sw padding bias relu prologue stats')
FcCase = collections.namedtuple('FcCase', 'name M K N bias relu')
DeconvCase = collections.namedtuple('DeconvCase', 'name B H W cin kh kw cout sh sw bias relu')
PROLOGUES = ('', 'pos', 'neg', 'posshift')      # none | scales 0.5..1.5 | scales of both signs | every shift positive (a padded border must stay 0)


def conv_out(c):
    return conv_geometry(c.H, c.W, c.kh, c.kw, c.sh, c.sw, c.padding)


def conv_macs(c):
    Ho, Wo = conv_out(c)[:2]
    return float(c.B * Ho * Wo) * c.kh * c.kw * c.cin * c.cout


def conv_supported(c):
    """include/sagen.h: cin a power of two >= 4 (any multiple of 4 for 1x1), 3, or 1 with VALID, kw % 4 == 0, sw % 4 == 0 (a power-of-two kw
    above one filter row); the prologue on a multi-tap conv with cin % 16 == 0, cin <= 512."""
    pow2 = c.cin >= 4 and c.cin & (c.cin - 1) == 0
    if c.padding == 'VALID' and (c.H < c.kh or c.W < c.kw):
        return False
    if c.prologue:
        return pow2 and c.cin % 16 == 0 and c.cin <= 512 and c.kh * c.kw > 1
    if c.cin == 1:
        return c.padding == 'VALID' and c.kw % 4 == 0 and c.sw % 4 == 0 and (c.kh == 1 or c.kw & (c.kw - 1) == 0)
    return c.cin == 3 or pow2 or (c.kh * c.kw == 1 and c.cin % 4 == 0)


def conv_cases():
    C = ConvCase
    cases = [
        # -- tile grid: M and N tails of every BM / BN (default or forced: M > 128 and N >= 64), N % 4 != 0, M <= 32
        C('g_tails_k120', 2, 9, 11, 8, 3, 5, 100, 1, 1, 'SAME', True, True, '', False),           # K = 120: ragged K tail, Cin 8 with 15 taps
        C('g_kpad48', 3, 8, 9, 16, 3, 1, 72, 1, 1, 'SAME', False, False, '', True),               # Kpad = 48: the K32 tiles refuse it
        C('g_n70', 2, 10, 8, 8, 1, 3, 70, 1, 1, 'SAME', True, False, '', True),                   # N % 4 != 0, forceable; K = 24
        C('g_n33_k36', 1, 5, 7, 4, 3, 3, 33, 1, 1, 'SAME', True, False, '', False),               # Cin 4 with 9 taps: K % 16 == 4
        C('g_m6', 1, 4, 5, 32, 3, 3, 40, 1, 1, 'VALID', False, True, '', False),                  # M = 6
        C('g_n20', 2, 7, 6, 16, 2, 2, 20, 1, 2, 'SAME', False, True, '', True),                   # N <= 32: the 128x32 tile with an N tail
        # -- geometry
        C('g_1x1_c12', 2, 9, 9, 12, 1, 1, 20, 2, 2, 'SAME', True, True, '', True),
        C('g_1x1_c36', 3, 7, 7, 36, 1, 1, 64, 1, 1, 'SAME', False, False, '', False),             # forceable; K = 36
        C('g_same_oddpad', 1, 7, 9, 4, 4, 2, 8, 1, 1, 'SAME', False, False, '', True),            # total pad 3 in h, 1 in w
        C('g_same_nopad', 2, 8, 9, 8, 2, 3, 16, 2, 3, 'SAME', True, False, '', False),            # (Ho-1)*sh + kh <= h: SAME pads nothing
        C('g_valid_unread', 1, 10, 12, 16, 3, 2, 24, 4, 3, 'VALID', False, False, '', False),     # rows 7.. and column 11 are never read
        # -- stem (cin 3, padded to 4 channels) and spectrogram (cin 1: the filter row is the channel axis) inputs
        C('stem_7x7_s2', 1, 22, 26, 3, 7, 7, 64, 2, 2, 'SAME', False, False, '', True),           # forceable; Kpad = 208
        C('stem_3x5', 2, 6, 9, 3, 3, 5, 20, 1, 1, 'VALID', True, True, '', False),
        C('spec_7x16', 1, 15, 64, 1, 7, 16, 32, 4, 8, 'VALID', True, True, '', False),
        C('spec_1x12', 2, 5, 40, 1, 1, 12, 12, 1, 4, 'VALID', False, True, '', True),
        # -- the prologue in the fp32-activation kernels (not 3x3 stride 1)
        C('pro_5x3_neg', 2, 9, 10, 16, 5, 3, 40, 2, 1, 'SAME', False, False, 'neg', True),
        C('pro_2x2_posshift', 1, 6, 7, 32, 2, 2, 36, 1, 1, 'SAME', True, True, 'posshift', False),
        C('pro_3x3_s2_pos', 2, 9, 9, 16, 3, 3, 64, 2, 2, 'SAME', True, False, 'pos', True),
        # -- dense 3x3 stride-1 SAME with cin % 16 == 0: the plane path (conv3p) with the full scratch, the shared-tap kernels
        #    (igemm3dw) with a scratch of the pre-planes size
        C('p3_h2', 2, 2, 33, 32, 3, 3, 64, 1, 1, 'SAME', False, False, '', True),                 # forceable (M = 132)
        C('p3_w8', 3, 7, 8, 16, 3, 3, 64, 1, 1, 'SAME', False, False, 'posshift', True),          # forceable (M = 168)
        C('p3_one_row_tile', 1, 3, 131, 16, 3, 3, 32, 1, 1, 'SAME', False, True, 'neg', False),   # a 62-pixel tile inside one image row
        C('p3_many_images', 19, 4, 9, 16, 3, 3, 16, 1, 1, 'SAME', True, False, '', True),         # image-edge and batch-edge gap slots
        C('p3_cin128', 2, 8, 9, 128, 3, 3, 72, 1, 1, 'SAME', True, True, 'pos', True),            # forceable; Cin > 64
        C('p3_n136', 1, 13, 11, 64, 3, 3, 136, 1, 1, 'SAME', False, False, '', True),             # forceable; N tail in every BN
    ]
    # -- random draws: generic geometry, then dense 3x3 stride-1 SAME
    r = np.random.default_rng(20241018)
    i = 0
    while i < 14:
        kh, kw = int(r.choice([1, 2, 3, 5, 7])), int(r.choice([1, 3, 4, 5, 7]))
        sh, sw = int(r.choice([1, 2, 3])), int(r.choice([1, 2, 4]))
        cin = int(r.choice([4, 12, 20, 36, 64])) if kh * kw == 1 else int(r.choice([4, 8, 16, 32, 64]))
        cout = int(r.choice([4, 20, 32, 33, 64, 100, 128]))
        H, W, B = int(r.integers(kh, kh + 12)), int(r.integers(kw, kw + 16)), int(r.integers(1, 5))
        pro = PROLOGUES[i % 4] if cin % 16 == 0 and kh * kw > 1 else ''
        c = C('cv_r%02d' % i, B, H, W, cin, kh, kw, cout, sh, sw, 'SAME' if i % 2 else 'VALID', bool(i & 1), bool(i & 2), pro, bool(i & 4))
        if conv_macs(c) > MAC_CAP / 8:
            continue
        cases.append(c)
        i += 1
    i = 0
    while i < 8:
        H, W, B = int(r.integers(2, 14)), int(r.integers(8, 24)), int(r.integers(1, 5))
        cin, cout = int(r.choice([16, 32, 64, 128])), int(r.choice([8, 24, 32, 48, 64, 96, 136]))
        c = C('cv_d%02d' % i, B, H, W, cin, 3, 3, cout, 1, 1, 'SAME', bool(i & 4), bool(i & 1), PROLOGUES[(i + 1) % 4], bool(i & 2))
        if conv_macs(c) > MAC_CAP / 8:
            continue
        cases.append(c)
        i += 1
    assert len({c.name for c in cases}) == len(cases)
    return cases


def fc_cases():
    F = FcCase
    cases = [
        # -- the direct epilogue: K < 256 (fewer than 16 K tiles), every K % 16
        F('fc_k100', 70, 100, 96, True, True), F('fc_k40_n20', 33, 40, 20, True, False), F('fc_k12_n8', 5, 12, 8, False, True),
        F('fc_k64_n99', 40, 64, 99, True, True),
        # -- ... and at least 384 blocks of the 32x128 tile with 16 K tiles; one block fewer splits K
        F('fc_blocks384', 3, 256, 128 * 383 + 4, True, True), F('fc_blocks383', 3, 256, 128 * 383, True, False),
        # -- split-K: M <= 32 (the 32x128 sizing), M == 1, K % 16 == 4 / 8 / 12, the reducer's scalar form (N % 4 != 0) with 2, 3, 5, 7 partials
        F('fc_m6_k260', 6, 260, 300, True, True), F('fc_k264_n99', 96, 264, 99, True, False), F('fc_k412_n130', 40, 412, 130, False, True),
        F('fc_m1', 1, 1024, 130, True, True), F('fc_n99_sk3', 96, 400, 99, True, True), F('fc_n99_sk5', 96, 640, 99, False, True),
        F('fc_n30_sk7', 33, 912, 30, True, False), F('fc_n1', 17, 256, 1, True, True),
        # -- M > 128 and N >= 64: a forced tile applies
        F('fc_f130_k100', 130, 100, 68, True, True), F('fc_f200_k512', 200, 512, 136, True, False), F('fc_f129_n70', 129, 260, 70, False, False),
    ]
    r = np.random.default_rng(977)
    for i in range(6):
        cases.append(F('fc_r%02d' % i, int(r.integers(1, 160)), 4 * int(r.integers(1, 300)), int(r.integers(1, 200)), bool(i & 1), bool(i & 2)))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def deconv_cases():
    D = DeconvCase
    cases = [
        D('dc_k_eq_s', 2, 3, 5, 8, 2, 2, 12, 2, 2, True, True),                    # no overlap
        D('dc_one_axis', 1, 4, 6, 16, 3, 2, 8, 1, 2, True, False),                 # kernel > stride in h only
        D('dc_k_not_mult', 2, 5, 4, 4, 3, 5, 12, 2, 3, False, True),               # kernel no multiple of the stride; sh*sw*cout = 72
        D('dc_h1', 3, 1, 9, 32, 3, 5, 8, 2, 2, True, True),
        D('dc_w1', 2, 7, 1, 8, 4, 3, 16, 2, 1, False, False),
        D('dc_cout6', 2, 4, 5, 16, 3, 3, 6, 2, 2, True, True),                     # cout % 4 != 0
        D('dc_f200', 2, 9, 9, 8, 3, 3, 16, 2, 2, True, False),                     # forceable: M = 200, N = 64
        D('dc_f182_n120', 1, 12, 13, 4, 5, 4, 20, 3, 2, True, True),               # forceable: M = 182, N = 120, K = 16
    ]
    r = np.random.default_rng(4243)
    for i in range(8):
        sh, sw = int(r.choice([1, 2, 3])), int(r.choice([1, 2, 4]))
        kh, kw = sh + int(r.integers(0, 4)), sw + int(r.integers(0, 5))
        cases.append(D('dc_r%02d' % i, int(r.integers(1, 4)), int(r.integers(1, 9)), int(r.integers(1, 12)), int(r.choice([4, 8, 16, 32, 64])), kh, kw,
                       int(r.choice([4, 6, 12, 32, 40])), sh, sw, bool(i & 1), bool(i & 2)))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def _rng(c, integers):
    return np.random.default_rng(sum(map(ord, c.name)) * 7919 + (1 if integers else 0))


def conv_operands(c, integers=False):
    """(x, w, bias, scale, shift) float32 (None where absent).  Random: N(0,1) activations, weights / sqrt(K); integers: -2..2, scales of
    {-2,-1,1,2}, shifts -2..2 (1..2 for 'posshift'), biases -3..3."""
    r = _rng(c, integers)
    xs, ws = (c.B, c.H, c.W, c.cin), (c.kh, c.kw, c.cin, c.cout)
    if integers:
        x, w = r.integers(-2, 3, size=xs), r.integers(-2, 3, size=ws)
        b = r.integers(-3, 4, size=c.cout) if c.bias else None
        sc = r.choice([-2, -1, 1, 2] if c.prologue == 'neg' else [1, 2], size=c.cin) if c.prologue else None
        sf = (r.integers(1, 3, size=c.cin) if c.prologue == 'posshift' else r.integers(-2, 3, size=c.cin)) if c.prologue else None
    else:
        x, w = r.normal(size=xs), r.normal(size=ws) / np.sqrt(c.kh * c.kw * c.cin)
        b = r.normal(size=c.cout) if c.bias else None
        sc = (r.uniform(0.5, 1.5, size=c.cin) * (r.choice([-1.0, 1.0], size=c.cin) if c.prologue == 'neg' else 1.0)) if c.prologue else None
        sf = (np.abs(r.normal(size=c.cin)) + 0.5 if c.prologue == 'posshift' else r.normal(size=c.cin)) if c.prologue else None
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    return f(x), f(w), f(b), f(sc), f(sf)


CONV_INT_X_RANGE = {'': 2, 'pos': 6, 'neg': 6, 'posshift': 6}      # |relu(x*scale + shift)| <= 2*2 + 2


def fc_operands(c, integers=False):
    r = _rng(c, integers)
    if integers:
        x, w, b = r.integers(-2, 3, size=(c.M, c.K)), r.integers(-2, 3, size=(c.K, c.N)), r.integers(-3, 4, size=c.N)
    else:
        x, w, b = r.normal(size=(c.M, c.K)), r.normal(size=(c.K, c.N)) / np.sqrt(c.K), r.normal(size=c.N)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f(x), f(w), (f(b) if c.bias else None)


def deconv_operands(c, integers=False):
    r = _rng(c, integers)
    xs, ws = (c.B, c.H, c.W, c.cin), (c.kh, c.kw, c.cout, c.cin)
    if integers:
        x, w, b = r.integers(-2, 3, size=xs), r.integers(-2, 3, size=ws), r.integers(-3, 4, size=c.cout)
    else:
        x, w, b = r.normal(size=xs), r.normal(size=ws) / np.sqrt(c.kh * c.kw * c.cin / (c.sh * c.sw)), r.normal(size=c.cout)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f(x), f(w), (f(b) if c.bias else None)


# ------------------------------------------------------------------------------------------------------------------------
# what the library runs: csrc/igemm.hip's igemm_pick_tile / igemm_tile_ok / igemm_auto_splitk and the plane branch of csrc/api.hip's
# sagen_conv2d, restated for the op level.  The sweeps assert it against the library's own answer (sagen_conv2d_kernel_name,
# sagen_fc_kernel_name, sagen_deconv2d_kernel_name), case by case and under every kernel-selection switch.
# ------------------------------------------------------------------------------------------------------------------------
TILE_NAMES = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tile_names_v1.txt')).read().split('\n')
SELECTION_KEYS = ('SAGEN_NO_P3', 'SAGEN_FP32_ONLY', 'SAGEN_FORCE_TILE')
Tile = collections.namedtuple('Tile', 'name family bm bn bk fp16 gathered tail')


def _tile(name):
    family, args = name[:-1].split('<')
    a = args.split(',')
    if family == 'conv3pp_kernel':
        return Tile(name, family, 128, 64, 16, False, False, False)
    fp16 = family in ('conv3h_kernel', 'conv3hr_kernel') or (family == 'conv3g_kernel' and a[5] == 'true')
    return Tile(name, family, int(a[0]), int(a[1]), int(a[5]) if family == 'igemm_kernel' else 16, fp16, family == 'conv3g_kernel', len(a) == 7 and family == 'conv3g_kernel')


TILES = [_tile(n) for n in TILE_NAMES]
OP_LEVEL_FAMILIES = ('igemm_kernel', 'igemm3_kernel', 'igemm3dw_kernel', 'conv3p_kernel')      # what the heuristics reach
FORCED_ONLY_FAMILIES = ('conv3g_kernel',)     # bf16 gathered tiles: sagen_conv2d launches them on its planes when forced (no prologue)


def _t(family, *args):
    name = '%s<%s>' % (family, ','.join(str(a).lower() if isinstance(a, bool) else str(a) for a in args))
    return TILES[TILE_NAMES.index(name)]


# every registry tile no op-level call can launch, with the reason (test_forward_oracle_host.py: exactly the tiles forward_plan never
# returns for any case under any SAGEN_FORCE_TILE)
NOT_AT_OP_LEVEL = {}
for _tl in TILES:
    if _tl.fp16:
        NOT_AT_OP_LEVEL[_tl.name] = 'fp16x2 planes and their filter scales are built by the runtime only (model-level tests)'
    elif _tl.family == 'igemm3s2_kernel':
        NOT_AT_OP_LEVEL[_tl.name] = 'the stem tile contracts the 7x8-tap filter layout only the runtime packs (sagen_conv2d packs 7x7 taps)'
# tiles igemm_tile_ok admits when SAGEN_FORCE_TILE names them on a plane case, which the sweeps deliberately do not run
NOT_SWEPT = {t.name: 'the two-team tiles run when forced onto a dense 3x3 case with planes (no SAGEN_P3PP needed: that switch only offers them to the '
                     "runtime's autotuner); they are an experiment no heuristic picks and stay out of the op-level sweeps on purpose"
             for t in TILES if t.family == 'conv3pp_kernel'}
assert all(t.tail is False or t.name in NOT_AT_OP_LEVEL for t in TILES)        # (the fused decoder tail: fp16x2 conv3g tiles)

Problem = collections.namedtuple('Problem', 'M N K Kpad Cin ntaps w_split pro dw3 np3')


def conv_problem(c):
    Ho, Wo = conv_out(c)[:2]
    if c.cin == 1:
        Cin, ntaps = c.kw, c.kh
    elif c.cin == 3:
        Cin, ntaps = 4, c.kh * c.kw
    else:
        Cin, ntaps = c.cin, c.kh * c.kw
    K = Cin * ntaps
    dw3 = (c.kh == 3 and c.kw == 3 and c.sh == 1 and c.sw == 1 and c.padding == 'SAME' and c.cin % 16 == 0 and c.H >= 2 and c.W >= 8)
    return Problem(c.B * Ho * Wo, c.cout, K, cdiv(K, 16) * 16, Cin, ntaps, True, bool(c.prologue), dw3, c.B * c.H * (c.W + 1))


def fc_problem(c):
    return Problem(c.M, c.N, c.K, cdiv(c.K, 16) * 16, c.K, 1, False, False, False, 0)


def deconv_problem(c):
    Hout, Wout = c.H * c.sh + c.kh - c.sh, c.W * c.sw + c.kw - c.sw
    ntaps = cdiv(c.kh, c.sh) * cdiv(c.kw, c.sw)
    K = ntaps * c.cin
    return Problem(c.B * cdiv(Hout, c.sh) * cdiv(Wout, c.sw), c.sh * c.sw * c.cout, K, cdiv(K, 16) * 16, c.cin, ntaps, True, False, False, 0)


def problem(c):
    return conv_problem(c) if isinstance(c, ConvCase) else fc_problem(c) if isinstance(c, FcCase) else deconv_problem(c)


def _uniform_taps(p, bk):
    return (p.Cin % bk == 0 if p.ntaps > 1 else True) and p.K % bk == 0


def tile_ok(p, t, planes):
    """igemm_tile_ok for an op-level problem; planes: the bf16 activation planes are present (the plane branch of sagen_conv2d)."""
    if p.Kpad % t.bk or t.fp16 or t.tail or t.family == 'igemm3s2_kernel':
        return False
    if t.family != 'igemm_kernel' and not p.w_split:
        return False
    if t.family in ('igemm3dw_kernel', 'conv3p_kernel', 'conv3pp_kernel') and not p.dw3:
        return False
    if t.family in ('conv3p_kernel', 'conv3pp_kernel'):
        return planes
    if t.family == 'conv3g_kernel':
        return planes and not p.pro
    return not (p.pro and not _uniform_taps(p, t.bk))


def force_applies(p):
    return p.M > 128 and p.N >= 64


def pick_tile(p, env, planes=False):
    if 'SAGEN_FORCE_TILE' in env and force_applies(p) and tile_ok(p, TILES[int(env['SAGEN_FORCE_TILE'])], planes):
        return TILES[int(env['SAGEN_FORCE_TILE'])]
    blocks = lambda t: cdiv(p.M, t.bm) * cdiv(p.N, t.bn)
    want = 2 * 256
    if p.w_split and 'SAGEN_FP32_ONLY' not in env:
        if planes and p.dw3:
            n_m = cdiv(p.np3, 128)
            big = n_m >= want if p.N <= 64 else n_m * cdiv(p.N, 64) >= want
            return _t('conv3p_kernel', 128, 64, 64, 32) if big else _t('conv3p_kernel', 64, 64, 32, 32)
        if p.dw3:
            if p.N <= 64:
                return _t('igemm3dw_kernel', 128, 64, 64, 32, False) if blocks(_t('igemm3dw_kernel', 128, 64, 64, 32, False)) >= want else _t('igemm3dw_kernel', 64, 64, 32, 32, True)
            if blocks(_t('igemm3dw_kernel', 128, 128, 64, 64, False)) >= 384:
                return _t('igemm3dw_kernel', 128, 128, 64, 64, False)
            return _t('igemm3dw_kernel', 128, 64, 64, 32, True) if blocks(_t('igemm3dw_kernel', 128, 64, 64, 32, True)) >= 384 else _t('igemm3dw_kernel', 64, 64, 32, 32, True)
        if p.M <= 32:
            return _t('igemm3_kernel', 32, 128, 32, 32, 1)
        if p.N <= 32:
            return _t('igemm3_kernel', 128, 32, 32, 32, 1)
        if p.N <= 64:
            return _t('igemm3_kernel', 128, 64, 64, 32, 1) if blocks(_t('igemm3_kernel', 128, 64, 64, 32, 1)) >= want else _t('igemm3_kernel', 64, 64, 32, 32, 1)
        if blocks(_t('igemm3_kernel', 128, 128, 64, 64, 1)) >= 384:
            return _t('igemm3_kernel', 128, 128, 64, 64, 1)
        return _t('igemm3_kernel', 64, 128, 32, 64, 2) if blocks(_t('igemm3_kernel', 64, 128, 32, 64, 1)) >= want else _t('igemm3_kernel', 64, 64, 32, 32, 2)
    if p.M <= 32:
        return _t('igemm_kernel', 32, 128, 32, 32, 2, 16)
    if p.N <= 32:
        return _t('igemm_kernel', 128, 32, 32, 32, 2, 16)
    if p.N <= 64:
        for t in (_t('igemm_kernel', 256, 64, 64, 64, 3, 16), _t('igemm_kernel', 128, 64, 64, 32, 3, 16)):
            if blocks(t) >= want:
                return t
        return _t('igemm_kernel', 64, 64, 32, 32, 3, 16)
    for t in (_t('igemm_kernel', 128, 128, 64, 64, 3, 16), _t('igemm_kernel', 128, 64, 64, 32, 3, 16)):
        if blocks(t) >= want:
            return t
    return _t('igemm_kernel', 64, 64, 32, 32, 3, 16)


def auto_splitk(p, t):
    bm, bn = (32, 128) if t.name == 'igemm_kernel<32,128,32,32,2,16>' else (64, 64)
    blocks, nk = cdiv(p.M, bm) * cdiv(p.N, bn), p.Kpad // 16
    if blocks >= 384 or nk < 16:
        return 1
    return max(min(cdiv(512, blocks), nk // 8, 64), 1)


Plan = collections.namedtuple('Plan', 'tile splitk planes')
SCRATCHES = ('full', 'pre-planes')


def has_plane_room(c):
    """Does sagen_conv2d_scratch_bytes reserve room for the planes (so the two scratch sizes differ)?"""
    return isinstance(c, ConvCase) and c.kh == 3 and c.kw == 3 and c.cin % 16 == 0 and (c.cin // 16) * c.B * c.H * (c.W + 1) * 96 < 2 ** 31


def forward_plan(c, env=None, scratch='full'):
    """(tile, split-K, whether the plane pre-pass runs) for a case under a kernel selection and one of the two scratch sizes."""
    env, p = env or {}, problem(c)
    if isinstance(c, FcCase):
        t = pick_tile(p, env)
        return Plan(t, auto_splitk(p, t), False)
    if isinstance(c, ConvCase):
        room = scratch == 'full' or not has_plane_room(c)
        if ('SAGEN_NO_P3' not in env and 'SAGEN_FP32_ONLY' not in env and room and c.sh == 1 and c.sw == 1 and c.padding == 'SAME' and
                c.cin % 16 == 0 and p.dw3 and c.cin <= 512 and has_plane_room(c)):
            t = pick_tile(p, env, planes=True)
            if t.family in ('conv3p_kernel', 'conv3pp_kernel', 'conv3g_kernel'):
                return Plan(t, 1, True)
    return Plan(pick_tile(p, env), 1, False)


def plan_string(pl):
    return '%s splitk=%d planes=%d' % (pl.tile.name, pl.splitk, 1 if pl.planes else 0)


def all_cases():
    return conv_cases() + fc_cases() + deconv_cases()


def forceable_tiles():
    """Registry indices of the tiles SAGEN_FORCE_TILE can put onto at least one case (computed from forward_plan alone)."""
    cases = all_cases()
    return [i for i, t in enumerate(TILES)
            if any(force_applies(problem(c)) and forward_plan(c, {'SAGEN_FORCE_TILE': str(i)}, s).tile is t for c in cases for s in SCRATCHES)]


def swept_tiles():
    """... minus the ones left out on purpose (NOT_SWEPT): the ids of the per-tile selection tests."""
    return [i for i in forceable_tiles() if TILES[i].name not in NOT_SWEPT]


def selection_cases(env):
    """The cases a selection changes (some scratch size's plan differs from the default's), cheapest first; for a forced tile the two
    cheapest of each kind (conv, dense 3x3, fc, deconv) the tile admits: a child costs a process start and a few small launches."""
    if 'SAGEN_FORCE_TILE' not in env:
        return [c for c in all_cases() if any(forward_plan(c, env, s) != forward_plan(c, {}, s) for s in SCRATCHES)]
    # (a tile the heuristic already picks for a forceable case "changes" nothing there: it still has to run forced)
    t = TILES[int(env['SAGEN_FORCE_TILE'])]
    changed = [c for c in all_cases() if force_applies(problem(c)) and any(forward_plan(c, env, s).tile is t for s in SCRATCHES)]
    kind = lambda c: 'fc' if isinstance(c, FcCase) else 'deconv' if isinstance(c, DeconvCase) else 'dw3' if problem(c).dw3 else 'conv'
    p = lambda c: problem(c)
    changed.sort(key=lambda c: float(p(c).M) * p(c).N * p(c).K)
    out = []
    for k in ('conv', 'dw3', 'fc', 'deconv'):
        out += [c for c in changed if kind(c) == k][:2]
    return out


# ------------------------------------------------------------------------------------------------------------------------
# directed classes
# ------------------------------------------------------------------------------------------------------------------------
def _reachable_shapes(c):
    """(bm, bn, bk) of every tile that runs the case: by default with either scratch, or forced."""
    out = set()
    for s in SCRATCHES:
        t = forward_plan(c, {}, s).tile
        out.add((t.bm, t.bn, t.bk))
        if force_applies(problem(c)):
            for i, t in enumerate(TILES):
                if t.name not in NOT_SWEPT and forward_plan(c, {'SAGEN_FORCE_TILE': str(i)}, s).tile is t:
                    out.add((t.bm, t.bn, t.bk))
    return out


def forward_classes(c):
    """The directed classes a case belongs to."""
    p, out = problem(c), set()
    shapes = _reachable_shapes(c)
    if isinstance(c, ConvCase):
        Ho, Wo, pt, pb, pl, pr = conv_out(c)
        for bm in (32, 64, 128, 256):
            if p.M % bm and any(s[0] == bm for s in shapes):
                out.add('conv:m-tail-bm%d' % bm)
        for bn in (32, 64, 128, 256):
            if p.N % bn and any(s[1] == bn for s in shapes):
                out.add('conv:n-tail-bn%d' % bn)
        if p.N % 4:
            out.add('conv:n%4')
        if p.M <= 32:
            out.add('conv:m<=32')
        if p.K % 16 and c.cin in (4, 8) and (c.kh * c.kw) % 2:
            out.add('conv:ragged-k')
        if p.Kpad % 32:
            out.add('conv:kpad%32')
            if force_applies(p):
                out.add('conv:kpad%32-forceable')
        if p.Cin < 16 and p.ntaps > 1:
            out.add('conv:taps-not-uniform')
        if c.kh * c.kw == 1 and c.cin % 4 == 0 and c.cin & (c.cin - 1):
            out.add('conv:1x1-cin-not-pow2')
        if c.padding == 'SAME':
            if (pt + pb) % 2 and (pl + pr) % 2:
                out.add('conv:same-odd-pad')
            if pt + pb + pl + pr == 0 and (c.kh > 1 or c.kw > 1):
                out.add('conv:same-no-pad')
            out.add('conv:padded' if pt + pb + pl + pr else 'conv:all-taps-inside')
        else:
            out.add('conv:all-taps-inside')
            if (Ho - 1) * c.sh + c.kh < c.H or (Wo - 1) * c.sw + c.kw < c.W:
                out.add('conv:valid-unread')
        if c.cin == 3:
            out.add('conv:cin3-7x7s2' if (c.kh, c.kw, c.sh, c.sw) == (7, 7, 2, 2) else 'conv:cin3-other')
        if c.cin == 1:
            out.add('conv:cin1-kh>1' if c.kh > 1 else 'conv:cin1-kh1')
        out.add('conv:epi-b%d-r%d-s%d' % (c.bias, c.relu, c.stats))
        if c.prologue == 'neg':
            out.add('conv:prologue-neg')
        if c.prologue == 'posshift' and pt + pb + pl + pr:
            out.add('conv:prologue-posshift-padded')
        if c.prologue and not p.dw3:
            out.add('conv:prologue-in-kernel')
        if forward_plan(c).planes:
            out.add('p3')
            if has_plane_room(c) and not forward_plan(c, {}, 'pre-planes').planes:
                out.add('p3:pre-planes-scratch')
            if c.H == 2:
                out.add('p3:h2')
            if c.W == 8:
                out.add('p3:w8')
            if c.W + 1 > 2 * 62:
                out.add('p3:one-row-tile')
            if c.B >= 16:
                out.add('p3:many-images')
            if c.cin > 64:
                out.add('p3:cin>64')
            if c.prologue:
                out.add('p3:prologue')
    elif isinstance(c, FcCase):
        pl_ = forward_plan(c)
        blocks32 = cdiv(c.M, 32) * cdiv(c.N, 128)
        if c.K < 256:
            out.add('fc:k<256')
        if c.K % 16:
            out.add('fc:k%%16=%d' % (c.K % 16))
            if pl_.splitk > 1:
                out.add('fc:k%16-splitk')
        if c.K >= 256 and pl_.splitk == 1 and (blocks32 if c.M <= 32 else cdiv(c.M, 64) * cdiv(c.N, 64)) >= 384:
            out.add('fc:blocks>=384')
        if c.M <= 32 and pl_.splitk > 1:
            out.add('fc:m<=32-splitk')
        if c.M == 1:
            out.add('fc:m1')
        if c.N % 4:
            out.add('fc:n%4-sk1' if pl_.splitk == 1 else 'fc:n%4-sk2..3' if pl_.splitk <= 3 else 'fc:n%4-sk>=5' if pl_.splitk >= 5 and pl_.splitk % 4 else 'fc:n%4-other')
        if c.N < 32:
            out.add('fc:n<32')
        if force_applies(p):
            out.add('fc:forceable')
    else:
        if c.kh == c.sh and c.kw == c.sw:
            out.add('deconv:k==s')
        if (c.kh > c.sh) != (c.kw > c.sw):
            out.add('deconv:k>s-one-axis')
        if c.kh % c.sh or c.kw % c.sw:
            out.add('deconv:k-not-multiple')
        if all(p.N % bn for bn in (32, 64, 128)):
            out.add('deconv:n-off-tiles')
        if c.H == 1:
            out.add('deconv:h1')
        if c.W == 1:
            out.add('deconv:w1')
        if c.cout % 4:
            out.add('deconv:cout%4')
        if force_applies(p):
            out.add('deconv:forceable')
    return out


FORWARD_REQUIRED_CLASSES = (
    ['conv:m-tail-bm%d' % b for b in (32, 64, 128, 256)] + ['conv:n-tail-bn%d' % b for b in (32, 64, 128, 256)] +
    ['conv:n%4', 'conv:m<=32', 'conv:ragged-k', 'conv:kpad%32', 'conv:kpad%32-forceable', 'conv:taps-not-uniform', 'conv:1x1-cin-not-pow2',
     'conv:same-odd-pad', 'conv:same-no-pad', 'conv:valid-unread', 'conv:all-taps-inside', 'conv:padded', 'conv:cin3-7x7s2', 'conv:cin3-other',
     'conv:cin1-kh>1', 'conv:cin1-kh1'] + ['conv:epi-b%d-r%d-s%d' % (b, r, s) for b in (0, 1) for r in (0, 1) for s in (0, 1)] +
    ['conv:prologue-neg', 'conv:prologue-posshift-padded', 'conv:prologue-in-kernel', 'p3', 'p3:pre-planes-scratch', 'p3:h2', 'p3:w8', 'p3:one-row-tile',
     'p3:many-images', 'p3:cin>64', 'p3:prologue',
     'fc:k<256', 'fc:k%16=4', 'fc:k%16=8', 'fc:k%16=12', 'fc:k%16-splitk', 'fc:blocks>=384', 'fc:m<=32-splitk', 'fc:m1', 'fc:n%4-sk1', 'fc:n%4-sk2..3',
     'fc:n%4-sk>=5', 'fc:n<32', 'fc:forceable',
     'deconv:k==s', 'deconv:k>s-one-axis', 'deconv:k-not-multiple', 'deconv:n-off-tiles', 'deconv:h1', 'deconv:w1', 'deconv:cout%4', 'deconv:forceable'])
