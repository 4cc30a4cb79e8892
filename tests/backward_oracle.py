"""References and case generators of the backward op-level sweeps (test_gpu_backward_ops.py; pinned on the host by
test_backward_oracle_host.py).  Plain numpy / torch-CPU, fp64, nothing of the product is imported here.

The weight gradient of include/sagen.h in one form,

    dw[th,tw,g,d] = sum_{b,i,j} G[b, i*sh + th + h0, j*sw + tw + w0, g] * D[b,i,j,d]        (G zero outside its extent),

is computed directly (one strided slice and one einsum per tap): no autograd, so origins and extents no convolution has are covered.
"""
import collections

import numpy as np

# ------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------


def _tap_slices(n_g, n_d, s, off):
    """Positions i in [0, n_d) with 0 <= i*s + off < n_g as (slice over D, slice over G), or None when there are none."""
    lo = max(0, -(off // s)) if off < 0 else 0            # smallest i with i*s + off >= 0
    hi = min(n_d, (n_g - 1 - off) // s + 1) if n_g - 1 - off >= 0 else 0
    if hi <= lo:
        return None
    return slice(lo, hi), slice(lo * s + off, (hi - 1) * s + off + 1, s)


def wgrad_ref(G, D, kh, kw, stride=(1, 1), origin=(0, 0)):
    """fp64 dw [kh,kw,Cg,Cd] of the formula above.  G [B,HG,WG,Cg], D [B,Hd,Wd,Cd]."""
    G, D = np.asarray(G, np.float64), np.asarray(D, np.float64)
    assert G.ndim == 4 and D.ndim == 4 and G.shape[0] == D.shape[0]
    (sh, sw), (h0, w0) = stride, origin
    dw = np.zeros((kh, kw, G.shape[3], D.shape[3]))
    for th in range(kh):
        rows = _tap_slices(G.shape[1], D.shape[1], sh, th + h0)
        for tw in range(kw):
            cols = _tap_slices(G.shape[2], D.shape[2], sw, tw + w0)
            if rows is None or cols is None:
                continue
            dw[th, tw] = np.einsum('bijg,bijd->gd', G[:, rows[1], cols[1]], D[:, rows[0], cols[0]], optimize=True)
    return dw


def wgrad_abs_ref(G, D, kh, kw, stride=(1, 1), origin=(0, 0)):
    """The same sum over |G| * |D|: the scale of the elementwise rounding bound."""
    return wgrad_ref(np.abs(np.asarray(G, np.float64)), np.abs(np.asarray(D, np.float64)), kh, kw, stride, origin)


def dgrad_ref(x_shape, w, stride, padding, dy):
    """fp64 autograd of tf.nn.convolution (oracle/torch_ref.conv2d_tf) with respect to its input: dx NHWC."""
    import torch
    from oracle.torch_ref import conv2d_tf
    x = torch.zeros(*x_shape, dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
    y = conv2d_tf(x, torch.as_tensor(np.asarray(w), dtype=torch.float64), tuple(stride), padding)
    assert tuple(y.shape[2:]) == tuple(np.asarray(dy).shape[1:3]), (tuple(y.shape), np.asarray(dy).shape)
    y.backward(torch.as_tensor(np.asarray(dy), dtype=torch.float64).permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1).contiguous().numpy()


def same_pad(n, k, s):
    """(output size, pad before) of TF SAME."""
    out = -(-n // s)
    return out, max((out - 1) * s + k - n, 0) // 2


# ------------------------------------------------------------------------------------------------------------------------
# sagen_wgrad cases
# ------------------------------------------------------------------------------------------------------------------------
WgradCase = collections.namedtuple('WgradCase', 'name B HG WG Cg Hd Wd Cd kh kw sh sw h0 w0 scaled form')

MAC_CAP = 1.5e8           # kh*kw*B*Hd*Wd*Cg*Cd of one case: keeps the three fp64 references of a case well below a second


def _macs(c):
    return float(c.kh * c.kw) * c.B * c.Hd * c.Wd * c.Cg * c.Cd


def _conv_case(name, B, H, W, Cg, Cd, kh, kw, sh, sw, padding, scaled=False):
    if padding == 'SAME':
        (Ho, pt), (Wo, pl) = same_pad(H, kh, sh), same_pad(W, kw, sw)
    else:
        Ho, Wo, pt, pl = (H - kh) // sh + 1, (W - kw) // sw + 1, 0, 0
    assert Ho >= 1 and Wo >= 1, name
    return WgradCase(name, B, H, W, Cg, Ho, Wo, Cd, kh, kw, sh, sw, -pt, -pl, scaled, 'conv-' + padding)


def _row_case(name, B, Hd, Wd, Cg, Cd, kh, sh, h0, HG=None, scaled=False):
    """A call the filter-row kernel admits: 3 taps wide, horizontal stride 1, one pad column either side (w0 = -1, WG = Wd >= 12)."""
    HG = HG if HG is not None else (Hd - 1) * sh + kh + h0 + (1 if h0 < 0 else 0)
    return WgradCase(name, B, max(HG, 1), Wd, Cg, Hd, Wd, Cd, kh, 3, sh, 1, h0, -1, scaled, 'free')


def _deconv_case(name, B, H, W, Cin, Cout, kh, kw, sh, sw, scaled=False):
    """conv2d_transpose: G = dy on the fine grid [(H-1)*sh + kh, (W-1)*sw + kw], D = x on the coarse one, origin 0."""
    return WgradCase(name, B, (H - 1) * sh + kh, (W - 1) * sw + kw, Cout, H, W, Cin, kh, kw, sh, sw, 0, 0, scaled, 'deconv')


def _fc_case(name, M, K, N, scaled=False):
    return WgradCase(name, M, 1, 1, K, 1, 1, N, 1, 1, 1, 1, 0, 0, scaled, 'fc')


def wgrad_cases():
    cases = []
    # -- the filter-row kernel's admission rule: every TH of {1,3,5,7} with every vertical stride of {1,2,3}; Wd down to 12, Hd 1 and 2,
    #    padded grids B*Hd*(Wd+1) off the multiples of 16, both of its tiles, Cd tails inside its 64-wide tile
    geo = [(2, 5, 12), (1, 1, 12), (3, 2, 13), (1, 7, 14), (2, 3, 17), (1, 4, 20), (5, 1, 15), (1, 2, 29), (2, 6, 12), (1, 9, 13), (3, 3, 21), (1, 5, 31)]
    chan = [(64, 64), (128, 100), (36, 20), (136, 32), (16, 96), (8, 132), (64, 256), (20, 8), (128, 128), (12, 4), (32, 64), (4, 100)]
    k = 0
    for th in (1, 3, 5, 7):
        for sh in (1, 2, 3):
            (B, Hd, Wd), (Cg, Cd) = geo[k], chan[k]
            h0 = [-(th // 2), 0, -(th - 1), 1][k % 4] if th > 1 else [0, -1, 2][k % 3]
            cases.append(_row_case('row-th%d-sh%d' % (th, sh), B, Hd, Wd, Cg, Cd, th, sh, h0, scaled=(k % 3 == 1)))
            k += 1
    # -- one-row images, several of them, narrower than a chunk: a 16-pixel chunk then crosses two row ends AND two image ends
    cases += [_row_case('row-hd1-b6-wd12', 6, 1, 12, 64, 64, 3, 1, -1, HG=1), _row_case('row-hd1-b5-wd13', 5, 1, 13, 136, 20, 1, 2, 0, HG=1)]
    # -- the fold: Cg 16 / 32 gathered channels, a column of TH filter rows in tiles of 8 / 4, every ragged TH
    k = 0
    for Cg in (16, 32):
        for th in (2, 3, 4, 6, 9, 10):
            sh = [1, 2, 3, 4][k % 4]
            Cd = [64, 96, 20, 128, 32, 100, 8, 256, 64, 4, 132, 32][k]
            B, H, W = 1 + k % 3, th + 3 + 2 * (k % 5), [9, 5, 14, 3, 21, 7][k % 6]
            cases.append(_conv_case('fold-cg%d-th%d' % (Cg, th), B, H, W, Cg, Cd, th, 1, sh, 1 + k % 2, 'SAME' if k % 2 else 'VALID', scaled=(k % 3 == 2)))
            k += 1
    # -- the four BM x BN tiles of the per-tap kernels, channel tails inside a 64-wide and inside a 128-wide tile
    cases += [
        _conv_case('tile-64x64-tails', 2, 9, 11, 36, 20, 3, 5, 1, 1, 'SAME'),
        _conv_case('tile-64x128-tail', 3, 8, 7, 64, 100, 2, 4, 2, 1, 'VALID', scaled=True),
        _conv_case('tile-128x64-tail', 2, 7, 10, 136, 32, 3, 1, 1, 2, 'SAME'),
        _conv_case('tile-128x128-tails', 1, 11, 9, 136, 132, 5, 3, 2, 2, 'SAME'),
        _conv_case('tile-128x128-full', 2, 6, 13, 128, 256, 1, 4, 1, 3, 'VALID'),
        _conv_case('narrow-3-rows-a-chunk', 4, 9, 5, 20, 96, 3, 3, 1, 1, 'SAME', scaled=True),
        _conv_case('narrow-w1', 3, 23, 1, 12, 64, 7, 1, 2, 1, 'SAME'),
        _conv_case('one-pixel', 1, 3, 3, 8, 4, 3, 3, 1, 1, 'VALID'),
    ]
    # -- enough pixels for deep pixel-range splits with a ragged last range, in each of the three default families
    cases += [
        _row_case('row-28x56', 1, 28, 56, 64, 64, 3, 1, -1, HG=28),
        _conv_case('big-fold-5x1', 2, 40, 33, 16, 32, 5, 1, 1, 1, 'SAME'),
        _conv_case('big-2x2', 3, 31, 37, 36, 100, 2, 2, 1, 1, 'VALID', scaled=True),
    ]
    # -- conv2d_transpose form (G on the fine grid) and the fully connected form (1x1 grid, the rows are the pixels: deep pixel splits,
    #    ragged and empty trailing pixel ranges)
    cases += [
        _deconv_case('deconv-3x5-s1', 2, 5, 10, 128, 64, 3, 5, 1, 1),
        _deconv_case('deconv-3x5-s2', 3, 7, 6, 36, 20, 3, 5, 2, 2, scaled=True),
        _deconv_case('deconv-7x4-s4x3', 1, 6, 9, 64, 32, 7, 4, 4, 3),
        _deconv_case('deconv-2x3-s3x1', 2, 4, 13, 8, 132, 2, 3, 3, 1),
        _fc_case('fc-7', 7, 64, 64),
        _fc_case('fc-96-n100', 96, 512, 100),
        _fc_case('fc-3000', 3000, 136, 20, scaled=True),
        _fc_case('fc-2049', 2049, 36, 256),
        _fc_case('fc-1', 1, 4, 4),
        _fc_case('fc-8200', 8200, 8, 8),                                        # 64 pixel ranges, the last seven of them empty
        _conv_case('taps-35', 4, 37, 35, 20, 8, 7, 5, 1, 1, 'VALID'),                   # many tiles: the workgroup target decides the split
    ]
    # -- random draws
    r = np.random.default_rng(20240611)
    i = 0
    while i < 40:
        kh, kw = int(r.choice([1, 2, 3, 5, 7, 9])), int(r.choice([1, 3, 4, 5, 7]))
        sh, sw = int(r.choice([1, 2, 3, 4])), int(r.choice([1, 2, 3, 4]))
        Cg = int(r.choice([4, 8, 12, 16, 20, 32, 36, 64, 128, 136]))
        Cd = int(r.choice([4, 8, 20, 32, 64, 96, 100, 128, 132, 256]))
        B = int(r.integers(1, 7))
        form = ('SAME', 'VALID', 'free')[i % 3]
        scaled = i % 3 == 0 if form != 'free' else i % 2 == 0
        if form == 'free':
            Hd, Wd = int(r.integers(1, 10)) | 1, int(r.integers(1, 16)) | 1
            HG, WG = int(r.integers(1, (Hd - 1) * sh + kh + 3)), int(r.integers(1, (Wd - 1) * sw + kw + 3))
            h0, w0 = int(r.integers(-kh, 3)), int(r.integers(-kw, 3))
            c = WgradCase('rand%02d-free' % i, B, HG, WG, Cg, Hd, Wd, Cd, kh, kw, sh, sw, h0, w0, scaled, 'free')
        else:
            H, W = (kh + int(r.integers(0, 12))) | 1, (kw + int(r.integers(0, 18))) | 1
            c = _conv_case('rand%02d-%s' % (i, form.lower()), B, H, W, Cg, Cd, kh, kw, sh, sw, form, scaled)
        if _macs(c) > MAC_CAP:
            continue
        cases.append(c)
        i += 1
    assert len({c.name for c in cases}) == len(cases)
    return cases


def wgrad_operands(c, integers=False):
    """(G, D) float32 of a case: N(0,1), each channel scaled by 2^U(-6,6) in the `scaled` cases; or integers of -2..2."""
    r = np.random.default_rng(sum(map(ord, c.name)) * 7919 + (1 if integers else 0))
    gs, ds = (c.B, c.HG, c.WG, c.Cg), (c.B, c.Hd, c.Wd, c.Cd)
    if integers:
        return r.integers(-2, 3, size=gs).astype(np.float32), r.integers(-2, 3, size=ds).astype(np.float32)
    G, D = r.normal(size=gs), r.normal(size=ds)
    if c.scaled:
        G, D = G * 2.0 ** r.uniform(-6, 6, size=c.Cg), D * 2.0 ** r.uniform(-6, 6, size=c.Cd)
    return G.astype(np.float32), D.astype(np.float32)


def integer_exact(n, max_g=2, max_d=2):
    """n products of integers of magnitude <= max_g, max_d: every fp32 partial sum, in any order, is an integer below 2^24."""
    return n * max_g * max_d < 2 ** 24


# -- what csrc/wgrad.hip's wgrad_shape / wgrad_pick_splitk choose, restated: the sweeps assert it against the library's own answer
#    (sagen_wgrad_kernel_name), case by case and under every kernel-selection switch
SELECTIONS = [{}, {'SAGEN_WGRAD_F32': '1'}, {'SAGEN_FP32_ONLY': '1'}, {'SAGEN_WGRAD_REF': '1'}, {'SAGEN_WGRAD_NOROW': '1'},
              {'SAGEN_WGRAD_NOFOLD': '1'}, {'SAGEN_WGRAD_WGS': '64'}, {'SAGEN_WGRAD_WGS': '8192'}]
SELECTION_KEYS = ('SAGEN_WGRAD_F32', 'SAGEN_FP32_ONLY', 'SAGEN_WGRAD_REF', 'SAGEN_WGRAD_NOROW', 'SAGEN_WGRAD_NOFOLD', 'SAGEN_WGRAD_WGS')

WgradPlan = collections.namedtuple('WgradPlan', 'kernel bm bn fold splitk row nchunks ntile')


def cdiv(a, b):
    return -(-a // b)


def wgrad_plan(c, env=None, split=True):
    env = env or {}
    exact = 'SAGEN_FP32_ONLY' in env or 'SAGEN_WGRAD_F32' in env
    row = ('SAGEN_WGRAD_NOROW' not in env and not exact and c.kw == 3 and c.sw == 1 and c.w0 == -1 and c.WG == c.Wd and c.Wd >= 12)
    bm = 128 if c.Cg > 64 else 64
    bn = 128 if (c.Cd > 64 and not row) else 64
    fold = 128 // c.Cg if ('SAGEN_WGRAD_NOFOLD' not in env and not exact and not row and c.kw == 1 and c.kh >= 2 and c.Cg in (16, 32)) else 1
    if fold > 1:
        bm = 128
    P = c.B * c.Hd * (c.Wd + 1 if row else c.Wd)
    nchunks = cdiv(P, 16)
    ntile = cdiv(c.kh, fold) * cdiv(c.Cd, bn) if fold > 1 else c.kh * (1 if row else c.kw) * cdiv(c.Cg, bm) * cdiv(c.Cd, bn)
    per = c.kh * c.kw * c.Cg * c.Cd
    splitk = 1
    if split:
        forced = max(64, int(env['SAGEN_WGRAD_WGS'])) if 'SAGEN_WGRAD_WGS' in env else 0
        target = forced or (512 if (1024 // ntile) * per * 4 > (32 << 20) else 1024)
        splitk = max(1, min(target // ntile, nchunks // 8))
        splitk = min(splitk, 64, 256)                      # (sagen_wgrad_scratch_bytes holds 64 partials)
    if 'SAGEN_WGRAD_REF' in env:
        return WgradPlan('wgrad_ref_kernel', 0, 0, 1, 1, False, nchunks, ntile)
    kernel = 'wgrad_kernel' if exact else ('wgrad3r_kernel' if row else 'wgrad3_kernel')
    return WgradPlan(kernel, bm, bn, fold, splitk, row, nchunks, ntile)


def plan_string(p):
    if p.kernel == 'wgrad_ref_kernel':
        return 'wgrad_ref_kernel fold=1 splitk=1'
    return '%s<%d,%d> fold=%d splitk=%d' % (p.kernel, p.bm, p.bn, p.fold, p.splitk)


def wgrad_classes(c):
    """The directed classes a case belongs to (default kernel selection)."""
    p = wgrad_plan(c)
    out = {'form:' + c.form.split('-')[0]}
    if not p.row and p.fold == 1:
        out.add('tile:%dx%d' % (p.bm, p.bn))
    if p.row:
        out.add('row:th%d-sh%d' % (c.kh, c.sh))
        out.add('rowtile:%d' % p.bm)
        if c.Wd == 12:
            out.add('row:wd12')
        if c.Hd in (1, 2):
            out.add('row:hd%d' % c.Hd)
        if c.Hd == 1 and c.B >= 3 and c.Wd + 1 <= 14:
            out.add('row:chunk-spans-3-images')
        if (c.B * c.Hd * (c.Wd + 1)) % 16:
            out.add('row:grid-off-16')
        if c.Wd + 1 <= 14 and c.Hd >= 3:
            out.add('row:chunk-spans-3-rows')
        if c.Cd % 64:
            out.add('row:cd-tail')
    else:
        if 1 < c.Wd <= 7 and c.Hd >= 3:
            out.add('chunk-spans-3-rows')
    if p.fold > 1:
        out.add('fold:cg%d-th%d' % (c.Cg, c.kh))
    if p.fold == 1 and not p.row:
        if p.bm == 64 and c.Cg % 64:
            out.add('cg-tail-in-64')
        if p.bm == 128 and c.Cg % 128:
            out.add('cg-tail-in-128')
        if p.bn == 64 and c.Cd % 64:
            out.add('cd-tail-in-64')
        if p.bn == 128 and c.Cd % 128:
            out.add('cd-tail-in-128')
    if c.form == 'fc' and c.B >= 2000:
        out.add('fc-thousands')
    if p.splitk >= 8 and p.nchunks % p.splitk:
        out.add('split:deep-ragged')
    if p.splitk > 1 and cdiv(p.nchunks, p.splitk) * (p.splitk - 1) >= p.nchunks:
        out.add('split:empty-last-range')
    if c.h0 > 0 or c.w0 > 0:
        out.add('origin-positive')
    return out


WGRAD_REQUIRED_CLASSES = (
    ['row:th%d-sh%d' % (t, s) for t in (1, 3, 5, 7) for s in (1, 2, 3)] + ['row:wd12', 'row:hd1', 'row:hd2', 'row:grid-off-16',
    'row:chunk-spans-3-rows', 'row:chunk-spans-3-images', 'chunk-spans-3-rows', 'rowtile:64', 'rowtile:128', 'row:cd-tail'] +
    ['fold:cg%d-th%d' % (g, t) for g in (16, 32) for t in (2, 3, 4, 6, 9, 10)] +
    ['tile:64x64', 'tile:64x128', 'tile:128x64', 'tile:128x128', 'cg-tail-in-64', 'cg-tail-in-128', 'cd-tail-in-64', 'cd-tail-in-128',
     'form:conv', 'form:free', 'form:deconv', 'form:fc', 'fc-thousands', 'split:deep-ragged', 'origin-positive'])


def wgrad_supported(c):
    """What include/sagen.h documents for sagen_wgrad: positive sizes, cg and cd multiples of 4."""
    return min(c.B, c.HG, c.WG, c.Cg, c.Hd, c.Wd, c.Cd, c.kh, c.kw, c.sh, c.sw) >= 1 and c.Cg % 4 == 0 and c.Cd % 4 == 0


# ------------------------------------------------------------------------------------------------------------------------
# sagen_conv2d_bwd_data cases
# ------------------------------------------------------------------------------------------------------------------------
DgradCase = collections.namedtuple('DgradCase', 'name B H W cin cout kh kw sh sw padding')


def dgrad_out_hw(c):
    if c.padding == 'SAME':
        return same_pad(c.H, c.kh, c.sh)[0], same_pad(c.W, c.kw, c.sw)[0]
    return (c.H - c.kh) // c.sh + 1, (c.W - c.kw) // c.sw + 1


def dgrad_unread(c):
    """(first unread row, first unread column) of a VALID conv's input (H, W when every row / column is read)."""
    Ho, Wo = dgrad_out_hw(c)
    if c.padding != 'VALID':
        return c.H, c.W
    return (Ho - 1) * c.sh + c.kh, (Wo - 1) * c.sw + c.kw


def dgrad_supported(c):
    """include/sagen.h: cout a power of two >= 4 (cin a multiple of 4); stride 1 any padding; strided: VALID, or SAME without padding before."""
    if c.cout < 4 or c.cout & (c.cout - 1) or c.cin % 4 or c.H < c.kh and c.padding == 'VALID' or c.W < c.kw and c.padding == 'VALID':
        return False
    if c.sh == 1 and c.sw == 1 or c.padding == 'VALID':
        return True
    return same_pad(c.H, c.kh, c.sh)[1] == 0 and same_pad(c.W, c.kw, c.sw)[1] == 0


def dgrad_cases():
    D = DgradCase
    cases = [
        # strided VALID whose last rows / columns no window reads: dx must hold exact zeros there
        D('unread-rows', 2, 16, 15, 16, 32, 5, 3, 3, 2, 'VALID'),
        D('unread-cols', 1, 9, 12, 4, 4, 3, 3, 2, 4, 'VALID'),
        D('unread-both', 3, 12, 14, 12, 64, 2, 4, 3, 3, 'VALID'),
        D('unread-1x1-s2', 2, 8, 6, 20, 8, 1, 1, 2, 2, 'VALID'),
        D('unread-7x1-s4', 2, 26, 5, 8, 16, 7, 1, 4, 1, 'VALID'),
        D('unread-cin64', 1, 10, 11, 64, 128, 3, 5, 2, 4, 'VALID'),
        D('unread-cout256', 1, 7, 10, 32, 256, 2, 3, 4, 2, 'VALID'),
        D('unread-wide-stride', 2, 5, 13, 4, 16, 1, 3, 3, 4, 'VALID'),
        # strided SAME whose total padding is 0 or 1, all of it after
        D('same-s2-3x3', 2, 10, 18, 32, 64, 3, 3, 2, 2, 'SAME'),
        D('same-s2-1x1', 2, 9, 7, 12, 128, 1, 1, 2, 2, 'SAME'),
        D('same-s3-4x3', 1, 12, 9, 8, 8, 4, 3, 3, 3, 'SAME'),
        D('same-s2-2x2', 3, 7, 5, 20, 4, 2, 2, 2, 2, 'SAME'),
        D('same-s4-5x4', 1, 16, 12, 4, 32, 5, 4, 4, 4, 'SAME'),
        # stride 1 at the largest filter
        D('s1-7x7-same', 1, 9, 10, 8, 16, 7, 7, 1, 1, 'SAME'),
        D('s1-7x7-valid', 2, 8, 11, 4, 64, 7, 7, 1, 1, 'VALID'),
    ]
    r = np.random.default_rng(4242)
    i = 0
    while i < 22:
        kh, kw = int(r.integers(1, 8)), int(r.integers(1, 8))
        cout, cin = int(2 ** r.integers(2, 9)), int(r.choice([4, 8, 12, 20, 32, 64]))
        B = int(r.integers(1, 5))
        if i < 14:                                      # stride 1, SAME and VALID alternately
            c = D('s1-%02d' % i, B, kh + int(r.integers(0, 10)), kw + int(r.integers(0, 14)), cin, cout, kh, kw, 1, 1, 'SAME' if i % 2 else 'VALID')
        else:                                           # strided VALID, any remainder
            sh, sw = int(r.integers(1, 5)), int(r.integers(2, 5))
            c = D('sv-%02d' % i, B, kh + int(r.integers(0, 12)), kw + int(r.integers(0, 12)), cin, cout, kh, kw, sh, sw, 'VALID')
        if float(B * c.H * c.W) * kh * kw * cin * cout > MAC_CAP:
            continue
        cases.append(c)
        i += 1
    assert len({c.name for c in cases}) == len(cases)
    return cases


def dgrad_operands(c, integers=False):
    r = np.random.default_rng(sum(map(ord, c.name)) * 104729 + (1 if integers else 0))
    Ho, Wo = dgrad_out_hw(c)
    ws, ds = (c.kh, c.kw, c.cin, c.cout), (c.B, Ho, Wo, c.cout)
    if integers:
        return r.integers(-2, 3, size=ws).astype(np.float32), r.integers(-2, 3, size=ds).astype(np.float32)
    return (r.normal(size=ws) / np.sqrt(c.kh * c.kw * c.cin)).astype(np.float32), r.normal(size=ds).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# sagen_bn_bwd: every legal channel count
# ------------------------------------------------------------------------------------------------------------------------
BN_LEGAL_C = [4 * d for d in (1, 2, 4, 8, 16, 32, 64, 128, 256)]          # C = 4 * a divisor of 256


def bn_bwd_ref(ga, gb, res, y, gamma, beta, eps=1e-3, relu=True):
    """fp64 autograd of out = [relu](bn_train(y) + res) at y, gamma, beta for the incoming gradient ga (+ gb); y [n, C].
    Returns (dy, dgamma, dbeta, act) with act the forward output (whose sign is the ReLU mask) or None without ReLU."""
    import torch
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    yt, gt, bt = t(y).requires_grad_(True), t(gamma).requires_grad_(True), t(beta).requires_grad_(True)
    mean, var = yt.mean(0), yt.var(0, unbiased=False)
    z = (yt - mean) / torch.sqrt(var + eps) * gt + bt
    if res is not None:
        z = z + t(res)
    out = torch.relu(z) if relu else z
    g = t(ga) + (t(gb) if gb is not None else 0.0)
    out.backward(g)
    return yt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy(), (out.detach().numpy() if relu else None)
