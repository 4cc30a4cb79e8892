"""backward_oracle.py on the host: wgrad_ref pinned against torch fp64 autograd of the three layer forms, and the invariants of the
case generators the device sweeps (test_gpu_backward_ops.py) rely on.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import backward_oracle as BO
from util import rng


def _t(a):
    import torch
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def _close(a, b):
    return np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0)


CONV_GEOMETRIES = [
    # B, H, W, Cin, Cout, kh, kw, sh, sw, padding
    (2, 7, 9, 4, 8, 3, 3, 1, 1, 'SAME'), (1, 8, 5, 8, 4, 2, 4, 2, 1, 'SAME'), (3, 9, 11, 4, 4, 5, 3, 2, 3, 'VALID'),
    (2, 6, 13, 12, 8, 1, 1, 2, 2, 'SAME'), (1, 11, 4, 4, 12, 7, 1, 4, 1, 'VALID'), (2, 5, 5, 8, 8, 5, 5, 1, 1, 'SAME'),
    (1, 10, 9, 4, 4, 9, 7, 3, 4, 'SAME'), (2, 3, 12, 4, 8, 3, 3, 1, 1, 'VALID'), (4, 4, 4, 4, 4, 4, 4, 1, 1, 'SAME'),
]
DECONV_GEOMETRIES = [(2, 3, 5, 8, 4, 3, 5, 1, 1), (1, 4, 3, 4, 12, 3, 5, 2, 2), (2, 2, 4, 4, 4, 7, 4, 4, 3), (3, 5, 1, 8, 4, 2, 3, 3, 1)]


@pytest.mark.parametrize('geo', CONV_GEOMETRIES)
def test_wgrad_ref_is_the_filter_gradient_of_tf_convolution(geo):
    import torch
    from oracle.torch_ref import conv2d_tf
    B, H, W, Cin, Cout, kh, kw, sh, sw, padding = geo
    r = rng(sum(v for v in geo if isinstance(v, int)))
    x, w = r.normal(size=(B, H, W, Cin)), torch.zeros(kh, kw, Cin, Cout, dtype=torch.float64, requires_grad=True)
    y = conv2d_tf(_t(x).permute(0, 3, 1, 2), w, (sh, sw), padding)
    dy = r.normal(size=tuple(y.permute(0, 2, 3, 1).shape))
    y.backward(_t(dy).permute(0, 3, 1, 2))
    c = BO._conv_case('g', B, H, W, Cin, Cout, kh, kw, sh, sw, padding)
    assert (c.Hd, c.Wd) == dy.shape[1:3]
    assert _close(BO.wgrad_ref(x, dy, kh, kw, (sh, sw), (c.h0, c.w0)), w.grad.numpy())
    # the companion sum: the same formula on the magnitudes, an upper bound of every partial sum
    a = BO.wgrad_abs_ref(x, dy, kh, kw, (sh, sw), (c.h0, c.w0))
    assert np.all(a >= np.abs(w.grad.numpy()) - 1e-12) and _close(a, BO.wgrad_ref(np.abs(x), np.abs(dy), kh, kw, (sh, sw), (c.h0, c.w0)))
    # and the data gradient reference of the same layer is the adjoint of the forward: <dy, conv(x)> = <dgrad(dy), x>
    wv = r.normal(size=(kh, kw, Cin, Cout))
    dx = BO.dgrad_ref((B, H, W, Cin), wv, (sh, sw), padding, dy)
    fwd = conv2d_tf(_t(x).permute(0, 3, 1, 2), _t(wv), (sh, sw), padding).permute(0, 2, 3, 1).numpy()
    assert abs(np.sum(dx * x) - np.sum(fwd * dy)) <= 1e-10 * np.sqrt(np.sum(dx ** 2) * np.sum(x ** 2))


@pytest.mark.parametrize('geo', DECONV_GEOMETRIES)
def test_wgrad_ref_is_the_filter_gradient_of_conv2d_transpose(geo):
    import torch
    from oracle.torch_ref import deconv2d_tf
    B, H, W, Cin, Cout, kh, kw, sh, sw = geo
    r = rng(sum(geo))
    x, w = r.normal(size=(B, H, W, Cin)), torch.zeros(kh, kw, Cout, Cin, dtype=torch.float64, requires_grad=True)
    y = deconv2d_tf(_t(x).permute(0, 3, 1, 2), w, (sh, sw))
    dy = r.normal(size=tuple(y.permute(0, 2, 3, 1).shape))
    y.backward(_t(dy).permute(0, 3, 1, 2))
    c = BO._deconv_case('d', B, H, W, Cin, Cout, kh, kw, sh, sw)
    assert (c.HG, c.WG, c.Cg, c.Cd) == dy.shape[1:] + (Cin,)
    assert _close(BO.wgrad_ref(dy, x, kh, kw, (sh, sw), (0, 0)), w.grad.numpy())


@pytest.mark.parametrize('M,K,N', [(7, 8, 4), (33, 12, 20), (1, 4, 4)])
def test_wgrad_ref_is_the_weight_gradient_of_matmul(M, K, N):
    import torch
    r = rng(M + K + N)
    x, dy = r.normal(size=(M, K)), r.normal(size=(M, N))
    w = torch.zeros(K, N, dtype=torch.float64, requires_grad=True)
    (_t(x) @ w).backward(_t(dy))
    assert _close(BO.wgrad_ref(x[:, None, None, :], dy[:, None, None, :], 1, 1)[0, 0], w.grad.numpy())


def test_wgrad_ref_with_free_origins_against_a_pixel_loop():
    """Origins and extents no layer has (positive h0 / w0, G smaller than the taps reach): the formula, pixel by pixel."""
    r = rng(9)
    for (B, HG, WG, Hd, Wd, kh, kw, sh, sw, h0, w0) in [(2, 3, 4, 4, 3, 3, 2, 2, 1, 1, 2), (1, 5, 2, 3, 5, 2, 3, 1, 3, -2, -3), (2, 1, 1, 2, 2, 2, 2, 4, 4, 2, -1),
                                                        (1, 6, 7, 2, 3, 3, 3, 3, 2, -3, 1)]:
        G, D = r.normal(size=(B, HG, WG, 2)), r.normal(size=(B, Hd, Wd, 3))
        ref = np.zeros((kh, kw, 2, 3))
        for th in range(kh):
            for tw in range(kw):
                for b in range(B):
                    for i in range(Hd):
                        for j in range(Wd):
                            gi, gj = i * sh + th + h0, j * sw + tw + w0
                            if 0 <= gi < HG and 0 <= gj < WG:
                                ref[th, tw] += np.outer(G[b, gi, gj], D[b, i, j])
        assert _close(BO.wgrad_ref(G, D, kh, kw, (sh, sw), (h0, w0)), ref)


# ------------------------------------------------------------------------------------------------------------------------
# the generators
# ------------------------------------------------------------------------------------------------------------------------
def test_wgrad_cases_hold_every_directed_class():
    cases = BO.wgrad_cases()
    assert len(cases) >= 60 and len({c.name for c in cases}) == len(cases)
    assert cases == BO.wgrad_cases()                                           # fixed seeds
    assert all(BO.wgrad_supported(c) for c in cases)                           # only calls include/sagen.h documents: nothing to skip at run time
    have = set()
    for c in cases:
        have |= BO.wgrad_classes(c)
    missing = [k for k in BO.WGRAD_REQUIRED_CLASSES if k not in have]
    assert not missing, missing
    # the ranges the random draws come from are reached
    assert {c.kh for c in cases} >= {1, 2, 3, 5, 7, 9} and {c.kw for c in cases} >= {1, 3, 4, 5, 7}
    assert {c.sh for c in cases} >= {1, 2, 3, 4} and {c.sw for c in cases} >= {1, 2, 3, 4}
    assert {c.Cg for c in cases} >= {4, 8, 12, 16, 20, 32, 36, 64, 128, 136} and {c.Cd for c in cases} >= {4, 8, 20, 32, 64, 96, 100, 128, 132, 256}
    assert {c.B for c in cases} >= set(range(1, 7))
    assert {c.form for c in cases} >= {'conv-SAME', 'conv-VALID', 'free', 'deconv', 'fc'}
    assert sum(c.scaled for c in cases) >= len(cases) // 4
    free = [c for c in cases if c.form == 'free']
    assert any(c.h0 > 0 for c in free) and any(c.w0 > 0 for c in free) and any(c.h0 < -1 for c in free)
    # at least half of the cases take the integer known-answer check (in fact all: n * 2 * 2 < 2^24)
    assert sum(BO.integer_exact(c.B * c.Hd * c.Wd) for c in cases) * 2 >= len(cases)
    for c in cases[::7]:
        G, D = BO.wgrad_operands(c, integers=True)
        assert G.shape == (c.B, c.HG, c.WG, c.Cg) and D.shape == (c.B, c.Hd, c.Wd, c.Cd)
        assert set(np.unique(G)) <= {-2, -1, 0, 1, 2} and set(np.unique(D)) <= {-2, -1, 0, 1, 2}
        dw = BO.wgrad_ref(G, D, c.kh, c.kw, (c.sh, c.sw), (c.h0, c.w0))
        assert np.array_equal(dw, dw.astype(np.float32).astype(np.float64))    # the integer answers are fp32 numbers


def test_kernel_selection_matrix_reaches_every_family():
    """What each switch is meant to select, over the sweep's cases (the device children assert it against the library per case)."""
    cases = BO.wgrad_cases()
    plans = lambda env: [BO.wgrad_plan(c, env) for c in cases]
    fam = lambda env: {p.kernel for p in plans(env)}
    assert fam({}) == {'wgrad3_kernel', 'wgrad3r_kernel'} and any(p.fold == 8 for p in plans({})) and any(p.fold == 4 for p in plans({}))
    for env in ({'SAGEN_WGRAD_F32': '1'}, {'SAGEN_FP32_ONLY': '1'}):
        assert fam(env) == {'wgrad_kernel'} and {(p.bm, p.bn) for p in plans(env)} == {(64, 64), (64, 128), (128, 64), (128, 128)}
        assert all(p.fold == 1 for p in plans(env))
    assert fam({'SAGEN_WGRAD_REF': '1'}) == {'wgrad_ref_kernel'}
    assert fam({'SAGEN_WGRAD_NOROW': '1'}) == {'wgrad3_kernel'}
    assert all(p.fold == 1 for p in plans({'SAGEN_WGRAD_NOFOLD': '1'})) and fam({'SAGEN_WGRAD_NOFOLD': '1'}) == fam({})
    deep, shallow = plans({'SAGEN_WGRAD_WGS': '8192'}), plans({'SAGEN_WGRAD_WGS': '64'})
    assert max(p.splitk for p in deep) == 64 and sum(p.splitk for p in deep) > sum(p.splitk for p in plans({}))
    assert sum(p.splitk for p in shallow) < sum(p.splitk for p in plans({}))
    assert [set(e) <= set(BO.SELECTION_KEYS) for e in BO.SELECTIONS] == [True] * 8


def test_wgrad_plan_restates_the_library():
    """sagen_wgrad_kernel_name is host-only: the default selection's plan of every case, with and without a scratch."""
    import os
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    l = _lib.lib()
    env = {k: os.environ[k] for k in BO.SELECTION_KEYS if k in os.environ}
    buf = C.create_string_buffer(128)
    for c in BO.wgrad_cases():
        for split in (True, False):
            nbytes = l.sagen_wgrad_scratch_bytes(c.kh, c.kw, c.Cg, c.Cd) if split else 0
            assert l.sagen_wgrad_kernel_name(c.B, c.HG, c.WG, c.Cg, c.Hd, c.Wd, c.Cd, c.kh, c.kw, c.sh, c.sw, c.h0, c.w0, nbytes, buf, 128) == 0
            assert buf.value.decode() == BO.plan_string(BO.wgrad_plan(c, env, split)), (c.name, split)
    assert l.sagen_wgrad_kernel_name(1, 1, 1, 4, 1, 1, 4, 1, 1, 1, 1, 0, 0, 0, buf, 8) < 0          # buffer too small
    assert l.sagen_wgrad_kernel_name(0, 1, 1, 4, 1, 1, 4, 1, 1, 1, 1, 0, 0, 0, buf, 128) < 0


def test_dgrad_cases_hold_every_directed_class():
    cases = BO.dgrad_cases()
    assert len(cases) >= 30 and cases == BO.dgrad_cases()
    assert all(BO.dgrad_supported(c) for c in cases)
    assert {c.cout for c in cases} >= {4, 8, 16, 32, 64, 128, 256} and {c.cin for c in cases} >= {4, 8, 12, 20, 32, 64}
    s1 = [c for c in cases if c.sh == 1 and c.sw == 1]
    assert {c.padding for c in s1} == {'SAME', 'VALID'} and max(c.kh for c in s1) == 7 and max(c.kw for c in s1) == 7
    strided = [c for c in cases if c.sh > 1 or c.sw > 1]
    assert sum(c.padding == 'VALID' for c in strided) >= 8
    same = [c for c in strided if c.padding == 'SAME']
    assert len(same) >= 4 and all(BO.same_pad(c.H, c.kh, c.sh)[1] == 0 and BO.same_pad(c.W, c.kw, c.sw)[1] == 0 for c in same)
    assert any(BO.same_pad(c.H, c.kh, c.sh)[0] * c.sh - c.sh + c.kh > c.H for c in same)          # (some really pad, after)
    unread = [c for c in strided if c.padding == 'VALID' and ((c.H - c.kh) % c.sh or (c.W - c.kw) % c.sw)]
    assert len(unread) >= 6
    for c in unread:
        r0, c0 = BO.dgrad_unread(c)
        assert r0 < c.H or c0 < c.W
    assert any(BO.dgrad_unread(c)[0] < c.H for c in unread) and any(BO.dgrad_unread(c)[1] < c.W for c in unread)
    assert sum(BO.integer_exact(c.kh * c.kw * c.cout) for c in cases) * 2 >= len(cases)
    c = unread[0]
    w, dy = BO.dgrad_operands(c)
    dx = BO.dgrad_ref((c.B, c.H, c.W, c.cin), w, (c.sh, c.sw), c.padding, dy)
    r0, c0 = BO.dgrad_unread(c)
    assert np.all(dx[:, r0:] == 0) and np.all(dx[:, :, c0:] == 0) and np.any(dx[:, r0 - 1] != 0)


def test_bn_bwd_ref_against_the_closed_form():
    """The batch-norm reference is autograd of the textbook forward; its closed form (what the kernel implements) must agree,
    also for a constant channel (eps decides) and one pixel."""
    assert BO.BN_LEGAL_C == [c for c in range(4, 1025, 4) if 256 % (c // 4) == 0]
    r = rng(3)
    for n in (1, 3, 50):
        y = r.normal(size=(n, 4))
        y[:, 2] = 0.75
        gamma, beta, g = np.array([1.5, -0.5, 2.0, 0.0]), r.normal(size=4), r.normal(size=(n, 4))
        dy, dg, db, act = BO.bn_bwd_ref(g, None, None, y, gamma, beta, relu=False)
        assert act is None
        inv = 1.0 / np.sqrt(y.var(0) + 1e-3)
        xh = (y - y.mean(0)) * inv
        assert _close(db, g.sum(0)) and _close(dg, (g * xh).sum(0))
        assert np.abs(dy - gamma * inv * (g - g.mean(0) - xh * (g * xh).mean(0))).max() < 1e-12
