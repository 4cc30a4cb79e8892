"""forward_oracle.py on the host: the references pinned against an independent fp64 implementation (torch on the CPU), the invariants
of the case generators the device sweeps (test_gpu_forward_ops.py) rely on, and forward_plan against the library's own host-only
accessors.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import forward_oracle as FO
from util import rng


def _t(a):
    import torch
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def _close(a, b):
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0)


CONV_GEOMETRIES = [
    # B, H, W, Cin, Cout, kh, kw, sh, sw, padding
    (2, 7, 9, 4, 8, 3, 3, 1, 1, 'SAME'), (1, 8, 5, 8, 4, 2, 4, 2, 1, 'SAME'), (3, 9, 11, 4, 4, 5, 3, 2, 3, 'VALID'),
    (2, 6, 13, 12, 8, 1, 1, 2, 2, 'SAME'), (1, 11, 4, 1, 12, 7, 1, 4, 1, 'VALID'), (2, 5, 5, 3, 8, 5, 5, 1, 1, 'SAME'),
    (1, 10, 9, 4, 4, 9, 7, 3, 4, 'SAME'), (2, 3, 12, 4, 8, 3, 3, 1, 1, 'VALID'), (4, 4, 4, 4, 4, 4, 4, 1, 1, 'SAME'),
    (1, 22, 26, 3, 4, 7, 7, 2, 2, 'SAME'), (2, 8, 9, 8, 4, 2, 3, 2, 3, 'SAME'),
]


@pytest.mark.parametrize('geo', CONV_GEOMETRIES)
def test_conv_ref_is_tf_convolution(geo):
    """Against torch.nn.functional.conv2d in float64 with TF's SAME padding written out here (the smaller half before), with and
    without the prologue; the companion sums against their definitions."""
    import torch.nn.functional as F
    B, H, W, Cin, Cout, kh, kw, sh, sw, padding = geo
    r = rng(sum(v for v in geo if isinstance(v, int)))
    x, w = r.normal(size=(B, H, W, Cin)), r.normal(size=(kh, kw, Cin, Cout))
    sc, sf = r.uniform(-1.5, 1.5, size=Cin), r.normal(size=Cin)

    def torch_conv(xin, w=w):
        xt = _t(xin).permute(0, 3, 1, 2)
        if padding == 'SAME':
            Ho, Wo = -(-H // sh), -(-W // sw)
            th, tw = max((Ho - 1) * sh + kh - H, 0), max((Wo - 1) * sw + kw - W, 0)
            xt = F.pad(xt, (tw // 2, tw - tw // 2, th // 2, th - th // 2))
        return F.conv2d(xt, _t(w).permute(3, 2, 0, 1), stride=(sh, sw)).permute(0, 2, 3, 1).numpy()

    assert _close(FO.conv_ref(x, w, (sh, sw), padding), torch_conv(x))
    xin = np.maximum(x * sc + sf, 0)
    assert _close(FO.conv_ref(x, w, (sh, sw), padding, sc, sf), torch_conv(xin))          # the prologue comes BEFORE the padding
    A = FO.conv_abs_ref(x, w, (sh, sw), padding, sc, sf)
    assert _close(A, FO.conv_ref(np.abs(xin), np.abs(w), (sh, sw), padding)) and np.all(A >= np.abs(torch_conv(xin)) - 1e-12)
    assert _close(FO.conv_prologue_abs_ref(x, w, (sh, sw), padding, sc, sf), FO.conv_ref(np.abs(x * sc) + np.abs(sf), np.abs(w), (sh, sw), padding))
    assert np.all(FO.conv_prologue_abs_ref(x, w, (sh, sw), padding, sc, sf) >= A - 1e-12)
    n = FO.conv_terms(x.shape, w.shape, (sh, sw), padding)
    assert _close(n, torch_conv(np.ones((1, H, W, Cin)), np.ones((kh, kw, Cin, 1))))
    assert n.max() <= kh * kw * Cin and n.min() >= Cin and (padding == 'SAME' or n.min() == kh * kw * Cin)
    st = FO.stats_ref(torch_conv(x))
    assert _close(st[:Cout], torch_conv(x).sum((0, 1, 2))) and _close(st[Cout:], (torch_conv(x) ** 2).sum((0, 1, 2)))


@pytest.mark.parametrize('geo', [(2, 3, 5, 8, 4, 3, 5, 1, 1), (1, 4, 3, 4, 12, 3, 5, 2, 2), (2, 2, 4, 4, 4, 7, 4, 4, 3), (3, 5, 1, 8, 6, 2, 3, 2, 1),
                                 (1, 1, 6, 4, 4, 2, 2, 2, 2)])
def test_deconv_ref_is_conv2d_transpose(geo):
    import torch.nn.functional as F
    B, H, W, Cin, Cout, kh, kw, sh, sw = geo
    r = rng(sum(geo))
    x, w = r.normal(size=(B, H, W, Cin)), r.normal(size=(kh, kw, Cout, Cin))
    ref = F.conv_transpose2d(_t(x).permute(0, 3, 1, 2), _t(w).permute(3, 2, 0, 1), stride=(sh, sw)).permute(0, 2, 3, 1).numpy()
    assert ref.shape == (B, H * sh + kh - sh, W * sw + kw - sw, Cout)
    assert _close(FO.deconv_ref(x, w, (sh, sw)), ref)
    assert np.all(FO.deconv_abs_ref(x, w, (sh, sw)) >= np.abs(ref) - 1e-12)
    n = FO.deconv_terms(x.shape, w.shape, (sh, sw))
    assert _close(n, F.conv_transpose2d(_t(np.ones((1, Cin, H, W))), _t(np.ones((Cin, 1, kh, kw))), stride=(sh, sw)).permute(0, 2, 3, 1).numpy())
    assert n.min() >= Cin and n.max() <= -(-kh // sh) * -(-kw // sw) * Cin


@pytest.mark.parametrize('M,K,N', [(7, 8, 4), (33, 12, 20), (1, 4, 1)])
def test_fc_ref_is_matmul(M, K, N):
    import torch
    r = rng(M + K + N)
    x, w = r.normal(size=(M, K)), r.normal(size=(K, N))
    assert _close(FO.fc_ref(x, w), torch.matmul(_t(x), _t(w)).numpy())
    assert _close(FO.fc_abs_ref(x, w), torch.matmul(_t(x).abs(), _t(w).abs()).numpy())


# ------------------------------------------------------------------------------------------------------------------------
# the generators
# ------------------------------------------------------------------------------------------------------------------------
def test_cases_hold_every_directed_class():
    cases = FO.all_cases()
    assert cases == FO.all_cases()                                             # fixed seeds
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert not [(a, b) for a in names for b in names if a != b and a in b]     # `-k` selects by substring: no name inside another
    assert all(FO.conv_supported(c) for c in FO.conv_cases())                  # only calls include/sagen.h documents: nothing to skip at run time
    assert all(c.K % 4 == 0 for c in FO.fc_cases()) and all(c.kh >= c.sh and c.kw >= c.sw and c.cin & (c.cin - 1) == 0 for c in FO.deconv_cases())
    have = set()
    for c in cases:
        have |= FO.forward_classes(c)
    missing = [k for k in FO.FORWARD_REQUIRED_CLASSES if k not in have]
    assert not missing, missing
    assert max(FO.conv_macs(c) for c in FO.conv_cases()) <= FO.MAC_CAP and max(float(c.M) * c.K * c.N for c in FO.fc_cases()) <= FO.MAC_CAP
    assert {c.prologue for c in FO.conv_cases()} == set(FO.PROLOGUES)


def test_integer_cases_are_exact_and_every_statistic_is_checked():
    """The integer operands are what the docstrings say, every case takes the integer check, and every case with statistics meets the
    condition under which the kernels' fp32 tile sums are exact: no check is skipped at run time."""
    for c in FO.conv_cases():
        x, w, b, sc, sf = FO.conv_operands(c, integers=True)
        assert set(np.unique(x)) <= {-2, -1, 0, 1, 2} and set(np.unique(w)) <= {-2, -1, 0, 1, 2}
        assert (b is None) == (not c.bias) and (sc is None) == (not c.prologue)
        if c.prologue:
            assert set(np.unique(sc)) <= {-2, -1, 1, 2} and set(np.unique(sf)) <= {-2, -1, 0, 1, 2} and (c.prologue != 'posshift' or sf.min() >= 1)
            assert (c.prologue != 'neg' or sc.min() < 0) and np.abs(FO.prologue(x, sc, sf)).max() <= FO.CONV_INT_X_RANGE[c.prologue]
            fx, fw, fb, fsc, fsf = FO.conv_operands(c)
            assert (c.prologue != 'neg' or fsc.min() < 0) and (c.prologue != 'posshift' or fsf.min() > 0)
        geo = ((c.sh, c.sw), c.padding)
        assert FO.integer_exact(int(FO.conv_terms(x.shape, w.shape, *geo).max()), FO.CONV_INT_X_RANGE[c.prologue]), c.name
        raw = FO.conv_ref(x, w, *geo, sc, sf)
        assert np.array_equal(raw, raw.astype(np.float32).astype(np.float64))
        if c.stats:
            assert FO.stats_exact(raw), c.name
    assert all(FO.integer_exact(c.K) for c in FO.fc_cases())
    assert not FO.stats_exact(np.full((256, 1), 300.0)) and FO.stats_exact(np.full((256, 1), 255.0)) and FO.stats_exact(np.full((3, 2), 2000.0))


def test_a_positive_shift_tells_pad_then_bn_from_bn_then_pad():
    """The 'posshift' cases exist to catch a prologue applied to the padding: the reference must differ from that mistake."""
    c = next(c for c in FO.conv_cases() if 'conv:prologue-posshift-padded' in FO.forward_classes(c))
    x, w, _, sc, sf = FO.conv_operands(c)
    Ho, Wo, pt, pb, pl, pr = FO.conv_out(c)
    wrong = FO.conv_ref(np.maximum(np.pad(x.astype(np.float64), ((0, 0), (pt, pb), (pl, pr), (0, 0))) * sc + sf, 0), w, (c.sh, c.sw), 'VALID')
    right = FO.conv_ref(x, w, (c.sh, c.sw), c.padding, sc, sf)
    assert wrong.shape == right.shape and np.abs(wrong - right).max() > 1e-2
    assert np.array_equal(wrong[:, 1:-1, 1:-1], right[:, 1:-1, 1:-1]) or pt + pb > 2 or pl + pr > 2


# ------------------------------------------------------------------------------------------------------------------------
# forward_plan against the library (the accessors are host only: libsagen_hip.so answers them without a device)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _library_plan(lib, c, scratch='full'):
    from spatialaudiogen_amd import ops
    buf = C.create_string_buffer(128)
    if isinstance(c, FO.ConvCase):
        nbytes = ops.conv_2d_scratch_bytes(c.B, c.H, c.W, c.kh, c.kw, c.cin, c.cout, scratch == 'full')
        rc = lib.sagen_conv2d_kernel_name(c.B, c.H, c.W, c.cin, c.kh, c.kw, c.cout, c.sh, c.sw, int(c.padding == 'SAME'), int(bool(c.prologue)),
                                          int(c.stats), int(c.bias), nbytes, buf, 128)
    elif isinstance(c, FO.FcCase):
        rc = lib.sagen_fc_kernel_name(c.M, c.K, c.N, int(c.bias), lib.sagen_fc_scratch_bytes(c.M, c.K, c.N), buf, 128)
    else:
        rc = lib.sagen_deconv2d_kernel_name(c.B, c.H, c.W, c.cin, c.kh, c.kw, c.cout, c.sh, c.sw, int(c.bias),
                                            lib.sagen_deconv2d_scratch_bytes(c.kh, c.kw, c.cin, c.cout, c.sh, c.sw), buf, 128)
    assert rc == 0, (c.name, lib.sagen_last_error())
    return buf.value.decode()


def test_forward_plan_restates_the_library(lib):
    """Every case with both scratch sizes under the selection of this process's environment (the default one in the suite)."""
    from spatialaudiogen_amd import ops
    env = {k: os.environ[k] for k in FO.SELECTION_KEYS if k in os.environ}
    assert [lib.sagen_tile_name(i).decode() for i in range(lib.sagen_num_tiles())] == FO.TILE_NAMES
    for c in FO.all_cases():
        for scratch in FO.SCRATCHES:
            assert _library_plan(lib, c, scratch) == FO.plan_string(FO.forward_plan(c, env, scratch)), (c.name, scratch)
    for c in FO.conv_cases():                                                   # the two scratch sizes differ exactly where the planes have room
        full, pre = (ops.conv_2d_scratch_bytes(c.B, c.H, c.W, c.kh, c.kw, c.cin, c.cout, p) for p in (True, False))
        assert (pre < full) == FO.has_plane_room(c) and pre == lib.sagen_conv2d_min_scratch_bytes(c.B, c.H, c.W, c.kh, c.kw, c.cin, c.cout), c.name
        args = (c.B, c.H, c.W, c.cin, c.kh, c.kw, c.cout, c.sh, c.sw, int(c.padding == 'SAME'), int(bool(c.prologue)), int(c.stats), int(c.bias))
        buf = C.create_string_buffer(128)
        assert lib.sagen_conv2d_kernel_name(*args, pre, buf, 128) == 0 and lib.sagen_conv2d_kernel_name(*args, pre - 1, buf, 128) == -5, c.name


def test_selection_matrix_reaches_every_family_and_every_tile():
    """What each switch is meant to select, over the sweeps' cases (the device children assert it against the library per case)."""
    cases = FO.all_cases()
    fam = lambda env: {FO.forward_plan(c, env, s).tile.family for c in cases for s in FO.SCRATCHES}
    assert fam({}) == {'igemm_kernel', 'igemm3_kernel', 'igemm3dw_kernel', 'conv3p_kernel'} == set(FO.OP_LEVEL_FAMILIES)
    assert fam({'SAGEN_NO_P3': '1'}) == {'igemm_kernel', 'igemm3_kernel', 'igemm3dw_kernel'}
    assert fam({'SAGEN_FP32_ONLY': '1'}) == {'igemm_kernel'}
    assert {FO.forward_plan(c).tile.family for c in FO.fc_cases()} == {'igemm_kernel'}                      # sagen_fc never splits its filter
    assert all(FO.forward_plan(c, {}, 'full').planes and FO.forward_plan(c, {}, 'pre-planes').tile.family == 'igemm3dw_kernel'
               for c in FO.conv_cases() if 'p3' in FO.forward_classes(c))
    assert any(FO.forward_plan(c).splitk == 1 for c in FO.fc_cases()) and {FO.forward_plan(c).splitk for c in FO.fc_cases()} >= {2, 3, 5, 7, 8}
    # every tile of the registry is either forceable onto a case the force applies to (found from forward_plan alone) or named with the
    # reason why no op-level call launches it; of the forceable ones only the tiles named in NOT_SWEPT go without a selection child
    forceable = [i for i, t in enumerate(FO.TILES) if any(FO.force_applies(FO.problem(c)) and FO.forward_plan(c, {'SAGEN_FORCE_TILE': str(i)}, s).tile is t
                                                          for c in cases for s in FO.SCRATCHES)]
    assert forceable == FO.forceable_tiles() and len(FO.TILES) == len(FO.TILE_NAMES) == len(set(FO.TILE_NAMES))
    assert {FO.TILE_NAMES[i] for i in forceable} == set(FO.TILE_NAMES) - set(FO.NOT_AT_OP_LEVEL)
    assert all(len(why) > 20 for why in list(FO.NOT_AT_OP_LEVEL.values()) + list(FO.NOT_SWEPT.values()))
    assert set(FO.NOT_SWEPT) == {'conv3pp_kernel<0>', 'conv3pp_kernel<1>'} <= {FO.TILE_NAMES[i] for i in forceable}
    assert FO.swept_tiles() == [i for i in forceable if FO.TILE_NAMES[i] not in FO.NOT_SWEPT]
    assert {FO.TILES[i].family for i in FO.swept_tiles()} == set(FO.OP_LEVEL_FAMILIES + FO.FORCED_ONLY_FAMILIES)
    assert all(i in forceable for i, t in enumerate(FO.TILES) if t.family in FO.OP_LEVEL_FAMILIES)
    g = FO.TILE_NAMES.index('conv3g_kernel<128,64,64,32,2,false>')              # gathered tiles: plane cases without a prologue only
    sel = FO.selection_cases({'SAGEN_FORCE_TILE': str(g)})
    assert len(sel) == 2 and all(FO.problem(c).dw3 and not c.prologue and FO.forward_plan(c, {'SAGEN_FORCE_TILE': str(g)}).planes for c in sel)
    assert all(FO.forward_plan(c, {'SAGEN_FORCE_TILE': str(g)}) == FO.forward_plan(c) for c in cases if isinstance(c, FO.ConvCase) and c.prologue)
    forceable = FO.swept_tiles()
    for i in forceable:
        env = {'SAGEN_FORCE_TILE': str(i)}
        sel = FO.selection_cases(env)
        assert 1 <= len(sel) <= 8 and all(FO.force_applies(FO.problem(c)) for c in sel)
        assert all(any(FO.forward_plan(c, env, s).tile is FO.TILES[i] for s in FO.SCRATCHES) for c in sel), FO.TILE_NAMES[i]
    # a K tile of 32 refuses Kpad % 32 != 0, the prologue refuses a tile whose K tile straddles taps, the force needs M > 128 and N >= 64
    k32 = FO.TILE_NAMES.index('igemm_kernel<64,64,32,32,2,32>')
    c = next(c for c in FO.conv_cases() if c.name == 'g_kpad48')
    assert FO.forward_plan(c, {'SAGEN_FORCE_TILE': str(k32)}) == FO.forward_plan(c)
    c = next(c for c in FO.conv_cases() if c.name == 'g_m6')
    assert all(FO.forward_plan(c, {'SAGEN_FORCE_TILE': str(i)}) == FO.forward_plan(c) for i in range(len(FO.TILES)))
    assert len(FO.selection_cases({'SAGEN_NO_P3': '1'})) >= 6 and len(FO.selection_cases({'SAGEN_FP32_ONLY': '1'})) >= 40


def test_accessors_refuse_bad_arguments_and_short_buffers(lib):
    buf = C.create_string_buffer(128)
    big, WS = 1 << 30, -5                                                       # SAGEN_ERR_WORKSPACE
    assert lib.sagen_conv2d_kernel_name(1, 6, 6, 8, 3, 3, 8, 1, 1, 1, 0, 0, 0, big, buf, 128) == 0
    assert lib.sagen_conv2d_kernel_name(1, 6, 6, 8, 3, 3, 8, 1, 1, 1, 0, 0, 0, big, buf, 8) < 0            # buffer too small
    assert lib.sagen_conv2d_kernel_name(1, 6, 6, 8, 3, 3, 8, 1, 1, 1, 0, 0, 0, big, None, 128) < 0
    assert lib.sagen_conv2d_kernel_name(0, 6, 6, 8, 3, 3, 8, 1, 1, 1, 0, 0, 0, big, buf, 128) < 0          # bad dimensions
    assert lib.sagen_conv2d_kernel_name(1, 6, 6, 8, 3, 3, 8, 1, 1, 2, 0, 0, 0, big, buf, 128) < 0          # padding
    assert lib.sagen_conv2d_kernel_name(1, 6, 6, 12, 3, 3, 8, 1, 1, 1, 0, 0, 0, big, buf, 128) < 0         # cin
    assert lib.sagen_conv2d_kernel_name(1, 2, 2, 8, 3, 3, 8, 1, 1, 0, 0, 0, 0, big, buf, 128) < 0          # VALID larger than the input
    assert lib.sagen_conv2d_kernel_name(1, 6, 6, 8, 3, 3, 8, 1, 1, 1, 1, 0, 0, big, buf, 128) < 0          # prologue with cin % 16 != 0
    assert b'cannot run' in lib.sagen_last_error()
    assert lib.sagen_conv2d_kernel_name(1, 6, 6, 3, 3, 3, 8, 1, 1, 1, 1, 0, 0, big, buf, 128) < 0          # prologue with cin 3
    assert lib.sagen_conv2d_kernel_name(1, 6, 6, 8, 3, 3, 8, 1, 1, 1, 0, 0, 0, 64, buf, 128) == WS         # SAGEN_ERR_WORKSPACE: short scratch
    assert b'scratch too small' in lib.sagen_last_error()
    assert lib.sagen_fc_kernel_name(4, 8, 8, 1, big, buf, 128) == 0
    assert lib.sagen_fc_kernel_name(4, 6, 8, 1, big, buf, 128) < 0 and lib.sagen_fc_kernel_name(4, 8, 8, 1, 64, buf, 128) == WS
    assert lib.sagen_fc_kernel_name(4, 8, 8, 1, big, buf, 16) < 0 and lib.sagen_fc_kernel_name(4, 8, 0, 1, big, buf, 128) < 0
    assert lib.sagen_deconv2d_kernel_name(1, 2, 2, 8, 2, 2, 8, 2, 2, 1, big, buf, 128) == 0
    assert lib.sagen_deconv2d_kernel_name(1, 2, 2, 8, 1, 1, 8, 2, 2, 1, big, buf, 128) < 0                 # kernel smaller than the stride
    assert lib.sagen_deconv2d_kernel_name(1, 2, 2, 12, 2, 2, 8, 2, 2, 1, big, buf, 128) < 0 and lib.sagen_deconv2d_kernel_name(1, 2, 2, 8, 2, 2, 8, 2, 2, 1, 0, buf, 128) == WS
    assert lib.sagen_deconv2d_kernel_name(1, 2, 2, 8, 2, 2, 8, 2, 2, 1, big, buf, 95) < 0
