"""The space-to-depth instantiations of conv3h_kernel (csrc/conv3s.hip): the 3x3 stride-2 conv_1 of ResNet stages 3 - 5 over SPACE-TO-DEPTH fp16x2 planes.  The last merge of
the previous stage writes the four phase images (h & 1, w & 1) of its block output instead of the row-padded planes, the conv stages
two of them per filter row as contiguous images, and the 1x1 stride-2 shortcut becomes a dense 1x1 over phase image (0, 0).  Only the
summation order inside the three convs changes: every test is the full fixed-geometry model at a small batch, with the family forced
by the plan, against the fp64 oracle and against the same forward with the family switched off (plane_s2d = 0: the gathered kernel)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import rms, rel_rms_err, ensure_lib          # noqa: E402
from oracle.np_oracle import SptAudioGenOracle          # noqa: E402
from spatialaudiogen_amd.weights import variable_specs, init_weights, synth_inputs          # noqa: E402

pytestmark = pytest.mark.gpu

ENC = ['audio', 'video']
# (instantiations of the conv3h family: conv3h_kernel<BM,BN,WM,WN,KC,AR,true>, csrc/conv3s.hip)
S2D_TILES = ['conv3h_kernel<128,128,64,64,1,2,true>', 'conv3h_kernel<128,64,64,32,1,3,true>', 'conv3h_kernel<256,64,64,64,1,3,true>']
CONV1 = ['video_encoder/conv%d_1/conv_1' % st for st in (3, 4, 5)]
SHORTCUT = ['video_encoder/conv%d_1/shortcut' % st for st in (3, 4, 5)]


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    ensure_lib()
    return torch


def is_s2d(kernel):
    return kernel in S2D_TILES


def _u8(T, v):
    return T.round((T.as_tensor(v).double() + 0.5) * 255.0).clamp(0, 255).to(T.uint8)


def check_out(got, ref):
    err = rms(got - ref)
    assert np.isfinite(got).all()
    assert err <= 1e-4, 'abs RMS err %g' % err
    assert err <= 1e-3 * rms(ref), 'rel RMS err %g (out rms %g)' % (err / rms(ref), rms(ref))


@functools.lru_cache(maxsize=None)
def _case(B):
    """Weights, inputs and the oracle's output for the forced-tile cases: computed once per batch size, never modified."""
    P = init_weights(variable_specs(ENC), seed=6, mode='test')
    inp = synth_inputs(B, ENC, seed=31)
    return P, inp, SptAudioGenOracle(encoders=ENC).inference_ops(inp['audio'], P, video=inp['video'])


def force(net, B, tile_name):
    from spatialaudiogen_amd.model import SptAudioGen
    tid = SptAudioGen.tile_names().index(tile_name)
    for name in CONV1:
        net.plan_set(B, name, tid, 1)


def profiled(net, B, *inputs):
    net.profile_enable(B, True)
    out = net.inference_ops(*inputs)
    rows = net.profile_report(B)
    net.profile_enable(B, False)
    return out, rows


def assert_s2d_launches(rows, tile_name):
    """The new kernel on exactly the three conv_1 layers, their shortcuts on the dense form, nothing else changed family."""
    where = sorted(layer for k, layer, _, _ in rows if is_s2d(k))
    assert where == CONV1, where
    for name in CONV1:
        assert [k for k, layer, _, _ in rows if layer == name] == [tile_name], name
    layers = [layer for _, layer, _, _ in rows]
    for name in SHORTCUT:
        dense = [k for k, layer, _, _ in rows if layer == name + '#s2d']
        assert len(dense) == 1 and dense[0].startswith('conv3g_kernel'), (name, dense)
        assert name not in layers, name                    # ... and not a second time in the gathered form


@pytest.mark.parametrize('B', [2, 5])
@pytest.mark.parametrize('tile_name', S2D_TILES)
def test_forced_s2d_tiles_run_the_three_stride2_convs(T, tile_name, B):
    """B = 5: a partly filled last tile, tiles that straddle image boundaries (the row below an image is the next image's first row
    and must read as zero), an odd image count."""
    from spatialaudiogen_amd.model import SptAudioGen
    P, inp, ref = _case(B)
    net = SptAudioGen(1, encoders=ENC, separation='unet_mask')
    net.load_variables(P)
    net.inference_ops(inp['audio'], inp['video'])
    force(net, B, tile_name)
    out, rows = profiled(net, B, inp['audio'], inp['video'])
    assert_s2d_launches(rows, tile_name)
    got = out.cpu().numpy()
    trunk = net.intermediate(B, 'video_encoder/conv5_2').cpu().numpy()
    check_out(got, ref)
    assert net.counter(B, 'fp16x2_saturations') == 0
    # the family switched off: the same plan falls back to the gathered kernel on the row-padded planes
    net.set_option(B, 'plane_s2d', 0)
    out0, rows0 = profiled(net, B, inp['audio'], inp['video'])
    assert not any(is_s2d(k) or layer.endswith('#s2d') for k, layer, _, _ in rows0)
    for name in CONV1 + SHORTCUT:
        ks = [k for k, layer, _, _ in rows0 if layer == name]
        assert len(ks) == 1 and ks[0].startswith('conv3g_kernel'), (name, ks)
    other = out0.cpu().numpy()
    trunk0 = net.intermediate(B, 'video_encoder/conv5_2').cpu().numpy()
    d, dt = rms(got - other), rms(trunk - trunk0)
    print('\n[%s B=%d] rms(s2d - gathered): output %.3g (rms %.3g), conv5_2 %.3g (rms %.3g)' % (tile_name, B, d, rms(other), dt, rms(trunk0)))
    # the project's bar for a re-ordered contraction (test_gpu_model.py: the dh-split against the unsplit run)
    assert d <= 2e-5 * max(rms(other), 1e-9) + 1e-7, d
    net.set_option(B, 'plane_s2d', 1)
    assert T.equal(net.inference_ops(inp['audio'], inp['video']), out)          # back on, run to run


@pytest.mark.parametrize('case', ['tiny', 'huge', 'mixed', 'offset'])
def test_s2d_planes_hold_over_the_range_of_batch_norm_parameters(T, case):
    """The parameter sets of test_fp16x2_trunk_planes_hold_over_the_range_of_batch_norm_parameters with the space-to-depth family
    forced: the plane values are bit-identical to the row-padded ones and only land elsewhere, so nothing saturates and the bars
    hold; the yardstick is the gathered kernel on the same planes' values."""
    from spatialaudiogen_amd.model import SptAudioGen
    B = 3
    P = init_weights(variable_specs(ENC), seed=21, mode='test')
    r = np.random.Generator(np.random.PCG64(3))
    for k in list(P):
        if k.startswith('video_encoder/') and k.endswith('/bn/gamma') and '/conv1/' not in k:
            g, b = P[k].copy(), P[k.replace('gamma', 'beta')].copy()
            if case == 'tiny':
                g *= 1e-3; b *= 1e-3
            elif case == 'huge':
                g *= 300.0; b *= 300.0
            elif case == 'mixed':
                g *= np.exp(r.uniform(np.log(1e-3), np.log(30.0), size=g.shape)).astype(np.float32)
            else:
                b += 40.0
            P[k], P[k.replace('gamma', 'beta')] = g.astype(np.float32), b.astype(np.float32)
    inp = synth_inputs(B, ENC, seed=43)
    orc = SptAudioGenOracle(encoders=ENC)
    ref = orc.inference_ops(inp['audio'], P, video=inp['video'])
    net = SptAudioGen(1, encoders=ENC, separation='unet_mask')
    net.load_variables(P)
    net.inference_ops(inp['audio'], inp['video'])
    force(net, B, S2D_TILES[0])
    out, rows = profiled(net, B, inp['audio'], inp['video'])
    assert_s2d_launches(rows, S2D_TILES[0])
    got = out.cpu().numpy()
    trunk = net.intermediate(B, 'video_encoder/conv5_2').cpu().numpy()
    net.set_option(B, 'plane_s2d', 0)
    other = net.inference_ops(inp['audio'], inp['video']).cpu().numpy()
    trunk0 = net.intermediate(B, 'video_encoder/conv5_2').cpu().numpy()
    tr = orc.ends['video_encoder/conv5_2']
    e2, e0 = rel_rms_err(trunk, tr), rel_rms_err(trunk0, tr)
    o2, o0 = rel_rms_err(got, ref), rel_rms_err(other, ref)
    print('\n[%s] conv5_2 rel err: s2d %.3g, gathered %.3g; output rel err: s2d %.3g, gathered %.3g (output rms %.3g)' % (case, e2, e0, o2, o0, rms(ref)))
    assert np.isfinite(got).all() and np.isfinite(trunk).all()
    assert net.counter(B, 'fp16x2_saturations') == 0
    assert e2 < 1e-4 and o2 < 1e-3, (e2, o2)
    assert e2 <= 1.5 * e0 + 1e-7 and o2 <= 1.5 * o0 + 1e-7, (e2, e0, o2, o0)
    assert rel_rms_err(trunk, trunk0) < 1e-4


def test_grouped_s2d_groups_equal_the_single_forward_bit_for_bit(T):
    """G = 3 batches of 2 per launch, uint8 frames (sagen_forward_grouped_u8, what the benchmark calls), the new tile forced on both
    contexts: every group is the single forward of its batch, bit for bit - the operand pointer is relocated per group."""
    from spatialaudiogen_amd.model import SptAudioGen
    B, G = 2, 3
    P = init_weights(variable_specs(ENC), seed=11, mode='test')
    inp = synth_inputs(G * B, ENC, seed=77)
    for g in range(G):
        inp['audio'][g * B:(g + 1) * B] *= (1.0, 0.37, 1.9)[g]
    a, v = T.as_tensor(inp['audio']).cuda(), _u8(T, inp['video']).cuda()
    one = SptAudioGen(1, encoders=ENC, separation='unet_mask')
    one.load_variables(P)
    grp = SptAudioGen(1, encoders=ENC, separation='unet_mask', groups=G)
    grp.load_variables(P)
    one.inference_ops(a[:B], v[:B])
    grp.inference_ops(a, v)
    for tile_name in S2D_TILES[:2]:
        for net in (one, grp):
            force(net, B, tile_name)
        got, rows = profiled(grp, B, a, v)
        assert_s2d_launches(rows, tile_name)
        want = T.cat([one.inference_ops(a[g * B:(g + 1) * B], v[g * B:(g + 1) * B]) for g in range(G)], 0)
        for g in range(G):
            assert T.equal(got[g * B:(g + 1) * B], want[g * B:(g + 1) * B]), (tile_name, g, float((got - want)[g * B:(g + 1) * B].abs().max()))
    assert grp.counter(B, 'fp16x2_saturations') == 0
    k = (v[B:2 * B].double() / 255.0 - 0.5).float().cpu().numpy()
    ref = SptAudioGenOracle(encoders=ENC).inference_ops(inp['audio'][B:2 * B], P, video=k)
    check_out(got[B:2 * B].cpu().numpy(), ref)


def test_u8_frames_through_the_s2d_family(T):
    """sagen_forward_u8 (the headline's entry point) with the family forced, against the oracle on the frames' float values."""
    from spatialaudiogen_amd.model import SptAudioGen
    B = 3
    P = init_weights(variable_specs(ENC), seed=5, mode='test')
    inp = synth_inputs(B, ENC, seed=19)
    a, v = T.as_tensor(inp['audio']).cuda(), _u8(T, inp['video']).cuda()
    ref = SptAudioGenOracle(encoders=ENC).inference_ops(inp['audio'], P, video=(v.double() / 255.0 - 0.5).float().cpu().numpy())
    net = SptAudioGen(1, encoders=ENC, separation='unet_mask')
    net.load_variables(P)
    net.inference_ops(a, v)
    force(net, B, S2D_TILES[1])
    out, rows = profiled(net, B, a, v)
    assert_s2d_launches(rows, S2D_TILES[1])
    assert any(k.startswith('stem8') for k, _, _, _ in rows)
    check_out(out.cpu().numpy(), ref)


def test_autotune_times_both_families_and_its_plan_replays(T):
    """While tuning the merge writes both layouts, so the space-to-depth tiles and conv3g_kernel's are timed on real operands and the
    dense shortcut gets its own plan entry; whichever family wins a layer, the tuned forward holds the oracle's bar."""
    from spatialaudiogen_amd.model import SptAudioGen
    B = 2
    P = init_weights(variable_specs(ENC), seed=7, mode='test')
    inp = synth_inputs(B, ENC, seed=23)
    ref = SptAudioGenOracle(encoders=ENC).inference_ops(inp['audio'], P, video=inp['video'])
    net = SptAudioGen(1, encoders=ENC, separation='unet_mask')
    net.load_variables(P)
    plan = {layer: tile for layer, tile, _, _ in net.autotune(inp['audio'], inp['video'])}
    for name in CONV1:
        assert (is_s2d(plan[name]) or plan[name].startswith('conv3g_kernel')), (name, plan[name])
    for name in SHORTCUT:
        assert plan[name].startswith('conv3g_kernel') and plan[name + '#s2d'].startswith('conv3g_kernel'), name
    out, rows = profiled(net, B, inp['audio'], inp['video'])
    for c1, sc in zip(CONV1, SHORTCUT):
        ran = [k for k, layer, _, _ in rows if layer == c1]
        assert ran == [plan[c1]], (c1, ran)
        want_layer = sc + '#s2d' if is_s2d(plan[c1]) else sc
        assert [layer for _, layer, _, _ in rows if layer.startswith(sc)] == [want_layer]
    check_out(out.cpu().numpy(), ref)


def test_training_context_falls_back_from_a_forced_s2d_tile(T):
    """The training step keeps the gathered path (its trunk retains activations and is not the lean one): a plan that names the new
    tile falls back to the heuristic, and the step is the unforced step bit for bit."""
    from spatialaudiogen_amd.model import SptAudioGen
    from spatialaudiogen_amd.train import Trainer
    B = 2
    P = init_weights(variable_specs(ENC), seed=1, mode='test')
    inp = synth_inputs(B, ENC, seed=99)
    tgt = (inp['audio'][:, 24000:28800, :] * np.array([0.5, 0.25, -0.5], np.float32)).astype(np.float32)
    net = SptAudioGen(1, encoders=ENC, separation='unet_mask')
    net.load_variables(P)
    tr = Trainer(net, batch=B)
    keys = ('video_encoder/conv3_1/conv_1/weights', 'video_encoder/conv5_1/shortcut/weights', 'audio_encoder/conv1/weights')
    loss0 = float(tr.forward_backward(inp['audio'], inp['video'], None, tgt, update_moving=False))
    g0 = {k: tr.grad(k).clone() for k in keys}
    tid = SptAudioGen.tile_names().index(S2D_TILES[0])
    for name in CONV1:
        tr.plan_set(name, tid, 1)
    tr.profile_enable(True)
    loss1 = float(tr.forward_backward(inp['audio'], inp['video'], None, tgt, update_moving=False))
    rows = tr.profile_report()
    tr.profile_enable(False)
    assert not any(is_s2d(k) or layer.endswith('#s2d') for k, layer, _, _ in rows)
    assert abs(loss1 - loss0) <= 1e-12 * abs(loss0), (loss1, loss0)         # (the loss is an fp64 sum by atomics: its last bit depends on their order)
    for k in keys:
        assert T.equal(tr.grad(k), g0[k]), k
