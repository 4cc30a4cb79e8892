"""Layer-local fp64 checks of the ResNet trunk on fp16x2 planes: conv3h_kernel / conv3hr_kernel (every stride-1 3x3 conv), conv3g_kernel
on fp16x2 planes (the stride-2 conv_1 and the 1x1 projections), the stem8 kernels and the plane-writing passes of csrc/p3.hip, which the
op-level sweeps cannot reach (forward_oracle.NOT_AT_OP_LEVEL) and the model-level tests see only through conv5_2, behind seventeen
convs and batch-norms.

The training step's forward (resnet_train, csrc/model.h) runs these kernels and retains, in fp32, every tensor a layer needs: one step,
then every layer is checked against an fp64 reference computed from the DEVICE'S OWN input of that layer and batch-norm coefficients
formed in fp64 from the DEVICE'S OWN accumulators.  trunk_oracle.py holds the references and derives the bounds;
test_trunk_oracle_host.py proves that the two assertions made here (the elementwise bound, the layer-local rel-RMS < 2e-5) catch a
dropped tap, a dropped plane or cross term, a wrong closing pixel and an unwritten M tail.

Per layer - stem, pool, then per block conv_1, conv_2, merge: finite everywhere (the pure outputs of the forward - y0, t:x0, t:y1:k,
t:y2:k, t:out:k - are filled with NaN before the step; every read and write stays inside the live workspaces), the elementwise
bound, the rel-RMS bar, the accumulators' bound, no fp16x2 saturation, and the kernel that ran, from the profiler rows.  Where planes
are retained: they equal split_planes of the fp32 tensor the same pass wrote BIT FOR BIT, every closing pixel is zero in both planes,
a_inv is a power of two within a factor 2 of the rule of DESIGN.md 3.2 recomputed in fp64, nothing exceeds 65000, and the ReLU bit
mask equals t:out:k > 0.

Cases: uint8 entry (stem8 raw+pool at B = 2 and B = 5 - a partly filled last tile at every stage, images that straddle tiles, an odd
count - and stem8 raw with the pool pass at B = 2); the float entry; both trunk sets with flow; every conv3h / conv3hr tile forced on one stride-1 layer of every stage, every
fp16x2 conv3g tile on the three stride-2 conv_1 and their shortcuts, the dh-split; one child process per switch (SAGEN_TRAIN_KEEP_A1,
SAGEN_NO_H2, SAGEN_FP32_ONLY); and the link to the inference path (lean trunk, space-to-depth tiles, fused stem+pool), which retains
nothing: conv5_2 and the bottleneck against the checked training forward at 2e-5, the project's bar for a re-ordered contraction.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunk_oracle as TO          # noqa: E402
from util import ensure_lib, rel_rms_err          # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ('SAGEN_TRAIN_KEEP_A1', 'SAGEN_NO_H2', 'SAGEN_FP32_ONLY')
H_TILES = ['conv3h_kernel<128,64,64,32,1>', 'conv3h_kernel<128,128,64,64,1>', 'conv3h_kernel<64,64,32,32,1>', 'conv3h_kernel<256,64,64,64,1>',
           'conv3h_kernel<128,64,64,32,2>', 'conv3h_kernel<64,64,32,32,2>', 'conv3h_kernel<64,64,32,32,4>',
           'conv3hr_kernel<256,64,64,64,1>', 'conv3hr_kernel<128,64,64,32,1>', 'conv3hr_kernel<64,64,32,32,2>', 'conv3hr_kernel<128,128,64,64,1>']
G_TILES = ['conv3g_kernel<128,64,64,32,3,true>', 'conv3g_kernel<64,64,32,32,4,true>', 'conv3g_kernel<128,128,64,64,2,true>', 'conv3g_kernel<64,128,32,64,3,true>']
# the stride-1 3x3 convs of a stage: every conv3h / conv3hr tile admits all of them (Cin / 16 is a multiple of 4, W >= 8)
STRIDE1 = {2: ['conv2_1/conv_1', 'conv2_1/conv_2', 'conv2_2/conv_1', 'conv2_2/conv_2']}
STRIDE1.update({s: ['conv%d_1/conv_2' % s, 'conv%d_2/conv_1' % s, 'conv%d_2/conv_2' % s] for s in (3, 4, 5)})


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    ensure_lib()
    return torch


def _u8(T, v):
    return T.round((T.as_tensor(v).double() + 0.5) * 255.0).clamp(0, 255).to(T.uint8)


def _h2_kernel(k):
    return k.startswith(('conv3h_kernel', 'conv3hr_kernel')) or (k.startswith('conv3g_kernel') and ',true' in k)


def _step(T, encoders, B, seed, u8, prepare=None):
    """One training step as in test_gpu_backward._setup, the forward's pure outputs prefilled with NaN, under the profiler.
    Returns (tr, P, {scope: frames as the device got them}, profile rows)."""
    from test_gpu_backward import _setup
    from spatialaudiogen_amd.train import Trainer
    net, _, P, inp, target = _setup(T, list(encoders), B, seed)
    tr = Trainer(net, batch=B)
    if prepare:
        prepare(tr)
    video = _u8(T, inp['video']) if u8 else T.as_tensor(inp['video'])
    frames = {'video_encoder': video.cpu().numpy()[:, 0]}
    if 'flow' in encoders:
        frames['flow_encoder'] = np.asarray(inp['flow'], np.float32)[:, 0]
    for sfx in ('', '_b')[:len(frames)]:
        for name in ['y0', 't:x0'] + ['t:%s:%d' % (n, k) for k in range(8) for n in ('y1', 'y2', 'out')]:
            tr.buffer(name + sfx).fill_(float('nan'))
    tr.profile_enable(True)
    loss = tr.forward_backward(inp['audio'], video, inp.get('flow'), target, update_moving=False)
    T.cuda.synchronize()
    rows = tr.profile_report()
    tr.profile_enable(False)
    assert np.isfinite(float(loss))
    return tr, P, frames, rows


def _ran(rows, *layers):
    """The forward's launches under the given layer names, in order (the backward's rows carry a prefix: dgrad:, wgrad:, bnbwd:)."""
    return [k for k, layer, _, _ in rows if layer in layers]


def _check(records, name, kernel, got, ref, bound):
    res = TO.check_layer(got, ref, bound)
    print('%s %s: rel-RMS %.2e, worst element %s at %.3g of its bound' % (name, kernel, res['rel_rms'], res['at'], res['worst']))
    records.append((name, kernel, res['rel_rms'], res['worst']))
    assert res['finite'], ('elements not written', name, kernel)
    assert res['elementwise'], ('elementwise bound', name, kernel, res)
    assert res['rms'], ('layer-local rel-RMS', name, kernel, res)
    return res


def check_trunk(T, tr, P, B, scope, sfx, frames, rows, only=None, a1_written=False, with_stem=True):
    """Every layer of one trunk (only: just these conv layers and, for a projection block, its merge; with_stem = False: from the pooled tensor
    on) against its layer-local reference;
    returns [(layer, kernel, rel-RMS, worst fraction of the bound)]."""
    f32 = lambda name, shape: tr.buffer(name + sfx)[:int(np.prod(shape))].reshape(shape).cpu().numpy()
    try:
        h2a = tr.buffer('t:h2a' + sfx).cpu().numpy()
    except Exception:
        h2a = None                                          # no retained planes (bf16x3 planes / fp32 only)
    bnacc = tr.buffer('bnacc' + sfx).view(T.float64).cpu().numpy()
    acc = lambda li, C: bnacc[li * 1024:li * 1024 + 2 * C]
    var = lambda leaf: np.asarray(P['%s/%s' % (scope, leaf)], np.float64)
    records, full = [], only is None

    def planes(name, shape, v, a_inv, expected, exact):
        """The retained planes `name` of the fp32 tensor v (a reference where the device kept none: exact = False) under a_inv."""
        b, h, w, c = shape
        raw = tr.buffer(name + sfx)[:TO.plane_halfs(b, h, w, c) // 2].view(T.int16).cpu().numpy()
        hi, lo, closing = TO.decode_planes(raw, b, h, w, c)
        assert not closing.view(np.uint16).any(), ('closing pixels not zero', name)
        assert TO.is_pow2(a_inv), (name, a_inv)
        assert float(np.abs(v if exact else v[0]).max()) / a_inv <= 65000.0 and float(np.abs(hi.astype(np.float32)).max()) <= 65000.0, (name, a_inv)
        assert 0.5 <= a_inv / expected <= 2.0, ('scale against the rule of DESIGN.md 3.2', name, a_inv, expected)
        if exact:
            wh, wl = TO.split_planes(v, 1.0 / a_inv)
            assert np.array_equal(hi.view(np.uint16), wh.view(np.uint16)), ('hi plane', name, int((hi.view(np.uint16) != wh.view(np.uint16)).sum()))
            assert np.array_equal(lo.view(np.uint16), wl.view(np.uint16)), ('lo plane', name, int((lo.view(np.uint16) != wl.view(np.uint16)).sum()))
        else:         # the planes of a tensor the device did not keep in fp32: the representation bound around the reference, plus the prologue's
            back = (hi.astype(np.float64) + lo.astype(np.float64)) * a_inv
            tol = np.maximum(2.0 ** -22 * np.abs(v[0]), 2.0 ** -25 * a_inv) + v[1] * (1 + 2.0 ** -20)
            assert (np.abs(back - v[0]) <= tol).all(), ('plane values', name)

    # ---- stem and pool
    stem = scope + '/conv1/conv'
    N0 = B * 112 * 224
    g0, b0 = var('conv1/conv/bn/gamma'), var('conv1/conv/bn/beta')
    sc0, sh0, var0 = TO.bn_coeffs(acc(0, 64), 64, N0, g0, b0)
    tracked = TO.bn_range(var0, N0, g0, b0)                 # (statistical, rigorous) bound of the current block input
    x = f32('t:x0', (B, 56, 112, 64))
    if full and with_stem:
        y0 = f32('y0', (B, 112, 224, 64))
        ks = [k for k in _ran(rows, stem) if 'maxpool' not in k]
        assert len(ks) == 1, ks
        u8 = frames.dtype == np.uint8
        stem8 = ks[0].startswith('stem8pool_kernel')               # (uint8 frames without it: the general stem on the float32 x = u / 255 - 0.5)
        assert u8 or not stem8, (ks, frames.dtype)
        fr = frames if stem8 or not u8 else (frames.astype(np.float64) / 255.0 - 0.5).astype(np.float32)
        _check(records, stem, ks[0], y0, *TO.stem_layer(fr, P[stem + '/weights'], fr.dtype == np.uint8))
        frac = TO.stats_check(acc(0, 64), 64, y0)
        assert frac <= 1.0, ('accumulators', stem, frac)
        kp = _ran(rows, stem + '/bn-relu') or [k for k in _ran(rows, stem) if 'maxpool' in k]
        assert len(kp) == 1 and (kp[0] != 'p3_pack_kernel' or ks[0] == 'stem8pool_kernel<raw+pool>'), (ks, kp)
        _check(records, stem + '/pool', kp[0] + ('(raw+pool)' if kp[0] == 'p3_pack_kernel' else ''), x, *TO.pool_layer(y0, sc0, sh0))
        if h2a is not None:
            planes('t:pl:x:0', (B, 56, 112, 64), x, float(h2a[8]), TO.rule_a_inv(*tracked), True)
        del y0

    # ---- residual blocks
    cin = 64
    for k in range(8):
        st, unit = k // 2, k % 2 + 1
        Ho, Wo, cout = TO.STAGES[st]
        first = unit == 1 and cin != cout
        stride = 2 if first else 1
        pfx = '%s/conv%d_%d' % (scope, st + 2, unit)
        n1, n2, nsc, N = pfx + '/conv_1', pfx + '/conv_2', pfx + '/shortcut', B * Ho * Wo
        want = lambda n: full or n in only
        y1, y2, out = (f32('t:%s:%d' % (n, k), (B, Ho, Wo, cout)) for n in ('y1', 'y2', 'out'))
        g1, b1, g2, b2 = var(n1[len(scope) + 1:] + '/bn/gamma'), var(n1[len(scope) + 1:] + '/bn/beta'), var(n2[len(scope) + 1:] + '/bn/gamma'), var(n2[len(scope) + 1:] + '/bn/beta')
        sc1, sh1, var1 = TO.bn_coeffs(acc(1 + 2 * k, cout), cout, N, g1, b1)
        sc2, sh2, var2 = TO.bn_coeffs(acc(2 + 2 * k, cout), cout, N, g2, b2)
        ax = float(h2a[8 + k]) if h2a is not None else None               # 2^-ka of the block input's planes, of conv_2's input's
        aa = float(h2a[k]) if h2a is not None else None
        if want(n1):
            ks = _ran(rows, n1)
            assert len(ks) >= 1 and (h2a is None) != _h2_kernel(ks[0]), (n1, ks)
            _check(records, n1, '+'.join(ks), y1, *TO.conv_layer(x, P[n1 + '/weights'], stride, 'h2' if _h2_kernel(ks[0]) else 'sweep', ax))
            frac = TO.stats_check(acc(1 + 2 * k, cout), cout, y1)
            assert frac <= 1.0, ('accumulators', n1, frac)
        a1 = f32('t:a1:%d' % k, (B, Ho, Wo, cout)) if a1_written else None
        if full and a1_written:
            _check(records, pfx + '/bn1-relu', '+'.join(_ran(rows, pfx + '/bn1-relu')), a1, *TO.prologue_layer(y1, sc1, sh1))
        if full and h2a is not None:
            planes('t:pl:a1:%d' % k, (B, Ho, Wo, cout), a1 if a1_written else TO.prologue_layer(y1, sc1, sh1), aa,
                   TO.rule_a_inv(*TO.bn_range(var1, N, g1, b1)), a1_written)
        if want(n2):
            ks = _ran(rows, n2, n2 + '#mat')
            assert len(ks) >= 1 and (h2a is None) != _h2_kernel(ks[0]), (n2, ks)
            mode = 'h2' if _h2_kernel(ks[0]) else 'sweep'
            rb = TO.conv_layer(a1, P[n2 + '/weights'], 1, mode, aa) if a1_written else TO.conv_layer(y1, P[n2 + '/weights'], 1, mode, aa, pro=(sc1, sh1))
            _check(records, n2, '+'.join(ks), y2, *rb)
            frac = TO.stats_check(acc(2 + 2 * k, cout), cout, y2)
            assert frac <= 1.0, ('accumulators', n2, frac)
        res_range = tracked
        if first:
            res_range = TO.acc_range(acc(20 + st, cout), cout, N)
        if full or (first and nsc in only):
            ks, res, res_bound = ['identity'], x, 0.0
            if first:
                ks = _ran(rows, nsc)
                assert len(ks) == 1 and (h2a is None) != _h2_kernel(ks[0]), (nsc, ks)
                res, res_bound = TO.conv_layer(x, P[nsc + '/weights'], 2, 'h2' if _h2_kernel(ks[0]) else 'sweep', ax)
                if h2a is not None:                      # (the projection accumulates its statistics only for the fp16 scale of the merge)
                    frac = TO.stats_check(acc(20 + st, cout), cout, res, res_bound)
                    assert frac <= 1.0, ('accumulators', nsc, frac)
            _check(records, pfx + '/merge', '+'.join(_ran(rows, pfx + '/merge')) + ('(shortcut: %s)' % ks[0] if first else ''), out,
                   *TO.merge_layer(y2, sc2, sh2, res, res_bound))
        bn2 = TO.bn_range(var2, N, g2, b2)
        tracked = (bn2[0] + res_range[0], bn2[1] + res_range[1])
        if full and h2a is not None:
            mb = tr.buffer('t:mb:%d%s' % (k, sfx)).view(T.uint8)[:out.size // 8].cpu().numpy()
            assert np.array_equal(mb, np.packbits(out.reshape(-1) > 0, bitorder='little')), ('ReLU bit mask', k)
            assert TO.is_pow2(float(h2a[8 + k + 1])) and 0.5 <= float(h2a[8 + k + 1]) / TO.rule_a_inv(*tracked) <= 2.0, ('merge scale', k, float(h2a[8 + k + 1]), tracked)
            if k < 7:
                planes('t:pl:x:%d' % (k + 1), (B, Ho, Wo, cout), out, float(h2a[8 + k + 1]), TO.rule_a_inv(*tracked), True)
        x, cin = out, cout
    assert tr.ctx.counter('fp16x2_saturations') == 0
    return records


def _summary(tag, records):
    print('[%s] %d layers: worst rel-RMS %.2e (%s), worst fraction of a bound %.3g (%s)' % (
        tag, len(records), max(r[2] for r in records), max(records, key=lambda r: r[2])[0], max(r[3] for r in records), max(records, key=lambda r: r[3])[0]))


# ------------------------------------------------------------------------------------------------------------------------
# 1 - 3: the entries and both trunk sets
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,rawpool', [(2, 1), (5, 1), (2, 0)])
def test_every_layer_uint8_entry(T, B, rawpool):
    """sagen_train_step_u8: the stem8 raw+pool kernel (or, with the context option train_rawpool off, the stem8 raw kernel and
    p3_maxpool_kernel), then every layer on fp16x2 planes."""
    tr, P, frames, rows = _step(T, ('audio', 'video'), B, 3, True, None if rawpool else lambda tr: tr.ctx.set_option('train_rawpool', 0))
    assert tr.last_entry == 'sagen_train_step_u8'
    rec = check_trunk(T, tr, P, B, 'video_encoder', '', frames['video_encoder'], rows)
    assert len(rec) == 2 + 8 * 3 and all(_h2_kernel(r[1]) for r in rec if r[0].endswith(('/conv_1', '/conv_2')))
    assert (rec[0][1], rec[1][1]) == (('stem8pool_kernel<raw+pool>', 'p3_pack_kernel(raw+pool)') if rawpool else ('stem8pool_kernel<raw>', 'p3_maxpool_kernel'))
    _summary('u8 B=%d%s' % (B, '' if rawpool else ' raw stem + pool pass'), rec)


def test_every_layer_float_entry(T):
    """sagen_train_step: the general stem, p3_maxpool_kernel writing t:x0 and the first planes."""
    tr, P, frames, rows = _step(T, ('audio', 'video'), 2, 4, False)
    assert tr.last_entry == 'sagen_train_step'
    rec = check_trunk(T, tr, P, 2, 'video_encoder', '', frames['video_encoder'], rows)
    assert len(rec) == 2 + 8 * 3 and 'p3_maxpool_kernel' in rec[1][1]
    _summary('float B=2', rec)


def test_every_layer_of_both_trunk_sets_with_flow(T):
    tr, P, frames, rows = _step(T, ('audio', 'video', 'flow'), 2, 5, True)
    for scope, sfx in (('video_encoder', ''), ('flow_encoder', '_b')):
        rec = check_trunk(T, tr, P, 2, scope, sfx, frames[scope], rows)
        assert len(rec) == 2 + 8 * 3
        _summary(scope, rec)


# ------------------------------------------------------------------------------------------------------------------------
# 4: forced tiles
# ------------------------------------------------------------------------------------------------------------------------
def _forced(T, plan, seed):
    """plan: {layer below video_encoder/: (tile name, split-K)}; checks exactly these layers and that the forced kernel ran there."""
    from spatialaudiogen_amd.model import SptAudioGen
    names = SptAudioGen.tile_names()
    plan = {'video_encoder/' + k: v for k, v in plan.items()}

    def prepare(tr):
        for layer, (tile, sk) in plan.items():
            tr.plan_set(layer, names.index(tile), sk)
    tr, P, frames, rows = _step(T, ('audio', 'video'), 2, seed, True, prepare)
    for layer, (tile, sk) in plan.items():
        assert _ran(rows, layer) == [tile] + (['splitk_reduce_kernel'] if sk > 1 else []), (layer, _ran(rows, layer))
    return check_trunk(T, tr, P, 2, 'video_encoder', '', frames['video_encoder'], rows, only=set(plan))


@pytest.mark.parametrize('tile', H_TILES)
def test_forced_stride1_tile_on_every_stage(T, tile):
    """Each conv3h_kernel / conv3hr_kernel tile on one stride-1 layer of every stage (the layer rotates with the tile)."""
    i = H_TILES.index(tile)
    layers = [STRIDE1[s][i % len(STRIDE1[s])] for s in (2, 3, 4, 5)]
    rec = _forced(T, {l: (tile, 1) for l in layers}, 6)
    assert [r[0] for r in rec] == ['video_encoder/' + l for l in layers] and all(r[1] == tile for r in rec)
    _summary(tile, rec)


@pytest.mark.parametrize('tile', G_TILES)
def test_forced_gathered_tile_on_the_stride2_layers(T, tile):
    """Each fp16x2 conv3g_kernel tile on the three stride-2 conv_1 and their 1x1 projections (checked through the merge and their statistics)."""
    plan = {'conv%d_1/%s' % (s, n): (tile, 1) for s in (3, 4, 5) for n in ('conv_1', 'shortcut')}
    rec = _forced(T, plan, 7)
    assert [r[0] for r in rec] == ['video_encoder/conv%d_1/%s' % (s, n) for s in (3, 4, 5) for n in ('conv_1', 'merge')]
    assert all(tile in r[1] for r in rec)
    _summary(tile, rec)


def test_forced_dh_split(T):
    """Split-K = 3 by the filter row on stage 5, whose partials fit the split-K scratch: the reducer sums the partials and the statistics."""
    tile = H_TILES[0]
    rec = _forced(T, {l: (tile, 3) for l in STRIDE1[5]}, 8)
    assert len(rec) == 3 and all(r[1] == tile + '+splitk_reduce_kernel' for r in rec)
    _summary(tile + ' dh-split', rec)


# ------------------------------------------------------------------------------------------------------------------------
# 5: the switches, one child process each
# ------------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import test_gpu_trunk_layers as M
sw = sys.argv[1]
M.ensure_lib()
tr, P, frames, rows = M._step(torch, ('audio', 'video'), 2, 9, sw == 'SAGEN_TRAIN_KEEP_A1')
rec = M.check_trunk(torch, tr, P, 2, 'video_encoder', '', frames['video_encoder'], rows, a1_written=True, with_stem=False)      # (the stems have their cases)
convs = [r for r in rec if r[0].endswith(('/conv_1', '/conv_2'))]
assert len(convs) == 16 and len([r for r in rec if r[0].endswith('/bn1-relu')]) == 8
if sw == 'SAGEN_TRAIN_KEEP_A1':
    assert all(M._h2_kernel(r[1]) for r in convs)
else:
    assert not any(M._h2_kernel(r[1]) for r in rec), [r[1] for r in rec]
if sw == 'SAGEN_FP32_ONLY':
    assert all(r[1].startswith('igemm_kernel') for r in convs), [r[1] for r in convs]
M._summary(sw, rec)
print('CHILD OK')
'''
_stopped = []          # why no further child is started: an earlier one did not return 0


@pytest.mark.parametrize('switch', SWITCHES)
def test_layers_under_a_process_switch(T, switch):
    """The switches are read once per process.  SAGEN_TRAIN_KEEP_A1: the fp32 conv_2 input t:a1:k against relu(bn1(y1)), and its planes bit
    for bit; SAGEN_NO_H2: bf16x3 planes; SAGEN_FP32_ONLY: the fp32 kernels - both at the bound of the forward sweeps."""
    assert not _stopped, 'not started: %s' % _stopped[0]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env[switch] = '1'
    cmd = [sys.executable, '-c', CHILD % (ROOT, os.path.join(ROOT, 'tests')), switch]
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _stopped.append('the child of %s ran into its timeout' % switch)
        pytest.fail('%s: timeout\n%s' % (switch, str(e.stdout or '')[-4000:]))
    if r.returncode != 0:
        _stopped.append('the child of %s returned %d' % (switch, r.returncode))
    assert r.returncode == 0, '%s (exit status %d):\n%s\n%s' % (switch, r.returncode, r.stdout[-6000:], r.stderr[-3000:])
    print('\n'.join(l for l in r.stdout.split('\n') if 'of its bound' in l or l.startswith('[')))
    assert 'CHILD OK' in r.stdout


# ------------------------------------------------------------------------------------------------------------------------
# 6: the inference path retains nothing - tie it to the checked one
# ------------------------------------------------------------------------------------------------------------------------
def test_inference_trunk_agrees_with_the_checked_training_forward(T):
    """net.inference_ops (lean trunk, space-to-depth tiles, fused stem + pool) on the inputs and weights of the uint8 case: conv5_2 against
    t:out:7 and the bottleneck likewise, at 2e-5 (the project's bar for a re-ordered contraction)."""
    from test_gpu_backward import _setup
    from spatialaudiogen_amd.train import Trainer
    B = 2
    net, _, P, inp, target = _setup(T, ['audio', 'video'], B, 3)
    video = _u8(T, inp['video']).cuda()
    net.inference_ops(T.as_tensor(inp['audio']).cuda(), video)
    c52 = net.intermediate(B, 'video_encoder/conv5_2').cpu().numpy().reshape(B, 7, 14, 512)
    bott = net.intermediate(B, 'bottleneck').cpu().numpy().reshape(B, 3, -1)
    assert net.counter(B, 'fp16x2_saturations') == 0
    tr = Trainer(net, batch=B)
    tr.forward_backward(inp['audio'], video, None, target, update_moving=False)
    T.cuda.synchronize()
    t52 = tr.buffer('t:out:7')[:B * 7 * 14 * 512].reshape(B, 7, 14, 512).cpu().numpy()
    tb = tr.buffer('bott').cpu().numpy().reshape(B, 3, -1)
    e1, e2 = rel_rms_err(c52, t52), rel_rms_err(bott, tb)
    print('inference against the training forward: conv5_2 rel-RMS %.2e, bottleneck rel-RMS %.2e' % (e1, e2))
    assert np.isfinite(c52).all() and np.isfinite(bott).all()
    assert e1 <= 2e-5 and e2 <= 2e-5, (e1, e2)
