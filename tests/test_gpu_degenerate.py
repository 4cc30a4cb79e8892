"""The HIP path on the inputs real clips open and close with (tests/degenerate_cases.py): silence, black / white / constant frames, a
still camera (flow exactly zero), one frame repeated - whole batches, single windows, groups and a deploy of them.

Every forward is held against oracle.torch_ref.TorchRef in fp64.  The bar of a tensor is max(the project's bar, 4 x e32), e32 being
the error of TorchRef in float32 against the fp64 one on the same tensor and input, computed here from the two CPU references only
(degenerate_cases.references): constant frames leave the stem's batch-norm a large common mean over a border-only deviation, and plain
fp32 arithmetic itself misses 1e-4 there (tests/test_degenerate_host.py holds those e32 values where they were measured).

Run with -s for one JSON line per case (profiles/degenerate_inputs.jsonl is that output)."""
import json

import numpy as np
import pytest

import degenerate_cases as D
from degenerate_cases import rms
from util import rel_rms_err, ensure_lib, rng, oracle_window

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    ensure_lib()
    return torch


_REFS, _WEIGHTS, _NETS, _FRESH = {}, {}, {}, {}


def weights(enc):
    if enc not in _WEIGHTS:
        _WEIGHTS[enc] = D.weights(enc)
    return _WEIGHTS[enc]


def refs(name, B):
    """(inputs, out64, ends64, e32_abs, e32_rel) of a case (an encoder tuple for a name: the unmodified batch), computed once and never
    written to.  out64 and e32 are TorchRef's; ends64['bottleneck'] is the numpy oracle's `ends` (the second fp64 implementation, held to
    1e-9 of TorchRef's here as in the host module), so that both references are consulted at every batch size."""
    if (name, B) not in _REFS:
        from oracle.np_oracle import SptAudioGenOracle
        enc = D.CASES[name][1] if name in D.CASES else name
        inp = D.make(name, B) if name in D.CASES else D.random_batch(B, enc)
        out64, ends64, e32, e32_rel = D.references(weights(enc), enc, inp)
        orc = SptAudioGenOracle(encoders=list(enc))
        out = orc.inference_ops(inp['audio'], weights(enc), video=D.frames_float(inp['video']) if 'video' in inp else None, flow=inp.get('flow'))
        bn = np.asarray(orc.ends['bottleneck'], np.float64).reshape(ends64['bottleneck'].shape)
        assert rms(out - out64) <= 1e-9 and rms(bn - ends64['bottleneck']) <= 1e-9 * max(1.0, rms(bn))
        ends64 = dict(ends64, bottleneck=bn)
        _REFS[(name, B)] = (inp, out64, ends64, e32, e32_rel)
    return _REFS[(name, B)]


def new_net(enc, groups=1):
    from spatialaudiogen_amd.model import SptAudioGen
    net = SptAudioGen(1, encoders=list(enc), separation='unet_mask', groups=groups)
    net.load_variables(weights(enc))
    return net


def forward(net, inp):
    return net.inference_ops(inp['audio'], inp.get('video'), inp.get('flow'))


def shared_net(enc, B):
    """One context per (encoders, batch) for all the cases of the table, in whatever order they run: what a FRESH context gave for the
    random batch is kept from its very first forward, and every case afterwards must leave the context giving exactly that again."""
    if (enc, B) not in _NETS:
        net = new_net(enc)
        _FRESH[(enc, B)] = forward(net, D.random_batch(B, enc)).clone()
        _NETS[(enc, B)] = net
    return _NETS[(enc, B)]


def device_ends(net, B, enc):
    names = ['bottleneck', 'localization/coeffs'] + [e + '_encoder/conv5_2' for e in enc[1:]]
    return {n: net.intermediate(B, n).cpu().numpy().astype(np.float64) for n in names}


def hold_bars(tag, name, B, got, ends, ref, report=True):
    """got / ends of the device against the fp64 reference `ref` = refs(name, B), at max(project bar, FACTOR x e32) per tensor"""
    _, out64, ends64, e32, e32_rel = ref
    enc = D.CASES[name][1] if name in D.CASES else name
    err = rms(got - out64)
    rows = {'case': name if isinstance(name, str) else 'random', 'B': B, 'mode': tag, 'out_rms': rms(out64), 'e32': e32, 'err': err}
    checks = [('output abs', err, D.ABS_TOL, e32), ('output rel', err, D.REL_TOL * rms(out64), e32)]
    for n, r in ends64.items():
        if ends is None:
            break
        e = rel_rms_err(ends[n].reshape(r.shape), r)
        proj = D.TRUNK_TOL if n.endswith('conv5_2') else D.BOTTLENECK_TOL if n == 'bottleneck' else D.REL_TOL
        checks.append((n + ' rel', e, proj, e32_rel[n]))
        rows['e32:' + n], rows['err:' + n] = e32_rel[n], e
    if report:
        print('\n' + json.dumps({k: (float('%.3g' % v) if isinstance(v, float) else v) for k, v in rows.items()}))
    assert np.isfinite(got).all()
    for what, e, proj, e32_t in checks:
        if name in D.PROJECT_BAR_HOLDS:          # fp32 is far inside the project's bar there: the project's bar holds unchanged
            assert D.FACTOR * e32_t <= proj, '%s %s: %g x e32 = %.3g would decide the bar (project bar %.3g)' % (name, what, D.FACTOR, D.FACTOR * e32_t, proj)
        assert e <= max(proj, D.FACTOR * e32_t), '%s B=%d [%s] %s: error %.3g, project bar %.3g, e32 %.3g' % (name, B, tag, what, e, proj, e32_t)


@pytest.mark.parametrize('name,B', D.case_ids())
def test_degenerate_batch_against_the_fp64_reference(T, name, B):
    enc = D.CASES[name][1]
    ref = refs(name, B)
    inp = ref[0]
    if B > 5:                # the host module leaves deploy's batch to this one: e32 where it was measured, as there
        assert D.E32_MEASURED[(name, B)] / 3.0 <= ref[3] <= 3.0 * D.E32_MEASURED[(name, B)], (ref[3], D.E32_MEASURED[(name, B)])
    net = shared_net(enc, B)
    sat0 = net.counter(B, 'fp16x2_saturations')
    got_t = forward(net, inp).clone()
    ends = device_ends(net, B, enc)
    got = got_t.cpu().numpy()
    hold_bars('default', name, B, got, ends, ref)
    assert net.counter(B, 'fp16x2_saturations') == sat0 == 0
    assert T.equal(forward(net, inp), got_t)                                          # a second forward: bit-identical
    # no scale, maximum word or statistic of the degenerate batch is left behind: the random batch as a fresh context saw it
    assert T.equal(forward(net, D.random_batch(B, enc)), _FRESH[(enc, B)])
    if name == 'silent':
        # the masked STFT is exactly 0, so the output is the localisation bias term coeffs[..., -1] held for 1600 samples a step
        # (mask_istft / ola_mix on an all-zero spectrum), against the device's own coefficients
        co = ends['localization/coeffs'].reshape(B, 3, 3, 33)
        want = np.repeat(co[..., -1], 1600, axis=1)
        assert want.shape == got.shape and np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()


def test_still_flow_does_not_see_the_flow_stem_filter(T):
    """Flow exactly 0: the flow stem's raw output is exactly 0 whatever its filter holds, its batch-norm gives beta, and nothing behind
    it can depend on the filter - the output is bit-identical with another random filter in its place."""
    B, enc = 2, D.CASES['still'][1]
    inp = refs('still', B)[0]
    net = shared_net(enc, B)
    net.profile_enable(B, True)
    a = forward(net, inp).clone()
    rows = net.profile_report(B)
    net.profile_enable(B, False)
    # the float-frame fast stem (stem8.hip: frame planes scaled by h2_scale_of_bound(batch maximum), here of 0) is what ran on the flow
    assert [k for k, layer, _, _ in rows if layer.startswith('flow_encoder/conv1')].count('stem8pool_kernel<f16>') == 1, rows[:12]
    P = dict(weights(enc))
    w = P['flow_encoder/conv1/conv/weights']
    P['flow_encoder/conv1/conv/weights'] = (rng(5).normal(size=w.shape) * 3.0 * np.std(w)).astype(np.float32)
    assert not np.array_equal(P['flow_encoder/conv1/conv/weights'], w)
    from spatialaudiogen_amd.model import SptAudioGen
    other = SptAudioGen(1, encoders=list(enc), separation='unet_mask')
    other.load_variables(P)
    assert T.equal(forward(other, inp), a)
    rnd = D.random_batch(B, enc)
    assert not T.equal(forward(other, rnd), _FRESH[(enc, B)])                         # (the filter does reach the output otherwise)


def _black_paths(B):
    """black frames through the three entry paths of one context: {path: (output, intermediates)}"""
    enc = D.CASES['black'][1]
    inp = refs('black', B)[0]
    net = new_net(enc)
    f32 = D.frames_float(inp['video'])
    assert np.all(f32 == np.float32(-0.5))
    net.profile_enable(B, True)
    out = {'float': (net.inference_ops(inp['audio'], f32).cpu().numpy(), device_ends(net, B, enc))}
    assert 'stem8pool_kernel<f16>' in {k for k, _, _, _ in net.profile_report(B)}            # float frames: the fp16x2 fast stem
    for fast in (1, 0):
        net.set_option(B, 'u8_fast_stem', fast)
        y = net.inference_ops(inp['audio'], inp['video']).cpu().numpy()
        assert ('stem8pool_kernel<h2>' in {k for k, _, _, _ in net.profile_report(B)}) == bool(fast)
        out['uint8 fast stem' if fast else 'uint8 general stem'] = (y, device_ends(net, B, enc))
    net.profile_enable(B, False)
    assert net.counter(B, 'fp16x2_saturations') == 0
    return out


@pytest.mark.parametrize('B', [2, 5])
def test_black_frames_through_every_entry_point_against_the_fp64_reference(T, B):
    """Black frames as float -0.5 (the fp16x2 fast stem) and as uint8 0 with the one-plane fast stem and with the general stem: each
    path by itself against fp64 at max(project bar, 4 x e32), output and intermediates - the kernels that ran checked by name."""
    ref = refs('black', B)
    for path, (y, ends) in _black_paths(B).items():
        hold_bars(path, 'black', B, y, ends, ref)


# relative RMS of the output between the uint8 and the float entry point on black frames, measured on MI355X
_U8_FLOAT_MEASURED = {(2, 1): 5.41e-5, (2, 0): 3.86e-5, (5, 1): 1.09e-5, (5, 0): 5.21e-5}


@pytest.mark.parametrize('B,fast', [pytest.param(B, fast, marks=pytest.mark.xfail(strict=True, reason=(
    'measured %.3g relative RMS between the uint8 (u8_fast_stem=%d) and the float entry point on black frames at B = %d.  Each path is '
    '3.7e-5 .. 5.6e-5 from fp64 by itself, inside every bar (test_black_frames_through_every_entry_point_against_the_fp64_reference) '
    'and an order better than plain fp32, so two such paths cannot agree to 2e-6.  They differ in their stem kernels only, by float32 '
    'rounding of the raw stem output (uint8 general stem and float general stem are bit-identical); the stem batch-norm divides that '
    'rounding - a shift of the constant interior against the border pixels - by a border-only deviation, and the trunk carries it on '
    '(DESIGN.md, Degenerate inputs)') % (e, fast, B))) for (B, fast), e in _U8_FLOAT_MEASURED.items()])
def test_black_frames_as_uint8_and_as_float_agree_to_rounding(T, B, fast):
    """uint8 0 and float -0.5 are the same frame: the uint8 entry point (one-plane fast stem, and the general kernels) and the float
    entry point are paths of one computation - under 2e-6 relative RMS, the bound test_audio_only_intermediates_and_output sets for
    two such paths.  NOT MET: 5.4e-5 / 3.9e-5 at B = 2 (fast / general uint8 stem), 1.1e-5 / 5.2e-5 at B = 5; the bound is that of
    well-conditioned inputs.  Only this agreement is an expected failure: each path's own accuracy is asserted above."""
    paths = _black_paths(B)
    e = rel_rms_err(paths['uint8 fast stem' if fast else 'uint8 general stem'][0], paths['float'][0])
    print('\nblack B=%d: uint8 (u8_fast_stem=%d) against float frames: %.3g relative RMS' % (B, fast, e))
    assert e < 2e-6, e


@pytest.mark.parametrize('B', [2, 5])
def test_black_frames_on_the_general_kernels_are_one_computation(T, B):
    """What IS one computation stays bit-identical on black frames: the uint8 entry point with the general stem (x / 255 - 0.5 fused into
    the pad pass) and the float entry point with the general float-frame kernels - as test_uint8_video_entry_point holds for noise."""
    enc = D.CASES['black'][1]
    inp = refs('black', B)[0]
    net = new_net(enc)
    net.inference_ops(inp['audio'], inp['video'])
    net.set_option(B, 'f16_fast_stem', 0)
    net.set_option(B, 'u8_fast_stem', 0)
    a = net.inference_ops(inp['audio'], D.frames_float(inp['video']))
    assert T.isfinite(a).all() and T.equal(net.inference_ops(inp['audio'], inp['video']), a)


def test_batch_norm_finalisation_clamps_a_negative_variance(T):
    """A constant channel has variance 0, and E[x^2] - E[x]^2 of sums that carry any rounding lands on either side of it: with the
    squares rounded to float32 before they are summed, a constant of 3e4 misses by up to 6e-8 * 9e8 = 54, far beyond eps = 1e-3 on the
    negative side.  The finalisation clamps the variance at 0 (scale = gamma / sqrt(eps), finite) instead of taking the root of a
    negative number."""
    from spatialaudiogen_amd import ops
    B, H, W = 2, 4, 4
    n = B * H * W
    # (float32 square minus exact square: 0, 0, -0.024, +1.03, -6.25, -0.30, +1.28, -0.94)
    c = np.array([0.0, -0.5, 1000.1, -30000.3, 31234.5, -4567.89, 12345.678, 20001.3], np.float32).astype(np.float64)
    sq = (c.astype(np.float32) * c.astype(np.float32)).astype(np.float64)             # the float32-rounded square of every element
    stats = np.stack([n * c, n * sq])
    var = sq - c * c
    assert np.sum(var < -1e-3) >= 2 and np.sum(var > 1e-3) >= 1                       # beyond eps on both sides, and exactly 0
    r = rng(3)
    gamma, beta = r.uniform(0.5, 1.5, size=8).astype(np.float32), r.normal(size=8).astype(np.float32)
    sc, sh = ops.bn_finalize(T.as_tensor(stats).cuda().contiguous(), (B, H, W, 8), T.as_tensor(gamma).cuda(), T.as_tensor(beta).cuda())
    want_sc = gamma / np.sqrt(np.maximum(var, 0.0) + 1e-3)
    want_sh = beta - c * want_sc
    assert np.isfinite(sc.cpu().numpy()).all() and np.isfinite(sh.cpu().numpy()).all()
    assert rel_rms_err(sc.cpu().numpy(), want_sc) < 1e-6 and rel_rms_err(sh.cpu().numpy(), want_sh) < 1e-6


def test_maxpool_backward_routes_a_tied_window_to_its_first_maximum(T):
    """tf.nn.max_pool's gradient goes to the FIRST maximum of a window in scan order, once.  On an image whose raw values are a few
    integers every window holds exact ties (a constant frame makes all nine elements equal): the gradient at the batch-norm output
    against fp64 autograd, 1e-6 as test_maxpool_backward holds it on tie-free noise.  Crediting every tied element (what the gather did
    before) multiplies the stem's gradient on a black frame."""
    from spatialaudiogen_amd import ops
    from oracle.torch_ref import bn_train, _same
    import torch.nn.functional as F
    r = rng(9)
    for (B, H, W, C) in [(2, 12, 20, 64), (2, 11, 9, 64)]:
        y0 = r.integers(-1, 3, size=(B, H, W, C)).astype(np.float32)
        y0[0, 2:9, 1:8] = 2.0                                                    # a constant patch: nine-fold ties
        gamma, beta = r.uniform(0.5, 1.5, size=C).astype(np.float32), r.normal(0, 0.3, size=C).astype(np.float32)
        gamma[1::4] *= -1.0
        yd = T.as_tensor(y0).cuda()
        stats = T.stack([yd.double().sum((0, 1, 2)), (yd.double() ** 2).sum((0, 1, 2))]).contiguous()
        sc, sh = ops.bn_finalize(stats, (B, H, W, C), T.as_tensor(gamma).cuda(), T.as_tensor(beta).cuda())
        pooled = ops.maxpool3x3s2(yd, sc, sh)
        g = r.normal(size=tuple(pooled.shape)).astype(np.float32)
        z = bn_train(T.as_tensor(y0, dtype=T.float64).permute(0, 3, 1, 2), T.as_tensor(gamma, dtype=T.float64),
                     T.as_tensor(beta, dtype=T.float64)).detach().requires_grad_(True)
        pt, pb = _same(H, 3, 2)
        pl, pr = _same(W, 3, 2)
        p = F.max_pool2d(F.pad(F.relu(z), (pl, pr, pt, pb), value=float('-inf')), 3, 2)
        p.backward(T.as_tensor(g, dtype=T.float64).permute(0, 3, 1, 2))
        want = z.grad.permute(0, 2, 3, 1).numpy()
        dz = ops.maxpool3x3s2_bwd(yd, stats, T.as_tensor(gamma).cuda(), T.as_tensor(beta).cuda(), pooled, T.as_tensor(g).cuda()).cpu().numpy()
        assert rel_rms_err(dz, want) < 1e-6, rel_rms_err(dz, want)


@pytest.mark.parametrize('mode', ['bf16x3', 'general_stem', 'autotuned', 'decoder_planes'])
@pytest.mark.parametrize('name', ['black', 'all', 'one_black'])
def test_degenerate_batch_in_every_arithmetic_mode(T, name, mode):
    """B = 5 on the three-plane bf16 kernels (fp16x2 = 0), on the general uint8 stem (u8_fast_stem = 0), on a plan the tuner made
    while timing its candidates on the degenerate batch itself, and with the decoder on fp16x2 planes scaled by the producers' exact
    maxima (all-zero for a silent batch): the same bars.  The tuned plan must also hold the bar on a random batch."""
    B, enc = 5, D.CASES[name][1]
    ref = refs(name, B)
    inp = ref[0]
    net = new_net(enc)
    if mode == 'autotuned':
        plan = net.autotune(inp['audio'], inp.get('video'), inp.get('flow'))
        assert len([r for r in plan if not r[0].endswith('#materialize')]) >= 30
    else:
        forward(net, inp)
        opt, val = {'bf16x3': ('fp16x2', 0), 'general_stem': ('u8_fast_stem', 0), 'decoder_planes': ('decoder_planes', 1)}[mode]
        net.set_option(B, opt, val)
    got_t = forward(net, inp).clone()
    hold_bars(mode, name, B, got_t.cpu().numpy(), device_ends(net, B, enc), ref)
    assert net.counter(B, 'fp16x2_saturations') == 0
    assert T.equal(forward(net, inp), got_t)
    if mode == 'autotuned':
        rref = refs(enc, B)
        got = forward(net, rref[0])
        hold_bars('autotuned on ' + name, enc, B, got.cpu().numpy(), device_ends(net, B, enc), rref, report=False)


@pytest.mark.parametrize('decoder_planes', [0, 1])
@pytest.mark.parametrize('order', ['random-all-random', 'reversed', 'all-random-all', 'all-all-all'])
def test_a_degenerate_group_among_random_groups(T, order, decoder_planes):
    """G = 3 batches of B = 2 (audio + video, uint8 frames) in one grouped launch per layer, a silent black batch among random ones:
    every group bit-identical to the ungrouped forward of that batch alone.  A scale or maximum word shared across groups - a zero
    bound taken from the degenerate group, or a random group's bound put on it - shows here and nowhere else.  decoder_planes = 1 puts
    the mask decoder on fp16x2 planes scaled by its producers' per-group exact maxima, which small batches do not do by themselves."""
    B, G, enc = 2, 3, D.AV
    rnd = D.random_batch(2 * B, enc)
    r0 = {k: v[:B] for k, v in rnd.items()}
    r2 = {k: v[B:] for k, v in rnd.items()}
    r2['audio'] = r2['audio'] * np.float32(0.37)                   # the random groups differ in scale as well
    deg = {'audio': np.zeros_like(r0['audio']), 'video': np.zeros_like(r0['video'])}
    groups = {'random-all-random': [r0, deg, r2], 'reversed': [r2, deg, r0], 'all-random-all': [deg, r0, deg], 'all-all-all': [deg, deg, deg]}[order]
    one = new_net(enc) if decoder_planes else shared_net(enc, B)
    grp = new_net(enc, groups=G)
    if decoder_planes:
        forward(one, r0)
        forward(grp, {k: np.concatenate([r0[k]] * G, 0) for k in r0})
        one.set_option(B, 'decoder_planes', 1)
        grp.set_option(B, 'decoder_planes', 1)
    want = [forward(one, g).clone() for g in groups]
    if decoder_planes:                                             # (the plane pass really runs at this batch size)
        one.profile_enable(B, True)
        forward(one, deg)
        assert 'h2_pack_rows_kernel' in {k for k, _, _, _ in one.profile_report(B)}
        one.profile_enable(B, False)
    cat ={k: np.concatenate([g[k] for g in groups], 0) for k in ('audio', 'video')}
    got = forward(grp, cat).clone()
    for g in range(G):
        assert T.isfinite(got[g * B:(g + 1) * B]).all()
        assert T.equal(got[g * B:(g + 1) * B], want[g]), (order, g, float((got[g * B:(g + 1) * B] - want[g]).abs().max()))
    assert T.equal(forward(grp, cat), got)
    assert grp.counter(B, 'fp16x2_saturations') == 0
    # the degenerate group's intermediates too, and the degenerate batch against the reference
    grp.set_option(B, 'intermediate_group', 1 if order != 'all-random-all' else 0)
    forward(one, deg)
    for n in ('bottleneck', 'video_encoder/conv5_2'):
        assert T.equal(grp.intermediate(B, n), one.intermediate(B, n)), n


class Params(object):
    ambi_order, audio_rate, video_rate, context, sample_dur = 1, 48000, 10, 1.0, 0.1
    separation, num_sep_tracks, fft_window = 'unet_mask', 32, 0.025
    context_units, freq_mask_units, loc_units = [64, 128, 128], [], [512, 512]

    def __init__(self, encoders):
        self.encoders = encoders


def test_deploy_of_a_clip_that_fades_in_from_silence_and_black(T):
    """A 3 s clip whose first 1.5 s are silent and black, deployed for 1.25 s: one zero-padded batch of 10 whose real windows are all
    partly or wholly degenerate.  Windows cut by the oracle's window table; W a bit-exact copy of the mono crop; Y, Z, X against
    TorchRef fp64 at max(project bar, 4 x e32)."""
    import torch
    from oracle import np_oracle as O
    from oracle.torch_ref import TorchRef
    from spatialaudiogen_amd.deploy import W2XYZ, ClipArrays
    enc, secs = ['audio', 'video'], 3
    r = rng(17)
    audio = (0.3 * r.normal(size=(secs * 48000, 4))).astype(np.float32)
    video = D.frames_float(r.integers(0, 256, size=(secs * 10, 224, 448, 3)).astype(np.uint8))
    audio[:72000] = 0
    video[:15] = np.float32(-0.5)
    P = weights(D.AV)
    got = W2XYZ(params=Params(enc), variables=P).deploy(ClipArrays(audio, video), 0., 1.25)
    rows = O.deploy_window_table(O.audio_pow_times(secs), 0., 1.25)
    assert 0 < len(rows) < 10 and got.shape == (len(rows) * 4800, 4)
    a = np.zeros((10, 52799, 1), np.float32); v = np.zeros((10, 1, 224, 448, 3), np.float32)
    for i, row in enumerate(rows):
        a[i, :, 0] = oracle_window(audio, row)[:, 0]
        v[i, 0] = video[row[3]]
    assert not a[0].any() and np.all(v[0] == np.float32(-0.5))                       # the first window is silent and black
    n = len(rows)
    with D.ref_threads():
        y64 = TorchRef(P, enc, dtype=torch.float64).forward(a, v).numpy()[:n]
        y32 = TorchRef(P, enc, dtype=torch.float32).forward(a, v).numpy()[:n]
    e32 = rms(y32.astype(np.float64) - y64)
    assert np.array_equal(got[:, 0], a[:n, 24000:28800, 0].reshape(-1))              # W
    err = rms(got[:, 1:] - y64.reshape(-1, 3))
    print('\n' + json.dumps({'case': 'deploy_fade_in', 'B': 10, 'mode': 'deploy', 'out_rms': float('%.3g' % rms(y64)), 'e32': float('%.3g' % e32),
                             'err': float('%.3g' % err)}))
    assert np.isfinite(got).all()
    assert err <= max(D.ABS_TOL, D.FACTOR * e32) and err <= max(D.REL_TOL * rms(y64), D.FACTOR * e32), (err, e32, rms(y64))


@pytest.mark.parametrize('case', ['silent_target', 'both_silent', 'prediction_equals_target'])
def test_evaluation_metrics_on_silence_and_on_a_perfect_prediction(T, case):
    """evaluation_ops against the oracle's with the tolerances of test_evaluation_metrics.  The reference returns finite values on all
    three inputs: the SNR carries + 0.1 in numerator and denominator (model.py:104-108), so it is 0 dB when both are silent and
    10 log10((sum t^2 + 0.1) / 0.1), about 35 dB here, when the prediction equals the target - never inf or nan; the log-spectral
    distance has its EPS.  The device must return finite values too."""
    from oracle import np_oracle as O
    from spatialaudiogen_amd.model import SptAudioGen
    B = 3
    r = rng(23)
    x = 0.3 * r.normal(size=(B, 4800, 3))
    if case == 'silent_target':
        gt, pred = np.zeros_like(x), x
    elif case == 'both_silent':
        gt, pred = np.zeros_like(x), np.zeros_like(x)
    else:
        gt, pred = x.astype(np.float32).astype(np.float64), x.astype(np.float32).astype(np.float64)
    mask = np.ones((B, 3)); mask[1, 1] = 0.0
    ref_m, ref_stft, ref_lsd, ref_mse, ref_snr = O.evaluation_ops(pred, gt, mask)
    for ref in (ref_stft, ref_lsd, ref_mse, ref_snr, np.array(list(ref_m.values()))):
        assert np.isfinite(ref).all()                                                # the class of value the reference returns: finite
    if case == 'both_silent':
        assert not ref_stft.any() and not ref_mse.any() and not ref_snr.any() and not ref_lsd.any()
    if case == 'prediction_equals_target':
        assert not ref_mse.any() and np.all(ref_snr > 30.0)
    net = SptAudioGen(1, encoders=['audio'], separation='unet_mask')
    dev = lambda t: T.as_tensor(np.asarray(t, np.float32)).cuda()
    m, stft_ps, lsd_ps, mse_ps, snr_ps = net.evaluation_ops(dev(pred), dev(gt), None, dev(mask))
    got = [t.cpu().numpy() for t in (stft_ps, lsd_ps, mse_ps, snr_ps)]
    for g in got:
        assert np.isfinite(g).all()
    # relative bars as test_evaluation_metrics sets them; where the reference is exactly 0 the device must be 0 to rounding of the sums
    assert rms(got[0] - ref_stft) <= 1e-5 * rms(ref_stft) + 1e-12
    assert rms(got[2] - ref_mse) <= 1e-5 * rms(ref_mse) + 1e-12
    assert np.abs(got[3] - ref_snr).max() < 1e-3
    assert np.abs(got[1] - ref_lsd).max() < 2e-3 * max(1.0, np.abs(ref_lsd).max())
    assert list(m.keys()) == list(ref_m.keys())
    for k in ref_m:
        assert abs(m[k] - ref_m[k]) <= 2e-3 * max(1.0, abs(ref_m[k])), (k, m[k], ref_m[k])


def _train_case(T, name, B=2):
    from spatialaudiogen_amd.train import Trainer
    enc = D.CASES[name][1]
    if name in ('silent_window', 'one_black'):
        enc = D.AV
    inp = dict(D.make(name, B))
    if 'video' in inp:
        inp['video'] = D.frames_float(inp['video'])                                  # the training step takes the feeder's float frames
    target = (0.2 * rng(100).normal(size=(B, 4800, 3))).astype(np.float32)
    mask = np.ones((B, 4), np.float32)
    mask[0, 2] = 0.0
    net = new_net(enc)
    tr = Trainer(net, batch=B)
    loss = tr.forward_backward(inp['audio'], inp.get('video'), inp.get('flow'), target, mask, update_moving=False)
    T.cuda.synchronize()
    return enc, inp, target, mask, net, tr, float(loss)


@pytest.mark.parametrize('name', ['silent_window', 'one_black'])
def test_training_step_gradients_on_a_partly_degenerate_batch(T, name):
    """test_every_variable_gradient_matches_fp64_autograd's configuration and bars (audio + video, B = 2; the loss to 1e-4, every
    variable's gradient to 1e-4 relative RMS, median 3e-5, with the device's ReLU pattern handed to the fp64 autograd; before that the
    oracle's own free-running pattern within 1e-4 of the device's per layer and its free-running gradients within 3e-2; the decoder
    adjoint's two tensors to 1e-4) with one silent window, and with one black frame."""
    from oracle.torch_ref import TorchRef
    from test_gpu_backward import _device_relu_masks, _grad_table, RELU_DISAGREE_BAR, FREE_RUNNING_BAR
    B = 2
    enc, inp, target, mask, net, tr, loss = _train_case(T, name, B)
    dev_masks = _device_relu_masks(tr, net, list(enc), B)
    ref = TorchRef(weights(enc), list(enc), dtype=T.float64)
    # (1) the oracle's OWN forward, no masks handed in: its switching pattern against the device's, and its free-running gradients
    ref.record_masks = True
    loss_free, grads_free, pred_free, _ = ref.loss_and_grads(inp['audio'], inp.get('video'), inp.get('flow'), target, mask[:, 1:])
    ref.record_masks = False
    worst = 0.0
    for key, dm in dev_masks.items():
        own = ref.own_masks[key]
        assert own.shape == dm.shape, (key, own.shape, dm.shape)
        frac = float(np.mean(own != dm))
        worst = max(worst, frac)
        assert frac <= RELU_DISAGREE_BAR, 'ReLU pattern of %s differs from the fp64 forward on %.3g of its %d elements' % (key, frac, dm.size)
    assert rel_rms_err(tr.pred.cpu().numpy(), pred_free) < 1e-3
    assert abs(loss - loss_free) <= 1e-4 * abs(loss_free), (loss, loss_free)
    free_rows = _grad_table(tr, grads_free)
    free_errs = sorted(e for _, e, _ in free_rows)
    free_report = '\n'.join('%-60s err %.2e  rms %.2e' % r_ for r_ in free_rows)
    print('\n[%s] free-running: gradient rel-RMS median %.2e max %.2e' % (name, free_errs[len(free_errs) // 2], free_errs[-1]))
    assert free_errs[-1] <= FREE_RUNNING_BAR and free_errs[len(free_errs) // 2] <= FREE_RUNNING_BAR / 2, free_report
    # (2) the oracle evaluated with the device's switching pattern: the backward itself, at 1e-4
    ref.relu_masks = dev_masks
    loss_ref, grads_ref, pred_ref, ig = ref.loss_and_grads(inp['audio'], inp.get('video'), inp.get('flow'), target, mask[:, 1:],
                                                           keep=('localization/coeffs', 'separation/deconv1'))
    assert rel_rms_err(tr.pred.cpu().numpy(), pred_ref) < 1e-3
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref), (loss, loss_ref)
    # the two tensors the decoder's adjoint produces, before any contraction
    dco = tr.buffer('t:dcoeffs').cpu().numpy().reshape(B, 3, 100)[:, :, :99].reshape(B, 3, 3, 33)
    assert rel_rms_err(dco, ig['localization/coeffs']) < 1e-4, rel_rms_err(dco, ig['localization/coeffs'])
    ddm = tr.buffer('t:ddmask').cpu().numpy().reshape(B, 31, 1024, 32)
    ref_dm = np.transpose(ig['separation/deconv1'], (0, 2, 3, 1))[:, 40:71]
    assert rel_rms_err(ddm, ref_dm) < 1e-4, rel_rms_err(ddm, ref_dm)
    rows = _grad_table(tr, grads_ref)
    errs = sorted(e for _, e, _ in rows)
    report = '\n'.join('%-60s err %.2e  rms %.2e' % r_ for r_ in rows)
    print('\n[%s] ReLU disagreement max %.2e; gradient rel-RMS error: median %.2e  max %.2e (%s)'
          % (name, worst, errs[len(errs) // 2], errs[-1], max(rows, key=lambda t: t[1])[0]))
    assert all(np.isfinite(e) for e in errs) and errs[-1] <= 1e-4, report
    assert errs[len(errs) // 2] <= 3e-5, report


@pytest.mark.parametrize('name', ['black', 'still', 'all'])
def test_training_step_on_a_wholly_degenerate_batch_is_finite(T, name):
    """Constant frames and zero flow leave exact ties in the max-pool windows, and which element of a tie a gradient is routed to is a
    convention, not a value: only the loss is compared (1e-4 relative, the bar of test_every_variable_gradient_matches_fp64_autograd),
    and every gradient must be finite."""
    from oracle.torch_ref import TorchRef, stft_loss_torch
    enc, inp, target, mask, net, tr, loss = _train_case(T, name)
    with D.ref_threads():
        pred = TorchRef(weights(enc), list(enc), dtype=T.float64).forward(inp['audio'], inp.get('video'), inp.get('flow'))
    l64 = float(stft_loss_torch(pred, T.as_tensor(target).double(), T.as_tensor(mask[:, 1:]).double()))
    print('\n[%s] loss %.9g, fp64 reference %.9g (relative %.2e)' % (name, loss, l64, abs(loss - l64) / abs(l64)))
    assert np.isfinite(loss) and abs(loss - l64) <= 1e-4 * abs(l64), (loss, l64)
    for k in tr.opt.layout:
        assert bool(T.isfinite(tr.grad(k)).all()), k
    assert tr.ctx.counter('fp16x2_saturations') == 0
