"""Second order (ambi_order 2) on the HIP path against the fp64 oracle (oracle.np_oracle.SptAudioGenOracle(ambi_order=2)): the W,Y,Z,X
recording [B, snd_size, 4] goes in, the five second-order channels (ACN 4..8) [B, 4800, 5] come out (reference model.py:242-243,
326-333, 428-430).  Bars as for order 1: output RMS error <= 1e-4 absolute and <= 1e-3 relative to the output RMS."""
import ctypes as C

import numpy as np
import pytest

from util import rms, rel_rms_err, ensure_lib, rng
from oracle import np_oracle
from oracle.np_oracle import SptAudioGenOracle
from spatialaudiogen_amd.geometry import Geometry
from spatialaudiogen_amd.weights import variable_specs, init_weights, synth_inputs

pytestmark = pytest.mark.gpu

ABS_TOL, REL_TOL = 1e-4, 1e-3
G2 = Geometry(ambi_order=2)


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    ensure_lib()
    return torch


def make_net(enc, sep='unet_mask', nsep=32, groups=1):
    from spatialaudiogen_amd.model import SptAudioGen, SptAudioGenParams
    params = SptAudioGenParams(sep_num_tracks=nsep if sep == 'unet_mask' else 1)
    return SptAudioGen(2, encoders=list(enc), separation=sep, params=params, groups=groups)


def run_pair(T, enc, sep='unet_mask', batch=2, nsep=32, seed=0, u8=False, P=None):
    if P is None:
        P = init_weights(variable_specs(enc, sep, nsep if sep == 'unet_mask' else 1, geom=G2), seed=seed, mode='test')
    inp = synth_inputs(batch, enc, seed=1234 + seed, geom=G2)
    orc = SptAudioGenOracle(ambi_order=2, encoders=enc, separation=sep, sep_num_tracks=nsep if sep == 'unet_mask' else 1)
    ref = orc.inference_ops(inp['audio'], P, video=inp.get('video'), flow=inp.get('flow'))
    net = make_net(enc, sep, nsep)
    net.load_variables(P)
    video = inp.get('video')
    if u8 and video is not None:         # the decoder's frames: synth video is round(img) / 255 - 0.5 exactly
        video = np.round((video.astype(np.float64) + 0.5) * 255.0).astype(np.uint8)
    out = net.inference_ops(inp['audio'], video, inp.get('flow'))
    T.cuda.synchronize()
    return net, orc, out.cpu().numpy(), ref, P, inp


def check_out(got, ref):
    assert got.shape == ref.shape and got.shape[1:] == (4800, 5), (got.shape, ref.shape)
    err = rms(got - ref)
    assert np.isfinite(got).all()
    assert err <= ABS_TOL, 'abs RMS err %g' % err
    assert err <= REL_TOL * rms(ref), 'rel RMS err %g (out rms %g)' % (err / rms(ref), rms(ref))


@pytest.mark.parametrize('enc', [['audio'], ['audio', 'video'], ['audio', 'video', 'flow']])
def test_end_to_end_encoder_sets(T, enc):
    net, orc, got, ref, _, _ = run_pair(T, enc, seed=len(enc))
    check_out(got, ref)
    assert net.counter(2, 'fp16x2_saturations') == 0


@pytest.mark.parametrize('nsep', [16, 64])
def test_end_to_end_track_counts(T, nsep):
    net, orc, got, ref, _, _ = run_pair(T, ['audio'], nsep=nsep, seed=nsep)
    check_out(got, ref)
    assert net.counter(2, 'fp16x2_saturations') == 0


def test_end_to_end_no_separation(T):
    """'none' (model.py:274-280): the decoder's product broadcasts the four audio channels against the single track axis of the
    weights, exactly as the reference's graph (and the oracle) does."""
    net, orc, got, ref, _, inp = run_pair(T, ['audio', 'video'], sep='none', seed=7)
    check_out(got, ref)
    c = orc.ends['localization/coeffs']                                   # [B,3,5,4,2]
    a = inp['audio'].astype(np.float64)[:, 24000:28800, :]
    s = np.arange(4800) // 1600
    direct = c[:, s][..., 0].sum(3) * a.sum(2)[:, :, None] + c[:, s][:, :, :, 0, 1]
    assert rms(got - direct) <= ABS_TOL
    assert net.counter(2, 'fp16x2_saturations') == 0


def test_end_to_end_batch32_uint8_frames(T):
    net, orc, got, ref, _, _ = run_pair(T, ['audio', 'video'], batch=32, seed=11, u8=True)
    check_out(got, ref)
    assert net.counter(32, 'fp16x2_saturations') == 0


def test_intermediates(T):
    net, orc, got, ref, _, _ = run_pair(T, ['audio', 'video'], seed=3)
    B, nsep = 2, 32
    mag = net.intermediate(B, 'mag').cpu().numpy()
    assert mag.shape == (B, 127, 1024, 4)
    assert rel_rms_err(mag, orc.ends['audio_encoder/mag']) < 5e-6
    st = net.intermediate(B, 'stft').cpu().numpy().reshape(B, 4, 28, 513, 2)
    r = orc.ends['stft'][:, :, 89:117, :513]
    assert rel_rms_err(st[..., 0], r.real) < 5e-6 and rel_rms_err(st[..., 1], r.imag) < 5e-6
    co = net.intermediate(B, 'localization/coeffs').cpu().numpy().reshape(B, 3, 5, 4, nsep + 1)
    assert rel_rms_err(co, orc.ends['localization/coeffs']) < 5e-5
    d1 = net.intermediate(B, 'separation/deconv1').cpu().numpy()
    assert d1.shape == (B, 23, 1024, 4 * nsep)
    assert rel_rms_err(d1, orc.ends['separation/deconv1'][:, 44:67]) < 5e-5
    for l in range(1, 6):
        n = 'audio_encoder/conv%d' % l
        g = net.intermediate(B, n).cpu().numpy()
        assert rel_rms_err(g, orc.ends[n]) < 5e-5, n
    check_out(got, ref)


@pytest.mark.parametrize('i,j,o', [(0, 0, 0), (1, 5, 2), (3, 31, 4), (2, 17, 1)])
def test_index_known_answer(T, i, j, o):
    """Coefficients that route exactly one (input channel i, track j) to output o: the last localisation FC has zero weights and its
    biases ARE the coefficients (to the rounding of the FC's contraction).  Every other output column is its bias of input channel 0;
    the biases of input channels 1..3 (set large) never show up."""
    nsep = 32
    enc = ['audio']
    P = init_weights(variable_specs(enc, 'unet_mask', nsep, geom=G2), seed=40 + i, mode='test')
    P['localization/fc3/weights'][:] = 0.0
    cf = np.zeros((5, 4, nsep + 1), np.float32)
    cf[o, i, j] = 1.0
    bias0 = np.array([0.1, -0.2, 0.3, -0.4, 0.5], np.float32)
    cf[:, 0, nsep] = bias0
    cf[:, 1:, nsep] = 100.0                          # ignored by the reference (biases[:, :, :, 0], model.py:430)
    P['localization/fc3/biases'][:] = cf.reshape(-1)
    net, orc, got, ref, _, inp = run_pair(T, enc, nsep=nsep, seed=40 + i, P=P)
    check_out(got, ref)
    for oo in range(5):
        if oo != o:
            assert np.abs(got[:, :, oo] - bias0[oo]).max() < 1e-6, (oo, np.abs(got[:, :, oo] - bias0[oo]).max())
    sig = got[:, :, o] - bias0[o]
    assert rms(sig) > 1e-3
    # the routed signal is a masked copy of input channel i: it correlates with that channel far more than with the others
    a = inp['audio'][:, 24000:28800, :].astype(np.float64)
    corr = [abs(np.corrcoef(sig.reshape(-1), a[:, :, c].reshape(-1))[0, 1]) for c in range(4)]
    assert int(np.argmax(corr)) == i, corr


def _oracle_tail(dmask, spec, coeffs, nsep):
    """mask -> istft -> crop -> mix of the oracle (np_oracle.SptAudioGenOracle.separation_ops / inference_ops) on op-level tensors."""
    B = dmask.shape[0]
    x = dmask.astype(np.float64).transpose(0, 3, 1, 2).reshape(B, 4, nsep, 28, 1024)
    half = spec.astype(np.float64)[..., 0] + 1j * spec.astype(np.float64)[..., 1]            # [B,4,28,513]
    full = np.concatenate([half, np.conj(half[..., 1:512][..., ::-1])], -1)                   # Hermitian bins 513..1023
    sep = np_oracle.istft(full[:, :, None] * np_oracle.sigmoid(x), 4)[..., 448:448 + 4800]    # [B,4,nsep,4800]
    w = coeffs.astype(np.float64)[:, np.arange(4800) // 1600]                                 # [B,4800,5,4,nsep+1]
    return np.einsum('bnoij,bijn->bno', w[..., :nsep], sep) + w[:, :, :, 0, nsep]


@pytest.mark.parametrize('nsep', [16, 32, 64])
def test_op_level_mask_istft_mix_hoa(T, nsep):
    from spatialaudiogen_amd import _lib
    from spatialaudiogen_amd._lib import check
    l = ensure_lib()
    B = 2
    r = rng(100 + nsep)
    dmask = r.normal(0, 2, size=(B, 28, 1024, 4 * nsep)).astype(np.float32)
    spec = r.normal(0, 1, size=(B, 4, 28, 513, 2)).astype(np.float32)
    spec[..., 0, 1] = 0.0
    spec[..., 512, 1] = 0.0                          # DC and Nyquist bins of a real frame are real
    coeffs = r.normal(0, 0.2, size=(B, 3, 5, 4, nsep + 1)).astype(np.float32)
    ref = _oracle_tail(dmask, spec, coeffs, nsep)
    dev = lambda a: T.as_tensor(a).cuda()
    d, s, c = dev(dmask), dev(spec), dev(coeffs)
    out = T.empty(B, 4800, 5, device='cuda')
    nb = int(l.sagen_mask_istft_mix_hoa_scratch_bytes(B, 5))
    scratch = T.empty(nb // 4, device='cuda')
    stream = C.c_void_p(T.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(l.sagen_mask_istft_mix_hoa(p(d), p(s), p(c), B, nsep, 4, 5, p(out), p(scratch), nb, stream))
    T.cuda.synchronize()
    got = out.cpu().numpy()
    assert rel_rms_err(got, ref) < 2e-5, rel_rms_err(got, ref)
    assert _lib.lib() is l


def test_grouped_bit_identical_per_batch(T):
    enc = ['audio', 'video']
    P = init_weights(variable_specs(enc, 'unet_mask', 32, geom=G2), seed=5, mode='test')
    inp = synth_inputs(12, enc, seed=77, geom=G2)
    one = make_net(enc)
    one.load_variables(P)
    grp = make_net(enc, groups=3)
    grp.load_variables(P)
    got = grp.inference_ops(inp['audio'], inp['video'])
    want = T.cat([one.inference_ops(inp['audio'][g * 4:g * 4 + 4], inp['video'][g * 4:g * 4 + 4]) for g in range(3)], 0)
    assert got.shape == (12, 4800, 5)
    assert T.equal(got, want), float((got - want).abs().max())
    # and each group against the oracle
    orc = SptAudioGenOracle(ambi_order=2, encoders=enc)
    ref = orc.inference_ops(inp['audio'][4:8], P, video=inp['video'][4:8])
    check_out(got[4:8].cpu().numpy(), ref)


def test_metrics_five_channels(T):
    from spatialaudiogen_amd.model import SptAudioGen
    net = make_net(['audio'])
    B = 4
    r = rng(9)
    tgt = r.normal(0, 0.3, size=(B, 4800, 5)).astype(np.float32)
    pred = (tgt + r.normal(0, 0.1, size=tgt.shape)).astype(np.float32)
    mask = np.ones((B, 5), np.float32)
    mask[1, 3] = 0.0
    m, stft_ps, lsd_ps, mse_ps, snr_ps = net.evaluation_ops(pred, tgt, mask_channels=mask)
    ref_m, r_stft, r_lsd, r_mse, r_snr = np_oracle.evaluation_ops(pred, tgt, mask_channels=mask)
    assert stft_ps.shape == (B, 5)
    assert rel_rms_err(stft_ps.cpu().numpy(), r_stft) < 1e-5
    assert rel_rms_err(mse_ps.cpu().numpy(), r_mse) < 1e-5
    assert np.abs(snr_ps.cpu().numpy() - r_snr).max() < 1e-3
    assert np.abs(lsd_ps.cpu().numpy() - r_lsd).max() < 2e-3 * max(1.0, np.abs(r_lsd).max())
    for k in ('stft/avg', 'lsd/avg', 'mse/avg', 'snr/avg', 'pow/pred', 'pow/gt'):
        assert abs(m[k] - ref_m[k]) <= 2e-3 * max(1.0, abs(ref_m[k])), (k, m[k], ref_m[k])
    assert 'mse/ACN8' in m
    # the first-order entry and the C-channel entry at C = 3 compute the same per-sample values, bit for bit
    from spatialaudiogen_amd._lib import check
    l = ensure_lib()
    t3 = T.as_tensor(tgt[:, :, :3].copy()).cuda()
    p3 = T.as_tensor(pred[:, :, :3].copy()).cuda()
    stream = C.c_void_p(T.cuda.current_stream().cuda_stream)
    nb = int(l.sagen_eval_scratch_bytes(B))
    scratch = T.empty(nb // 4 + 1, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    check(l.sagen_eval_init(p(scratch), nb, B, stream))
    outs = []
    for c_entry in (False, True):
        ps = T.empty(4, B, 3, device='cuda')
        pw = T.zeros(2, dtype=T.float64, device='cuda')
        if c_entry:
            check(l.sagen_eval_metrics_c(p(p3), p(t3), B, 3, p(ps), p(pw), p(scratch), nb, stream))
        else:
            check(l.sagen_eval_metrics(p(p3), p(t3), B, p(ps), p(pw), p(scratch), nb, stream))
        T.cuda.synchronize()
        outs.append((ps.cpu().numpy(), pw.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    np.testing.assert_allclose(outs[0][1], outs[1][1], rtol=1e-12)
    assert SptAudioGen is not None


def test_training_refuses_order2(T):
    from spatialaudiogen_amd._lib import SagenTensor, SagenError, check
    l = ensure_lib()
    enc = ['audio']
    P = init_weights(variable_specs(enc, 'unet_mask', 32, geom=G2), seed=1, mode='test')
    net = make_net(enc)
    net.load_variables(P)
    ctx = net.context_for(2)
    buf = T.zeros(1 << 16, device='cuda')
    g = (SagenTensor * 1)()
    g[0].name, g[0].data, g[0].ndim = b'audio_encoder/conv1/biases', buf.data_ptr(), 1
    g[0].shape[0] = 32
    stream = C.c_void_p(T.cuda.current_stream().cuda_stream)
    with pytest.raises(SagenError, match='ambi_order'):
        check(l.sagen_train_bind(ctx.handle, g, 1, None, 0, C.c_void_p(buf.data_ptr()), buf.numel() * 4, stream))
