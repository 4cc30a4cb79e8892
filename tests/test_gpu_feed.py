"""The device-side feed (csrc/feed.hip through sagen_assemble_frames, feeder.DeviceFrames, deploy --decode device) against the host feed
it stands in for.  Everything here is an equality of bits: the op against the numpy of JpgFrames.frames / frames_to_float /
FlowFrames.frames (the cases of tests/feed_cases.py, which tests/test_cpu_twin_feed.py runs through the CPU twin), DeviceFrames against
those classes over a clip folder, and the wav of `deploy --decode device` against the wav of `--decode host`, byte for byte.

The op-level and DeviceFrames cases (HOST_CASES) also run against the CPU twin in a container without a GPU (tests/test_feed_host.py)."""
import os

import numpy as np
import pytest

import feed_cases as FC
from util import ensure_lib, rng

pytestmark = pytest.mark.gpu
HOST_CASES = 'op_ or device_frames'


def _device():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    return 'cpu' if _lib.IS_CPU_TWIN else 'cuda'


def _call(frames, index, shift, mode, table, scale_lo):
    import torch
    from spatialaudiogen_amd import _lib
    from spatialaudiogen_amd.ops import _ptr, _stream
    dev = _device()
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dt)).to(dev)
    fr, ix, sh, tb, sl = up(frames, np.uint8), up(index, np.int32), up(shift, np.int32), up(table, np.float32), up(scale_lo, np.float64)
    n_frames, h, w = frames.shape[:3]
    out = torch.full((len(index), h, w, 3), 0xAB, dtype=torch.uint8, device=dev) if mode == 0 else \
        torch.full((len(index), h, w, 3), float('nan'), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().sagen_assemble_frames(_ptr(fr) if n_frames else None, n_frames, h, w, _ptr(ix), _ptr(sh), len(index), mode, _ptr(tb), _ptr(sl),
                                                _ptr(out), _stream()))
    return out.cpu().numpy()


# ---- the op ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', FC.SHAPES)
def test_op_every_mode_equals_the_host_feed_bit_for_bit(h, w):
    FC.check_shape(_call, h, w)


def test_op_no_frames_is_all_padding():
    FC.check_no_frames(_call)


def test_op_any_int32_is_a_shift():
    FC.check_any_int32_shift(_call)


def test_flow_batch_at_the_deploy_frame_size():
    """224 x 448, ten items of four frames (392 workgroups per item, a repeat, padding, rolls either way) in the flow mode"""
    r = rng(7)
    fr = r.integers(0, 256, size=(4, 224, 448, 3)).astype(np.uint8)
    index = np.array([0, 1, 2, 3, 3, -1, 0, 4, 2, 1], np.int32)
    shift = np.array([0, 21, -220, 447, 448, 5, -1, 0, 100000, -100000], np.int32)
    lim = np.stack([np.array([0., 0.5, 2., 0.]), np.array([1., 0.5, 11.5, 4.])], 1)
    FC.same_bits(_call(fr, index, shift, 2, FC.flow_table(), FC.scale_lo_of(lim)), FC.expected(fr, index, shift, 2, lim))


# ---- DeviceFrames over a clip folder ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clip1(tmp_path_factory):
    """make_clip(flow=True, secs=1): ten video and ten flow frames, float64 limits"""
    from test_feeder import make_clip
    root = str(tmp_path_factory.mktemp('feed') / 'clip')
    make_clip(root, secs=1, flow=True)
    return root


class Counting(object):
    """a decoder that notes what it is asked for"""

    def __init__(self, decoder):
        self.decoder, self.device, self.calls = decoder, decoder.device, []

    def decode(self, items):
        self.calls.append([int(os.path.basename(i)[:6]) for i in items])
        return self.decoder.decode(items)


def test_device_frames_equal_the_host_readers(clip1):
    from spatialaudiogen_amd import feeder as F
    from spatialaudiogen_amd.jpeg import JpegDecoder
    dev = _device()
    vdir, fdir = os.path.join(clip1, 'video'), os.path.join(clip1, 'flow')
    host_v, host_f = F.JpgFrames(vdir), F.FlowFrames(fdir, os.path.join(fdir, 'flow_limits.npy'))
    counting = Counting(JpegDecoder(dev))
    dv = F.DeviceFrames(vdir, 'video', device=dev, decoder=counting, block=2)
    df = F.DeviceFrames(fdir, 'flow', device=dev)
    assert (dv.num_frames, dv.duration, dv.frame_shape, dv.rate) == (host_v.num_frames, host_v.duration, host_v.frame_shape, host_v.rate)
    assert (df.num_frames, df.duration, df.rate) == (10, host_f.duration, host_f.rate)
    # ensure decodes what is missing, in calls of at most `block` files, and nothing twice
    dv.ensure(3, 6)
    assert counting.calls == [[3, 4], [5]] and (dv.first, dv.stop) == (3, 6)
    dv.ensure(4, 6)
    dv.ensure(3, 3)
    assert len(counting.calls) == 2
    dv.ensure(2, 7)
    assert counting.calls[2:] == [[2], [6]] and (dv.first, dv.stop) == (2, 7)
    df.ensure(2, 7)
    for rot in (0.3, -3.1, None):
        got = dv.batch(range(2, 7), rot)
        assert got.dtype.is_floating_point is False and tuple(got.shape) == (5, 1, 224, 448, 3) and got.device.type == dev
        want = host_v.frames(2, 5, rot)
        assert np.array_equal(got.cpu().numpy()[:, 0], want)
        FC.same_bits(dv.batch(range(2, 7), rot, as_float=True).cpu().numpy()[:, 0], F.frames_to_float(want))
        FC.same_bits(df.batch(range(2, 7), rot).cpu().numpy()[:, 0], host_f.frames(2, 5, rot))
    assert not np.array_equal(host_v.frames(2, 1, 0.3), host_v.frames(2, 1))                 # the rotations do roll
    # any order, repeats, a rotation per item, padding after normalisation
    got = df.batch([6, 2, 2], [None, -3.1, 0.3], pad_to=5).cpu().numpy()
    want = np.concatenate([host_f.frames(6, 1), host_f.frames(2, 1, -3.1), host_f.frames(2, 1, 0.3), np.zeros((2, 224, 448, 3), np.float32)], 0)
    FC.same_bits(got[:, 0], want)
    got = dv.batch([4], pad_to=3, as_float=True).cpu().numpy()
    FC.same_bits(got[:, 0], np.concatenate([F.frames_to_float(host_v.frames(4, 1)), np.zeros((2, 224, 448, 3), np.float32)], 0))
    assert tuple(dv.batch([]).shape) == (0, 1, 224, 448, 3)
    with pytest.raises(ValueError):
        dv.batch([4], pad_to=3)                                                               # uint8 has no 0.0


def test_device_frames_refuse_before_a_launch(clip1, monkeypatch):
    from spatialaudiogen_amd import feeder as F, _lib
    dev = _device()
    vdir, fdir = os.path.join(clip1, 'video'), os.path.join(clip1, 'flow')
    dv = F.DeviceFrames(vdir, 'video', device=dev)
    dv.ensure(4, 6)

    def no_launch(*_a, **_k):
        raise AssertionError('the op was called')
    monkeypatch.setattr(_lib.lib(), 'sagen_assemble_frames', no_launch)
    for bad in ([3], [4, 6], [-1], [5, 4, 10]):
        with pytest.raises(IndexError):
            dv.batch(bad)
    with pytest.raises(ValueError):
        dv.batch([4, 5], [0.1])
    with pytest.raises(IndexError):
        dv.ensure(8, 11)                                                                      # the folder holds ten
    with pytest.raises(ValueError, match='flow_prep'):
        F.DeviceFrames(fdir, 'flow', device=dev, flow_prep=lambda x: x)
    with pytest.raises(ValueError, match='prep'):
        F.DeviceFrames(vdir, 'video', device=dev, prep=F.img_prep_fcn())
    with pytest.raises(ValueError):
        F.DeviceFrames(vdir, 'audio', device=dev)


def test_device_frames_read_a_float32_limits_file(clip1, tmp_path):
    """flow.write_flow_folder writes flow_limits.npy as float32 [n, 2]: FlowFrames then computes in float32, and so must the device"""
    import shutil
    from spatialaudiogen_amd import feeder as F
    dev = _device()
    fdir = str(tmp_path / 'flow32')
    os.makedirs(fdir)
    for i in range(3):
        shutil.copy(os.path.join(clip1, 'flow', '%06d.jpg' % i), fdir)
    lim = np.array([[0., 1.], [0.0123, 7.77], [2.5, 2.5]], np.float32)
    np.save(os.path.join(fdir, 'flow_limits.npy'), lim)
    host = F.FlowFrames(fdir, os.path.join(fdir, 'flow_limits.npy'))
    assert host.limits.dtype == np.float32
    df = F.DeviceFrames(fdir, 'flow', device=dev)
    df.ensure(0, 3)
    FC.same_bits(df.batch([0, 1, 2], -0.7).cpu().numpy()[:, 0], host.frames(0, 3, -0.7))
    lim64 = lim.astype(np.float64)
    lim64[1, 1] = 7.77                                                                        # a double that is no float32
    np.save(os.path.join(fdir, 'flow_limits.npy'), lim64)
    host = F.FlowFrames(fdir, os.path.join(fdir, 'flow_limits.npy'))
    df = F.DeviceFrames(fdir, 'flow', device=dev)
    df.ensure(1, 2)
    FC.same_bits(df.batch([1]).cpu().numpy()[:, 0], host.frames(1, 1))


# ---- deploy (needs the device) --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clip3(tmp_path_factory):
    from test_feeder import make_clip
    root = str(tmp_path_factory.mktemp('feed3') / 'clip')
    make_clip(root, secs=3, flow=True)
    return root


def _model_dir(root, enc):
    """train-params.txt + a TF tensor bundle assembled by hand, as tests/test_gpu_deploy.py::test_deploy_cli_from_disk builds it"""
    import bundle_by_hand as bh
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    os.makedirs(root)
    bh.write_bundle(os.path.join(root, 'model.ckpt-150000'), dict(init_weights(variable_specs(enc), seed=8, mode='test'), step=np.array(150000, np.int64)))
    with open(os.path.join(root, 'train-params.txt'), 'w') as f:
        f.write("encoders: %r\nseparation: unet_mask\nambi_order: 1\naudio_rate: 48000\nvideo_rate: 10\n"
                "context: 1.0\nsample_dur: 0.1\nnum_sep_tracks: 32\nloc_units: [512, 512]\nfft_window: 0.025\n"
                "context_units: [64, 128, 128]\nfreq_mask_units: []\nlr: 0.0001\nbatch_size: 32\n" % (enc,))
    return root


@pytest.mark.parametrize('enc,duration,groups,windows', [(['audio', 'video'], '1.2', 1, 7), (['audio', 'video', 'flow'], '1.2', 1, 7),
                                                         (['audio', 'video', 'flow'], '10', 2, 20)])
def test_deploy_cli_writes_the_same_wav_either_way(clip3, tmp_path, enc, duration, groups, windows):
    """7 windows: one zero-padded partial batch (float frames); 20 windows with --groups 2: two full batches in one grouped call
    (uint8 video).  Every stage of the device feed is byte-exact, so the files are equal byte for byte."""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd.deploy import main
    model_dir = _model_dir(str(tmp_path / 'model'), enc)
    files = {}
    for mode in ('host', 'device'):
        fn = str(tmp_path / (mode + '.wav'))
        main([model_dir, clip3, '--deploy_duration', duration, '--output_fn', fn, '--decode', mode, '--groups', str(groups)])
        files[mode] = open(fn, 'rb').read()
    from spatialaudiogen_amd.feeder import load_wav
    wav, rate = load_wav(str(tmp_path / 'host.wav'))
    assert rate == 48000 and wav.shape == (windows * 4800, 4) and np.abs(wav[:, 1:]).max() > 0
    assert files['device'] == files['host']


def test_deploy_and_overlay_paints_the_same_frames_either_way(clip3):
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import overlay
    from spatialaudiogen_amd.deploy import W2XYZ
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    from test_gpu_deploy import Params
    enc = ['audio']
    P = init_weights(variable_specs(enc), seed=4, mode='test')
    res = {}
    for mode in ('host', 'device'):
        model = W2XYZ(params=Params(enc), variables=P, decode=mode)
        res[mode] = model.deploy_and_overlay(clip3, 0., 10., overlay.Overlay(4))
    ambi, painted = res['host']
    assert ambi.shape == (20 * 4800, 4) and painted.shape == (15, 224, 448, 3) and painted.dtype == np.uint8
    assert np.array_equal(res['device'][0].view(np.uint32), ambi.view(np.uint32))
    assert np.array_equal(res['device'][1], painted)
    with pytest.raises(ValueError):
        W2XYZ(params=Params(enc), variables=P, decode='gpu')
