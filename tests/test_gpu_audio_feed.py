"""The device-side audio feed (csrc/audio_feed.hip through sagen_assemble_audio, feeder.DeviceAudio, deploy --decode device, evaluate
--decode device) against the host feed it stands in for.  The op against explicit numpy, bit for bit (the cases of
tests/audio_feed_cases.py, which tests/test_cpu_twin_audio_feed.py runs through the CPU twin); DeviceAudio against WavPieces.assemble
over ambix folders - bit for bit without a rotation, within 1 ulp of the host's `.dot` and bit for bit the fixed order with one; the
wav of `deploy --decode device` against `--decode host` byte for byte; eval-detailed.txt of evaluate(decode='device') against
decode='host' line for line.

The DeviceAudio cases (HOST_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_audio_feed.py)."""
import os

import numpy as np
import pytest

import audio_feed_cases as AC
from util import ensure_lib, rng

pytestmark = pytest.mark.gpu
HOST_CASES = 'device_audio'


def _device():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    return 'cpu' if _lib.IS_CPU_TWIN else 'cuda'


def _call(samples, lead, read_from, count, rot, size, want, t_off, t_len, offset=0):
    import ctypes as C
    import torch
    from spatialaudiogen_amd import _lib
    from spatialaudiogen_amd.ops import _ptr, _stream
    dev = _device()
    n, channels = samples.shape
    buf = torch.zeros(n * channels + offset, dtype=torch.as_tensor(samples[:0]).dtype, device=dev)
    buf[offset:] = torch.as_tensor(np.ascontiguousarray(samples).reshape(-1)).to(dev)
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dt)).to(dev)
    ld, rf, ct, rt = up(lead, np.int32), up(read_from, np.int64), up(count, np.int32), up(rot, np.float64)
    n_out = len(lead)
    shapes = {'full': (n_out, size, channels), 'mono': (n_out, size), 'target': (n_out, t_len, channels - 1)}
    out = {w: torch.full(shapes[w], float('nan'), dtype=torch.float32, device=dev) for w in want}
    base = C.c_void_p(buf.data_ptr() + offset * buf.element_size()) if n else None
    _lib.check(_lib.lib().sagen_assemble_audio(base, AC.sample_type(samples.dtype), n, channels, _ptr(ld), _ptr(rf), _ptr(ct), _ptr(rt), n_out,
                                               size, t_off, t_len, _ptr(out.get('full')), _ptr(out.get('mono')), _ptr(out.get('target')), _stream()))
    return {w: o.cpu().numpy() for w, o in out.items()}


# ---- the op ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', AC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('channels', AC.CHANNELS)
@pytest.mark.parametrize('size', AC.SIZES)
def test_op_every_window_kind_equals_numpy_bit_for_bit(size, channels, dtype):
    AC.check_shape(_call, size, channels, dtype)


def test_op_more_items_than_the_grid_takes():
    AC.check_grid_strides(_call)


def test_op_a_base_aligned_to_its_element_only():
    AC.check_offset_base(_call)


def test_op_no_samples_is_all_padding():
    AC.check_no_samples(_call)


# ---- DeviceAudio over an ambix folder (HOST_CASES) ----------------------------------------------------------------------------------
@pytest.mark.parametrize('subtype,short_last', [('PCM_16', 0), ('FLOAT', 0), ('PCM_16', 12345)])
def test_device_audio_equals_the_host_feeder_bit_for_bit(tmp_path, subtype, short_last):
    da = AC.check_device_audio_plain(_device(), AC.make_ambix(str(tmp_path / 'ambix'), subtype, short_last))
    assert da.sample_type == (0 if subtype == 'PCM_16' else 1) and da._samples.shape[0] == 3 * AC.RATE


def test_device_audio_rotates_in_the_fixed_order_within_an_ulp_of_the_host(tmp_path):
    AC.check_device_audio_rotated(_device(), AC.make_ambix(str(tmp_path / 'ambix')))


def test_device_audio_refuses_before_a_launch(tmp_path, monkeypatch):
    from spatialaudiogen_amd import feeder as F, _lib
    dev = _device()
    folder = AC.make_ambix(str(tmp_path / 'ambix'))
    da = F.DeviceAudio(folder, AC.RATE, device=dev)
    mono1 = F.DeviceAudio(folder, AC.RATE, ambi_order=0, device=dev)
    assert mono1.num_channels == 1

    def no_launch(*_a, **_k):
        raise AssertionError('the op was called')
    monkeypatch.setattr(_lib.lib(), 'sagen_assemble_audio', no_launch)
    for bad in (np.pi, -3.2, 4.0):
        with pytest.raises(ValueError, match='rotation'):
            da.batch([0.5], AC.CONTEXT, AC.SIZE, rotations=bad)
    with pytest.raises(ValueError):
        da.batch([0.5, 0.6], AC.CONTEXT, AC.SIZE, rotations=[0.1])
    with pytest.raises(ValueError):
        da.batch([0.5, 0.6], AC.CONTEXT, AC.SIZE, pad_to=1)
    with pytest.raises(ValueError):
        da.batch([0.5], AC.CONTEXT, AC.SIZE, want=('mono', 'stereo'))
    with pytest.raises(ValueError):
        da.batch([0.5], AC.CONTEXT, AC.SIZE, want=('target',))                                # no t_off / t_len
    with pytest.raises(ValueError):
        da.batch([0.5], AC.CONTEXT, AC.SIZE, want=('target',), t_off=AC.SIZE - 1, t_len=2)
    with pytest.raises(ValueError):
        mono1.batch([0.5], AC.CONTEXT, AC.SIZE, rotations=0.1)                                # one channel does not rotate
    with pytest.raises(ValueError):
        mono1.batch([0.5], AC.CONTEXT, AC.SIZE, want=('target',), t_off=0, t_len=1)
    with pytest.raises(ValueError, match='Hz'):
        F.DeviceAudio(folder, 44100, device=dev)                                              # nothing is resampled
    short = AC.make_ambix(str(tmp_path / 'short'))
    audio = F.load_wav(os.path.join(short, '000001.wav'))[0]
    F.save_wav(os.path.join(short, '000001.wav'), audio[:-7], AC.RATE)
    with pytest.raises(ValueError, match='last piece'):
        F.DeviceAudio(short, AC.RATE, device=dev)
    with pytest.raises(IOError):
        F.DeviceAudio(str(tmp_path), AC.RATE, device=dev)


# ---- deploy (needs the device) --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clip3(tmp_path_factory):
    from test_feeder import make_clip
    root = str(tmp_path_factory.mktemp('afeed3') / 'clip')
    make_clip(root, secs=3, flow=True)
    return root


@pytest.mark.parametrize('enc', [['audio', 'video'], ['audio', 'video', 'flow']], ids=lambda e: '+'.join(e))
def test_deploy_writes_the_same_wav_either_way(clip3, tmp_path, enc):
    """12 windows of a 3-second clip: a full batch of 10 and a partial one of 2, whose 8 zero windows the op writes (pad_to).  The
    device decode reads no window on the host: AudioReader.assemble is not called."""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import feeder as F
    from spatialaudiogen_amd.deploy import main
    from test_gpu_feed import _model_dir
    model_dir = _model_dir(str(tmp_path / 'model'), enc)
    files, cut = {}, {}
    assemble = F.WavPieces.assemble
    for mode in ('host', 'device'):
        calls = []

        def counted(self, *a, **k):
            calls.append(1)
            return assemble(self, *a, **k)
        F.WavPieces.assemble = counted
        try:
            fn = str(tmp_path / (mode + '.wav'))
            main([model_dir, clip3, '--deploy_duration', '1.7', '--output_fn', fn, '--decode', mode])
        finally:
            F.WavPieces.assemble = assemble
        files[mode], cut[mode] = open(fn, 'rb').read(), len(calls)
    wav, rate = F.load_wav(str(tmp_path / 'host.wav'))
    assert rate == 48000 and wav.shape == (12 * 4800, 4) and np.abs(wav[:, 1:]).max() > 0
    assert files['device'] == files['host']
    assert cut == {'host': 12, 'device': 0}


# ---- evaluate (needs the device) ------------------------------------------------------------------------------------------------------
def _eval_clip(root, secs, seed):
    """A clip folder for evaluate: `secs` wav pieces, the window list, and of the frames only those every 10th window names (5, 15, ...)."""
    from PIL import Image
    from spatialaudiogen_amd import feeder as F
    r = rng(seed)
    for sub in ('ambix', 'video', 'flow'):
        os.makedirs(os.path.join(root, sub))
    audio = np.clip(0.3 * r.normal(size=(secs * 48000, 4)), -1, 1)
    for i in range(secs):
        F.save_wav(os.path.join(root, 'ambix', '%06d.wav' % i), audio[i * 48000:(i + 1) * 48000], 48000)
    with open(os.path.join(root, 'audio_pow.lst'), 'w') as f:
        for i in range((secs - 1) * 10):
            f.write('{} {}\n'.format(i / 10. + 0.5, 0.1 + 0.01 * i))
    for i in range(5, (secs - 1) * 10, 10):
        for sub in ('video', 'flow'):
            fr = (r.integers(0, 256, size=(224, 448, 3)).astype(np.uint8) // 32) * 32
            Image.fromarray(fr).save(os.path.join(root, sub, '%06d.jpg' % i), quality=95)
    np.save(os.path.join(root, 'flow', 'flow_limits.npy'), np.stack([np.linspace(0, 0.5, secs * 10), np.linspace(1, 4, secs * 10)], 1))


@pytest.fixture(scope='module')
def eval_db(tmp_path_factory):
    """clipA 13 s -> 12 windows, clipB 25 s -> 24: the batches are [A x 12 + B x 4], [B x 16] and a partial [B x 4]"""
    db = tmp_path_factory.mktemp('afeed_db')
    _eval_clip(str(db / 'clipA'), 13, 31)
    _eval_clip(str(db / 'clipB'), 25, 32)
    layouts = str(db / 'layouts.txt')
    with open(layouts, 'w') as f:
        f.write('clipA WXYZ\nclipB WXY\n')
    return str(db), layouts


@pytest.mark.parametrize('enc,groups,all_metrics', [(['audio', 'video', 'flow'], 1, False), (['audio', 'video', 'flow'], 2, False),
                                                    (['audio', 'video'], 1, True)])
def test_evaluate_writes_the_same_rows_either_way(eval_db, tmp_path, enc, groups, all_metrics):
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd.evaluate import evaluate
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    from test_gpu_deploy import Params
    db, layouts = eval_db
    P = init_weights(variable_specs(enc), seed=9, mode='test')
    text = {}
    for mode in ('host', 'device'):
        model_dir = tmp_path / mode
        model_dir.mkdir()
        means, count = evaluate(str(model_dir), db, None, layouts, variables=P, params=Params(enc), partial_batch='pad', groups=groups,
                                all_metrics=all_metrics, decode=mode)
        assert count == 36
        text[mode] = open(str(model_dir / 'eval-detailed.txt')).read()
    lines = text['host'].splitlines()
    assert len(lines) == 37 and lines[1].startswith('clipA 0.5 |') and lines[13].startswith('clipB 0.5 |')
    assert text['device'] == text['host']
    with pytest.raises(ValueError):
        evaluate(str(tmp_path), db, None, layouts, variables=P, params=Params(enc), decode='gpu')
