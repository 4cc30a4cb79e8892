"""Second order (ambi_order 2, reference model.py:242-243) on the host side, no device needed: the variable inventory of the Python
layer and of the native context (sagen_create host-only, as tests/test_abi.py does) agree with the reference's shapes, order 1 is
unchanged, order 3 is refused, and the command lines refuse an order-2 model before doing any work."""
import ctypes as C
import os

import numpy as np
import pytest

from spatialaudiogen_amd.geometry import Geometry
from spatialaudiogen_amd.weights import variable_specs, synth_inputs

ENCODER_SETS = ((1, ['audio']), (3, ['audio', 'video']), (7, ['audio', 'video', 'flow']))
G2 = Geometry(ambi_order=2)


@pytest.fixture(scope='module')
def lib():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _cfg(**kw):
    from spatialaudiogen_amd._lib import SagenConfig
    c = SagenConfig()
    c.batch, c.encoders, c.separation, c.num_sep_tracks, c.n_loc_units = 4, 3, 1, 32, 2
    c.loc_units[0], c.loc_units[1] = 512, 512
    c.ambi_order, c.audio_rate, c.video_rate = 1, 48000, 10
    c.context, c.sample_duration, c.fft_window = 1.0, 0.1, 0.025
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _inventory(lib, h):
    name, ndim, shape = C.c_char_p(), C.c_int32(), (C.c_int64 * 4)()
    got = {}
    for i in range(lib.sagen_num_variables(h)):
        assert lib.sagen_variable_spec(h, i, C.byref(name), C.byref(ndim), shape) == 0
        got[name.value.decode()] = tuple(shape[k] for k in range(ndim.value))
    return got


def test_geometry_channel_counts():
    assert (G2.num_in, G2.num_out) == (4, 5)
    assert (Geometry().num_in, Geometry().num_out) == (1, 3)


@pytest.mark.parametrize('nsep', [16, 32, 64])
@pytest.mark.parametrize('enc', [e for _, e in ENCODER_SETS])
def test_order2_specs_match_the_reference_shapes(enc, nsep):
    s = variable_specs(enc, 'unet_mask', nsep, geom=G2)
    assert s['audio_encoder/conv1/weights'] == (7, 16, 4, 32)
    assert s['separation/deconv1/weights'] == (7, 16, 4 * nsep, 64)
    assert s['separation/deconv1/biases'] == (4 * nsep,)
    assert s['localization/fc3/weights'] == (512, 20 * (nsep + 1))
    assert s['localization/fc3/biases'] == (20 * (nsep + 1),)
    # everything that does not depend on the channel counts is the order-1 inventory
    s1 = variable_specs(enc, 'unet_mask', nsep)
    changed = {'audio_encoder/conv1/weights', 'separation/deconv1/weights', 'separation/deconv1/biases',
               'localization/fc3/weights', 'localization/fc3/biases'}
    assert list(s) == list(s1)
    assert {k: v for k, v in s.items() if k not in changed} == {k: v for k, v in s1.items() if k not in changed}


@pytest.mark.parametrize('nsep', [16, 32, 64])
def test_order1_specs_unchanged(nsep):
    s = variable_specs(['audio', 'video'], 'unet_mask', nsep)
    assert s['audio_encoder/conv1/weights'] == (7, 16, 1, 32)
    assert s['separation/deconv1/weights'] == (7, 16, nsep, 64)
    assert s['localization/fc3/weights'] == (512, 3 * (nsep + 1))
    n = variable_specs(['audio'], 'none', 1)
    assert n['localization/fc3/weights'] == (512, 6)


def test_order2_none_separation_specs():
    s = variable_specs(['audio'], 'none', 1, geom=G2)
    assert s['audio_encoder/conv1/weights'] == (7, 16, 4, 32)
    assert s['localization/fc3/weights'] == (512, 5 * 4 * 2)
    assert not any(k.startswith('separation/') for k in s)


def test_synth_inputs_channels():
    a2 = synth_inputs(2, ['audio'], seed=3, geom=G2)['audio']
    assert a2.shape == (2, G2.snd_size, 4) and a2.dtype == np.float32
    assert all(np.std(a2[:, :, i]) > 0.05 for i in range(4))
    assert not np.array_equal(a2[:, :, 0], a2[:, :, 1])
    a1 = synth_inputs(2, ['audio'], seed=3)['audio']
    assert a1.shape == (2, G2.snd_size, 1)
    np.testing.assert_array_equal(a1[:, :, 0], a2[:, :, 0])        # (the first channel draws what order 1 draws)


@pytest.mark.parametrize('sep,nsep', [(1, 16), (1, 32), (1, 64), (0, 1)])
@pytest.mark.parametrize('enc_mask,enc', ENCODER_SETS)
def test_native_inventory_at_order2(lib, enc_mask, enc, sep, nsep):
    h = C.c_void_p()
    assert lib.sagen_create(C.byref(h), C.byref(_cfg(encoders=enc_mask, separation=sep, num_sep_tracks=nsep, ambi_order=2))) == 0, \
        lib.sagen_last_error()
    try:
        specs = variable_specs(enc, 'unet_mask' if sep else 'none', nsep, geom=G2)
        assert _inventory(lib, h) == {k: tuple(v) for k, v in specs.items()}
        assert lib.sagen_workspace_bytes(h) > 4 * sum(int(np.prod(v)) for v in specs.values())
    finally:
        lib.sagen_destroy(h)


def test_native_order2_workspace_holds_the_wider_tensors(lib):
    """The mask buffer alone grows by num_in: 23 rows x 1024 bins x 4 * 32 channels per window."""
    sizes = {}
    for order in (1, 2):
        h = C.c_void_p()
        assert lib.sagen_create(C.byref(h), C.byref(_cfg(ambi_order=order, batch=8))) == 0
        sizes[order] = lib.sagen_workspace_bytes(h)
        lib.sagen_destroy(h)
    assert sizes[2] - sizes[1] >= 8 * 23 * 1024 * 3 * 32 * 4


def test_order3_is_refused(lib):
    h = C.c_void_p()
    assert lib.sagen_create(C.byref(h), C.byref(_cfg(ambi_order=3))) == -3                # SAGEN_ERR_UNSUPPORTED
    assert b'ambi_order' in lib.sagen_last_error()
    assert lib.sagen_create(C.byref(h), C.byref(_cfg(ambi_order=0))) == -3


def test_grouped_order2_is_accepted_and_none_refused(lib):
    h = C.c_void_p()
    assert lib.sagen_create_grouped(C.byref(h), C.byref(_cfg(ambi_order=2)), 3) == 0, lib.sagen_last_error()
    lib.sagen_destroy(h)
    assert lib.sagen_create_grouped(C.byref(h), C.byref(_cfg(ambi_order=2, separation=0, num_sep_tracks=1)), 3) == -3


def test_hoa_op_entries_refuse_bad_arguments(lib):
    assert lib.sagen_mask_istft_mix_hoa_scratch_bytes(2, 5) == 2 * 23 * 5 * 1024 * 4
    buf = (C.c_float * 16)()
    assert lib.sagen_mask_istft_mix_hoa(None, buf, buf, 2, 32, 4, 5, buf, buf, 1 << 30, None) == -1
    assert lib.sagen_mask_istft_mix_hoa(buf, buf, buf, 2, 32, 9, 7, buf, buf, 1 << 30, None) == -3
    assert lib.sagen_mask_istft_mix_hoa(buf, buf, buf, 2, 32, 4, 5, buf, buf, 16, None) == -5
    assert lib.sagen_eval_scratch_bytes_c(4, 3) == lib.sagen_eval_scratch_bytes(4)
    assert lib.sagen_eval_scratch_bytes_c(4, 5) > lib.sagen_eval_scratch_bytes(4)
    assert lib.sagen_eval_metrics_c(None, buf, 2, 5, buf, buf, buf, 1 << 30, None) == -1


def _params_dir(tmp_path, order):
    d = tmp_path / ('order%d' % order)
    d.mkdir()
    (d / 'train-params.txt').write_text(
        "ambi_order: %d\naudio_rate: 48000\nvideo_rate: 10\ncontext: 1.0\nsample_dur: 0.1\nencoders: ['audio', 'video']\n"
        "separation: unet_mask\nnum_sep_tracks: 32\nloc_units: [512, 512]\n" % order)
    return str(d)


def test_deploy_cli_refuses_order2(tmp_path):
    from spatialaudiogen_amd import deploy
    d = _params_dir(tmp_path, 2)
    with pytest.raises(SystemExit, match='ambi_order 2'):
        deploy.main([d, str(tmp_path / 'nowhere'), '--output_fn', str(tmp_path / 'out.wav')])
    assert not os.path.exists(str(tmp_path / 'out.wav'))


def test_evaluate_cli_refuses_order2(tmp_path):
    from spatialaudiogen_amd import evaluate
    d = _params_dir(tmp_path, 2)
    with pytest.raises(SystemExit, match='ambi_order 2'):
        evaluate.main([d, str(tmp_path / 'no_db')])
    assert not os.path.exists(os.path.join(d, 'eval-detailed.txt'))


def test_train_cli_refuses_order2(tmp_path):
    from spatialaudiogen_amd import train
    d = _params_dir(tmp_path, 2)
    with pytest.raises(SystemExit, match='ambi_order 2'):
        train.main(['synthetic', d, '--resume', '--synthetic'])
    with pytest.raises(SystemExit, match='ambi_order 2'):
        train.main(['synthetic', str(tmp_path / 'fresh'), '--ambi_order', '2', '--synthetic'])
    assert not os.path.exists(str(tmp_path / 'fresh'))


def test_first_order_params_pass_the_cli_check(tmp_path):
    from spatialaudiogen_amd.deploy import load_params, require_first_order
    require_first_order(load_params(_params_dir(tmp_path, 1)).ambi_order, 'deploy')
