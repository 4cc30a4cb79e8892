"""--all_metrics on the device: sagen_eval_mel_env (mel-LSD, envelope distance) and sagen_eval_emd (exact EMD-hat) against the fp64
restatements of tests/metric_oracle.py, and the evaluation driver's 28-column file (eval.py:125-132)."""
import os
import socket

import numpy as np
import pytest

import metric_oracle as mo
from oracle import np_oracle as O
from spatialaudiogen_amd.weights import variable_specs, init_weights
from test_eval_metrics_host import map_pairs
from util import ensure_lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_metrics_v1.npz')


def _signals(C, seed):
    """[16, 4800, C] pred / gt pairs: random, near-identical, silent, one silent side, tones, and one NaN window."""
    rng = np.random.default_rng(seed)
    gt = (rng.standard_normal((16, 4800, C)) * rng.choice([0.01, 0.1, 0.5], (16, 1, C))).astype(np.float32)
    pred = (rng.standard_normal((16, 4800, C)) * 0.1).astype(np.float32)
    pred[1] = gt[1] * (1 + 1e-3 * rng.standard_normal((4800, C)))       # near-identical
    pred[2] = gt[2]                                                      # identical
    pred[3] = 0; gt[3] = 0                                               # silent
    pred[4] = 0                                                          # one side silent
    n = np.arange(4800)[:, None]
    gt[5] = 0.3 * np.sin(2 * np.pi * (10 + np.arange(C)) * n / 4800)     # tones
    pred[5] = 0.2 * np.sin(2 * np.pi * (10 + np.arange(C)) * n / 4800 + 0.5)
    pred[6, 100, 0] = np.nan
    return pred.astype(np.float32), gt.astype(np.float32)


@pytest.mark.parametrize('C', [3, 5])
def test_mel_env_against_fp64(C):
    import torch
    ensure_lib()
    from spatialaudiogen_amd import ops
    pred, gt = _signals(C, seed=C)
    p, g = torch.as_tensor(pred).cuda(), torch.as_tensor(gt).cuda()
    mel, env = (x.cpu().numpy() for x in ops.eval_mel_env(p, g))
    mel2, env2 = (x.cpu().numpy() for x in ops.eval_mel_env(p, g))
    assert np.array_equal(mel, mel2, equal_nan=True) and np.array_equal(env, env2, equal_nan=True)    # bit-identical reruns
    assert mel.shape == (16, C) and env.shape == (16, C)
    for b in range(16):
        if b == 6:
            assert np.isnan(mel[b, 0]) and np.isnan(env[b, 0]) and np.isfinite(mel[b, 1:]).all()
            continue
        ref_mel = mo.mel_lsd(pred[b].astype(np.float64), gt[b].astype(np.float64))
        ref_env = mo.env_mse(pred[b], gt[b])
        sig = np.sqrt(np.mean(gt[b].astype(np.float64) ** 2 + pred[b].astype(np.float64) ** 2, 0))
        assert np.all(np.abs(env[b] - ref_env) <= 1e-4 * ref_env + 1e-6 * sig + 1e-12), (b, env[b], ref_env)
        assert np.all(np.abs(mel[b] - ref_mel) <= 1e-4 * np.maximum(1.0, ref_mel)), (b, mel[b], ref_mel)
    # identical windows: the envelope path treats pred and gt alike (exact 0); the mel path splits ONE complex FFT of pred + i gt,
    # which leaves rounding of the order of 1e-6 dB
    assert np.all(env[2] == 0) and np.all(mel[2] < 1e-5)
    assert np.all(mel[3] == 0) and np.all(env[3] == 0)


def test_emd_against_the_lp():
    import torch
    ensure_lib()
    from spatialaudiogen_amd import ops
    from spatialaudiogen_amd.ambisonics import angular_distance
    Cm, _, _ = mo.angular_distance_ref(30.0)
    P, Q = map_pairs(64, seed=11)
    P[9, 3] = np.nan
    cost = torch.as_tensor(angular_distance(30.0), dtype=torch.float64).cuda()
    nc = torch.zeros(1, dtype=torch.int32).cuda()
    p, q = torch.as_tensor(P).cuda(), torch.as_tensor(Q).cuda()
    got = ops.eval_emd(p, q, cost, nc).cpu().numpy()
    again = ops.eval_emd(p, q, cost, nc).cpu().numpy()
    assert int(nc.item()) == 0
    assert np.array_equal(got, again, equal_nan=True)
    assert np.isnan(got[9]).all()
    for k in range(64):
        if k == 9:
            continue
        # the reference's way: flipud maps with the unflipped mesh (eval.py:147-149 + distance.py:100-130)
        ref = mo.emd_pair(P[k].reshape(7, 12)[::-1], Q[k].reshape(7, 12)[::-1], Cm)
        for v in range(2):
            assert abs(got[k, v] - ref[v]) <= 1e-7 * abs(ref[v]) + 1e-12, (k, v, got[k, v], ref[v])
    zero = ops.eval_emd(torch.zeros(2, 84).cuda(), torch.zeros(2, 84).cuda(), cost).cpu().numpy()
    assert np.all(zero == 0)


def test_pinned_against_librosa_and_pyemd():
    """tools/eval_metrics_pin.py records seeded inputs and the values of librosa 0.6.0 / scipy / pyemd 0.5.1 on a machine that has
    them; without that file the device values are checked against the formulas only (test_mel_env_against_fp64, test_emd_...)."""
    if not os.path.exists(GOLDEN):
        pytest.skip('eval metrics UNPINNED against librosa 0.6.0 / pyemd 0.5.1 (tests/golden/eval_metrics_v1.npz absent: '
                    'run tools/eval_metrics_pin.py where those libraries are installed)')
    import torch
    ensure_lib()
    from spatialaudiogen_amd import ops
    from spatialaudiogen_amd.ambisonics import angular_distance
    z = np.load(GOLDEN)
    mel, env = (x.cpu().numpy() for x in ops.eval_mel_env(torch.as_tensor(z['pred']).cuda(), torch.as_tensor(z['gt']).cuda()))
    assert np.allclose(mel, z['mel_lsd'], rtol=1e-3, atol=1e-4) and np.allclose(env, z['env_mse'], rtol=1e-3, atol=1e-7)
    cost = torch.as_tensor(angular_distance(30.0), dtype=torch.float64).cuda()
    maps_p = np.ascontiguousarray(z['map_pred'][:, ::-1].reshape(len(z['map_pred']), -1))     # back from eval.py's flipud
    maps_g = np.ascontiguousarray(z['map_gt'][:, ::-1].reshape(len(z['map_gt']), -1))
    emd = ops.eval_emd(torch.as_tensor(maps_p).cuda(), torch.as_tensor(maps_g).cuda(), cost).cpu().numpy()
    assert np.allclose(emd, z['emd'], rtol=1e-5, atol=1e-9)


# ---- the driver -------------------------------------------------------------------------------------------------------------
def _parse(text):
    lines = text.splitlines()
    keys = lines[0].split(' | ')[1].split()
    rows = [(l.split(' | ')[0], [float(v) for v in l.split(' | ')[1].split()]) for l in lines[1:]]
    return keys, rows


def test_evaluate_all_metrics_matches_fp64(tmp_path):
    import torch
    ensure_lib()
    from test_feeder import make_clip
    from test_gpu_deploy import Params
    from spatialaudiogen_amd import feeder as F
    from spatialaudiogen_amd.evaluate import evaluate, METRIC_KEYS, ALL_METRIC_KEYS
    from spatialaudiogen_amd.deploy import audio_window
    assert torch.cuda.is_available()
    enc = ['audio']
    P = init_weights(variable_specs(enc), seed=9, mode='test')
    db = tmp_path / 'db'; db.mkdir()
    clips = {}
    for i, name in enumerate(['clipA', 'clipB']):
        make_clip(str(db / name), secs=3, seed=20 + i)
        clips[name] = np.concatenate([F.load_wav(os.path.join(str(db / name), 'ambix', '%06d.wav' % k))[0] for k in range(3)], 0)
    (tmp_path / 'layouts.txt').write_text('clipA WXYZ\nclipB WXY\n')
    files = {}
    for flag in (False, True):
        model_dir = tmp_path / ('model%d' % flag); model_dir.mkdir()
        means, count = evaluate(str(model_dir), str(db), None, str(tmp_path / 'layouts.txt'), variables=P, params=Params(enc),
                                partial_batch='pad', power_maps=True, all_metrics=flag)
        files[flag] = open(str(model_dir / 'eval-detailed.txt')).read()
        assert count == 4 and list(means) == (ALL_METRIC_KEYS if flag else METRIC_KEYS)
    keys0, rows0 = _parse(files[False])
    keys1, rows1 = _parse(files[True])
    assert keys0 == METRIC_KEYS and keys1 == ALL_METRIC_KEYS and len(rows1) == 4
    # the 18 old columns: bit-identical to the default run (same text)
    old = [ALL_METRIC_KEYS.index(k) for k in METRIC_KEYS]
    lines0 = files[False].splitlines()[1:]
    lines1 = files[True].splitlines()[1:]
    for l0, l1 in zip(lines0, lines1):
        assert l0.split(' | ')[0] == l1.split(' | ')[0]
        assert l0.split(' | ')[1].split() == [l1.split(' | ')[1].split()[k] for k in old]

    # fp64 restatement on the same 4 windows (zero-padded batch of 16, as the driver ran it)
    amb = np.zeros((16, 52799, 4)); masks = np.ones((16, 4))
    k = 0
    for name in ('clipA', 'clipB'):
        for t in (0.5, 1.5):
            amb[k] = audio_window(clips[name], t, 1.0, 52799, 48000)
            if name == 'clipB':
                masks[k] = [1, 1, 0, 1]
            k += 1
    pred = O.SptAudioGenOracle(encoders=enc).inference_ops(amb[:, :, :1], P)
    target = amb[:, 24000:28800, 1:]
    Cm, _, _ = mo.angular_distance_ref(30.0)
    for i in range(4):
        row = dict(zip(ALL_METRIC_KEYS, rows1[i][1]))
        mel = mo.mel_lsd(pred[i], target[i])
        env = mo.env_mse(pred[i], target[i])
        mono = amb[i, 24000:28800, :1]
        maps = [O.power_map(np.concatenate([mono, x], 1) * masks[i][None, :], 30.0) for x in (pred[i], target[i])]
        emd = mo.emd_pair(maps[0], maps[1], Cm)          # O.power_map returns the flipud map, as eval.py passes it
        ref = {'mel_lsd/avg': mel.mean(), 'mel_lsd/X': mel[2], 'mel_lsd/Y': mel[0], 'mel_lsd/Z': mel[1],
               'env_mse/avg': env.mean(), 'env_mse/X': env[2], 'env_mse/Y': env[0], 'env_mse/Z': env[1],
               'emd/dir': emd[0], 'emd/dir2': emd[1]}
        for key, v in ref.items():
            assert abs(row[key] - v) <= 2e-3 * max(1e-3, abs(v)) + 1e-6, (i, key, row[key], v)


def test_all_metrics_rows_identical_for_ranks_and_groups(tmp_path):
    ensure_lib()
    from test_feeder import make_clip
    from test_gpu_deploy import _run_eval_cli, _write_model_dir
    from spatialaudiogen_amd.evaluate import ALL_METRIC_KEYS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    enc = ['audio']
    P = init_weights(variable_specs(enc), seed=9, mode='test')
    db = tmp_path / 'db'; db.mkdir()
    for i in range(19):                                  # 57 windows = 3 batches + 9 dropped
        make_clip(str(db / ('clip%02d' % i)), secs=4, seed=100 + i, video=False)
    outs = {}
    for tag, world, extra in (('w1', 1, ()), ('w2', 2, ()), ('g2', 1, ('--groups', '2'))):
        model_dir = tmp_path / ('model_' + tag); model_dir.mkdir()
        _write_model_dir(str(model_dir), P, enc)
        s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
        outs[tag] = _run_eval_cli(root, str(model_dir), str(db), world, port, extra=('--all_metrics',) + extra)
    assert outs['w1'][1] == outs['w2'][1] == outs['g2'][1]
    means = lambda log: [l for l in log.splitlines() if l.startswith('EVAL | \t')]
    assert means(outs['w1'][0]) == means(outs['w2'][0]) == means(outs['g2'][0]) and len(means(outs['w1'][0])) == 28
    # the reference's summary (parse_eval_results.py): MSE, STFT, ENV, EMD from the file by column name
    keys, rows = _parse(outs['w1'][1])
    assert keys == ALL_METRIC_KEYS and len(rows) == 48
    vals = np.array([r for _, r in rows])
    summary = [vals[:, keys.index(k)].mean() for k in ('mse/avg', 'stft/avg', 'env_mse/avg', 'emd/dir')]
    assert np.isfinite(summary).all() and summary[2] > 0 and summary[3] > 0
