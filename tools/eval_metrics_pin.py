"""Pin the device's eval metrics to the libraries the reference uses.  Run on a machine with librosa 0.6.0, pyemd 0.5.1 and scipy:

    python tools/eval_metrics_pin.py tests/golden/eval_metrics_v1.npz

Writes seeded inputs and those libraries' values, which tests/test_gpu_eval_metrics.py::test_pinned_against_librosa_and_pyemd then
compares the device against:
    pred, gt [16, 4800, 3] fp32 (Y, Z, X)          mel_lsd, env_mse [16, 3]  (myutils.py:96-116 calls, made here directly)
    map_pred, map_gt [16, 7, 12] fp32, flipud as eval.py:147-149 hands them on    emd [16, 2] = (dir, dir2)  (distance.py:100-130)
The maps are synthetic non-negative fields on the 30 degree mesh; the EMD calls use the reference's mesh and arccos cost.
Only numpy / scipy / librosa / pyemd are needed (no GPU, nothing from this package)."""
import sys

import numpy as np


def main(out):
    import librosa
    import pyemd
    from scipy.signal import hilbert
    assert librosa.__version__ == '0.6.0', librosa.__version__
    rng = np.random.default_rng(20240601)
    gt = (rng.standard_normal((16, 4800, 3)) * rng.choice([0.01, 0.1, 0.5], (16, 1, 3))).astype(np.float32)
    pred = (gt * rng.uniform(0.0, 1.5, (16, 1, 3)) + 0.05 * rng.standard_normal((16, 4800, 3))).astype(np.float32)
    pred[0] = gt[0]
    pred[1] = 0
    mel = np.zeros((16, 3))
    env = np.zeros((16, 3))
    db = lambda s: 10 * np.log10(np.abs(s) + 1e-2)
    for b in range(16):
        for c in range(3):
            sp = librosa.feature.melspectrogram(y=pred[b, :, c], sr=48000, n_mels=128, fmax=12000)
            sg = librosa.feature.melspectrogram(y=gt[b, :, c], sr=48000, n_mels=128, fmax=12000)
            mel[b, c] = np.sqrt(np.mean((db(sg) - db(sp)) ** 2))
            env[b, c] = np.sqrt(np.mean((np.abs(hilbert(gt[b, :, c])) - np.abs(hilbert(pred[b, :, c]))) ** 2))
    # mesh and ground distance as distance.py:9-13, 101-110 build them
    phi = np.flip(np.arange(-180., 180., 30.)) / 180. * np.pi
    nu = np.arange(-90., 90.1, 30.) / 180. * np.pi
    phi, nu = np.meshgrid(phi, nu)
    u = np.stack((np.cos(nu) * np.cos(phi), np.cos(nu) * np.sin(phi), np.sin(nu)), 0).reshape((3, -1))
    cost = np.arccos(np.clip(u.T @ u, -1, 1))
    map_pred = (rng.random((16, 7, 12)) ** 3).astype(np.float32)
    map_gt = (rng.random((16, 7, 12)) ** 3 * rng.uniform(0.2, 2.0, (16, 1, 1))).astype(np.float32)
    map_gt[0] = map_pred[0]
    map_gt[1] = 0
    emd = np.zeros((16, 2))
    for b in range(16):
        m1, m2 = map_pred[b].reshape(-1), map_gt[b].reshape(-1)
        n = m1.size
        emd[b, 0] = pyemd.emd((m1 / n).astype(np.float64), (m2 / n).astype(np.float64), cost)
        emd[b, 1] = pyemd.emd((m1 / (m1.sum() + 0.01)).astype(np.float64), (m2 / (m2.sum() + 0.01)).astype(np.float64), cost)
    np.savez(out, pred=pred, gt=gt, mel_lsd=mel, env_mse=env, map_pred=map_pred, map_gt=map_gt, emd=emd,
             versions=np.array(['librosa ' + librosa.__version__, 'pyemd ' + getattr(pyemd, '__version__', '?')]))
    print('wrote', out)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
