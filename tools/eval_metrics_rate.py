"""Cost of evaluate --all_metrics per batch: device time of the forward alone, the forward + the on-graph metrics, the forward + all
28 columns' metrics (adds sagen_eval_mel_env, two power maps and sagen_eval_emd), for one batch of 16 and for a --groups 10 call
(160 windows), and the host time of tests/metric_oracle.py's fp64 restatements for the same windows on a pool of 16 processes.

    python tools/eval_metrics_rate.py [--reps 20] [--no-host]

Prints one JSON line per configuration (milliseconds per call)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _host_one(args):
    import metric_oracle as mo
    pred, gt, mp, mg, C = args
    return mo.mel_lsd(pred, gt), mo.env_mse(pred, gt), mo.emd_pair(mp[::-1], mg[::-1], C)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    import torch
    from spatialaudiogen_amd import ops
    from spatialaudiogen_amd.model import SptAudioGen
    from spatialaudiogen_amd.weights import variable_specs, init_weights, synth_inputs
    from spatialaudiogen_amd.ambisonics import sh_matrix, angular_distance
    torch.cuda.set_device(0)
    enc = ['audio', 'video']
    P = init_weights(variable_specs(enc), seed=0, mode='test')
    sh = torch.as_tensor(sh_matrix(30.0), dtype=torch.float32).cuda()
    cost = torch.as_tensor(angular_distance(30.0), dtype=torch.float64).cuda()
    nc = torch.zeros(1, dtype=torch.int32).cuda()
    for groups in (1, 10):
        B = 16 * groups
        net = SptAudioGen(1, encoders=enc, separation='unet_mask', groups=groups)
        net.load_variables(P)
        inp = synth_inputs(B, enc, seed=5)
        audio, video = torch.as_tensor(inp['audio']).cuda(), torch.as_tensor(inp['video']).cuda()
        target = (audio[:, 24000:28800, :1] * torch.tensor([0.5, 0.25, -0.5], device='cuda')).contiguous()
        mask = torch.ones(B, 3, device='cuda')
        mono = audio[:, 24000:28800, :1]

        def fwd():
            return net.inference_ops(audio, video)

        def old(pred):
            net.evaluation_ops(pred, target, None, mask)

        def new(pred):
            ops.eval_mel_env(pred, target)
            mp = ops.power_map_batched(torch.cat([mono, pred], 2).contiguous(), sh)
            mg = ops.power_map_batched(torch.cat([mono, target], 2).contiguous(), sh)
            ops.eval_emd(mp, mg, cost, nc)

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.reps

        pred = fwd()
        res = {'groups': groups, 'windows': B,
               'forward_ms': timed(fwd),
               'forward_old_metrics_ms': timed(lambda: old(fwd())),
               'forward_all_metrics_ms': timed(lambda: (lambda p: (old(p), new(p)))(fwd())),
               'new_metrics_only_ms': timed(lambda: new(pred)),
               'mel_env_only_ms': timed(lambda: ops.eval_mel_env(pred, target))}
        assert int(nc.item()) == 0
        if not args.no_host:
            import multiprocessing
            from concurrent.futures import ProcessPoolExecutor
            from spatialaudiogen_amd.ambisonics import angular_distance as ad
            mp = ops.power_map_batched(torch.cat([mono, pred], 2).contiguous(), sh).cpu().numpy().reshape(B, 7, 12)
            mg = ops.power_map_batched(torch.cat([mono, target], 2).contiguous(), sh).cpu().numpy().reshape(B, 7, 12)
            pr, gt = pred.cpu().numpy().astype(np.float64), target.cpu().numpy().astype(np.float64)
            C = ad(30.0)
            jobs = [(pr[b], gt[b], mp[b], mg[b], C) for b in range(B)]
            with ProcessPoolExecutor(16, mp_context=multiprocessing.get_context('spawn')) as ex:     # fresh workers, no GPU
                list(ex.map(_host_one, jobs[:16]))                       # warm the workers
                t0 = time.perf_counter()
                list(ex.map(_host_one, jobs))
                res['host_fp64_16proc_ms'] = (time.perf_counter() - t0) * 1e3
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
