"""Cost of the optical flow estimator on the device (csrc/flow.hip), with device events after warm-up, and of the same call on the
CPU twin (csrc_cpu/sagen_cpu.cpp: the same header in plain loops, one thread) on the same host.

The call measured is what the flow command line makes per block: FlowEstimator.process of 64 frames of 224 x 448 with the frame
before them, i.e. 64 frame pairs, at the defaults (levels 5, warps 3, iters 30, alpha 8, wrap).  It is measured at the fusion depth
the library chooses (fuse 0) and at forced depths; fuse 1 - one Jacobi sweep per launch - is the yardstick for the fused sweep.

    python tools/flow_rate.py [--reps 5] [--regions 3] [--fuse 0 1 2 3 4 6 8] [--no-twin] [--out profiles/flow_rate.jsonl]

One JSON line per depth is printed and appended to --out: the depth the launches ran at (`depth`: what fuse 0 resolved to, from
sagen_flow_auto_fuse), pairs/s and ms per call (median / min / max over the regions), and the share of the call spent in Jacobi
launches.  That share comes from a second measurement at twice the iterations: every other launch (luma, pyramid, smoothing,
upsampling, warp + derivatives, the store) is the same in both, so the difference is the cost of `iters` sweeps per warp, and
share = (t(2 iters) - t(iters)) / t(iters), from the medians; `jacobi_share_range` is the same from the extremes of both
measurements, and `jacobi_share_ok` is false when the median share left [0, 1], i.e. when noise made it meaningless.  The twin runs
in a child process (the library is chosen at import) on 2 pairs: one call to warm up, then 3 timed ones; its pairs/s is the median
and `twin_ms_per_call` keeps the spread."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, BLOCK = 224, 448, 64


def setup(n, device, fuse=0, iters=30):
    import torch
    from spatialaudiogen_amd import flow as F
    r = np.random.RandomState(5)
    base = r.randint(0, 256, size=(H // 8, (W + 8 * n) // 8 + 1, 3)).astype(np.float64)
    big = np.kron(base, np.ones((8, 8, 1)))                         # blocks of 8 x 8 pixels, moving 3 columns a frame
    frames = np.stack([big[:, 3 * k:3 * k + W] for k in range(n + 1)], 0).astype(np.uint8)
    t = torch.as_tensor(frames).to(device)
    est = F.FlowEstimator(F.FlowParams(iters=iters, fuse=fuse), device=device)
    return lambda: est.process(t[1:], t[0])


def twin_run():
    """(in the child, SAGEN_LIB naming the twin) one JSON line: pairs/s on the host."""
    n = 2
    fn = setup(n, 'cpu')
    fn()                                                            # page faults, the first touch of the scratch
    s = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        s.append(time.perf_counter() - t0)
    print(json.dumps({'pairs_per_s': n / float(np.median(s)), 'pairs': n, 'ms_per_call': [round(1e3 * t, 1) for t in sorted(s)]}))


def measure(fn, reps, regions):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--fuse', type=int, nargs='+', default=[0, 1, 2, 3, 4, 6, 8])
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flow_rate.jsonl'))
    ap.add_argument('--twin-run', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.twin_run:
        return twin_run()
    import torch
    assert torch.cuda.is_available(), 'this tool measures the device: there is none'
    torch.cuda.set_device(0)
    twin = None
    if not args.no_twin:
        from spatialaudiogen_amd import build
        env = dict(os.environ, SAGEN_LIB=build.build_cpu_twin())
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--twin-run'], env=env, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-2000:]
        twin = json.loads(r.stdout.strip().split('\n')[-1])
    from spatialaudiogen_amd import _lib
    auto = int(_lib.lib().sagen_flow_auto_fuse())
    lines = []
    for fuse in args.fuse:
        ms = measure(setup(BLOCK, 'cuda', fuse, 30), args.reps, args.regions)
        ms2 = measure(setup(BLOCK, 'cuda', fuse, 60), args.reps, args.regions)
        med, med2 = float(np.median(ms)), float(np.median(ms2))
        share = (med2 - med) / med
        res = {'what': 'optical_flow', 'frames': '%dx%d' % (H, W), 'pairs_per_call': BLOCK, 'levels': 5, 'warps': 3, 'iters': 30, 'fuse': fuse,
               'depth': fuse if fuse else auto, 'reps': args.reps, 'regions': args.regions,
               'ms_per_call': {'median': round(med, 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3)},
               'pairs_per_s': round(BLOCK / med * 1e3, 1),
               'ms_per_call_at_60_iters': {'median': round(med2, 3), 'min': round(min(ms2), 3), 'max': round(max(ms2), 3)},
               'jacobi_share': round(share, 3),
               'jacobi_share_range': [round((min(ms2) - max(ms)) / max(ms), 3), round((max(ms2) - min(ms)) / min(ms), 3)],
               'jacobi_share_ok': bool(0. <= share <= 1.)}
        if twin is not None:
            res['twin_pairs_per_s'] = round(twin['pairs_per_s'], 3)
            res['twin_ms_per_call'] = twin['ms_per_call']
            res['device_over_twin'] = round(res['pairs_per_s'] / twin['pairs_per_s'], 1)
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
