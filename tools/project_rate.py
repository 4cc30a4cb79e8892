"""Cost of the frame reprojection on the device (csrc/project.hip), with device events after warm-up, and of the same calls on the
CPU twin (csrc_cpu/sagen_cpu.cpp: the same header in plain loops, one thread) on the same host:

  - eac_to_er     EAC 2160 x 3240 (faces of 1080) -> ER 224 x 448 at the automatic supersampling (8): what turns a 4K EAC clip into
                  the folder deploy reads.  (YouTube's 3840-wide frames have cells of 1280 x 1080; the face table takes square
                  faces, so such a frame is scaled to 3240 columns first.)
  - er_to_view    ER 1080 x 1920 -> view 720 x 1280, hfov 90 degrees, one rotation per frame, S = 1: the head viewport.
  - er_to_er      ER 224 x 448 -> ER 224 x 448, S = 1, one rotation for all frames: the floor - one sample per pixel.

    python tools/project_rate.py [--reps 10] [--regions 3] [--no-twin] [--out profiles/project_rate.jsonl]

One JSON line per conversion is printed and appended to --out: frames/s and ms per call (median / min / max over the regions),
frame bytes/s (all source bytes + all destination bytes of the call over its time: the traffic a perfect cache would leave), tap
bytes/s (12 bytes per sample, what the gathers request), samples/s.  The twin runs in a child process (the library is chosen at
import) on fewer frames; its line carries frames/s only."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (source kind, source size, destination kind, destination size, frames per device call, frames per twin call, rotations)
CASES = {
    'eac_to_er': ('eac', (2160, 3240), 'er', (224, 448), 8, 1, None),
    'er_to_view': ('er', (1080, 1920), 'view', (720, 1280), 8, 1, 'each'),
    'er_to_er': ('er', (224, 448), 'er', (224, 448), 100, 4, 'one'),
}


def setup(name, n, device):
    import torch
    from spatialaudiogen_amd import project as P
    sk, (h, w), dk, size, _, _, rots = CASES[name]
    kinds = {'eac': P.eac3x2, 'er': P.equirect, 'view': lambda: P.perspective(90.)}
    src, dst = kinds[sk](), kinds[dk]()
    S = P.auto_supersample(src, (h, w), dst, size) if name == 'eac_to_er' else 1
    frames = torch.as_tensor(np.random.RandomState(5).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)).to(device)
    rot = None
    if rots == 'each':
        rot = P.view_trajectory(np.linspace(0., 90., n), 10., 5.)
    elif rots == 'one':
        rot = P.view_trajectory(33., 10., 5.)[0]
    rot = None if rot is None else torch.as_tensor(rot).to(device)
    pr = P.Projector(src, dst, size, supersample=S, device=device)
    return (lambda: pr.process(frames, rot)), S, (h, w), size


def twin_run(name):
    """(in the child, SAGEN_LIB naming the twin) one JSON line: frames/s of the case on the host."""
    n = CASES[name][5]
    fn, S, _, _ = setup(name, n, 'cpu')
    fn()
    t0 = time.perf_counter()
    fn()
    print(json.dumps({'frames_per_s': n / (time.perf_counter() - t0), 'frames': n}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'project_rate.jsonl'))
    ap.add_argument('--twin-run', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.twin_run:
        return twin_run(args.twin_run)
    import torch
    assert torch.cuda.is_available(), 'this tool measures the device: there is none'
    torch.cuda.set_device(0)
    lines = []
    for name, (sk, _, dk, _, n, _, _) in CASES.items():
        fn, S, (h, w), (H, W) = setup(name, n, 'cuda')
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.regions):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.reps)
        med = float(np.median(ms))
        frame_bytes, samples = 3. * n * (h * w + H * W), float(n) * H * W * S * S
        res = {'what': name, 'source': '%s %dx%d' % (sk, h, w), 'destination': '%s %dx%d' % (dk, H, W), 'supersample': S, 'frames_per_call': n,
               'reps': args.reps, 'ms_per_call': {'median': round(med, 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)},
               'frames_per_s': round(n / med * 1e3, 1), 'frame_GB_per_s': round(frame_bytes / med * 1e-6, 2),
               'tap_GB_per_s': round(12. * samples / med * 1e-6, 2), 'Gsamples_per_s': round(samples / med * 1e-6, 3)}
        if not args.no_twin:
            from spatialaudiogen_amd import build
            env = dict(os.environ, SAGEN_LIB=build.build_cpu_twin())
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--twin-run', name], env=env, capture_output=True, text=True, timeout=1200)
            assert r.returncode == 0, r.stderr[-2000:]
            twin = json.loads(r.stdout.strip().split('\n')[-1])
            res['twin_frames_per_s'] = round(twin['frames_per_s'], 3)
            res['device_over_twin'] = round(res['frames_per_s'] / twin['frames_per_s'], 1)
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
