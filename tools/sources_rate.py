"""Rate of the moving-point-source operations on the device (csrc/sources.hip), on seeded signals, trajectories and a seeded HRIR set
(nothing is read from disk).  Three legs, each over 60 s at 48 kHz in one call:

    encode   order 2, S = 4 sources of P = 5 control points           sagen_encode_sources
    mic      S = 4                                                    sagen_binauralize_sources, SAGEN_SOURCES_MIC
    hrir     moving, S = 1, D = 1150 directions, K = 200 taps         sagen_binauralize_sources, SAGEN_SOURCES_HRIR

    python tools/sources_rate.py [--reps 20] [--out profiles/sources_rate.jsonl]      # device events after warm-up, one JSON line per leg
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sources_rate.py --trace-run
    python tools/sources_rate.py --digest DIR                                         # the kernels of that trace, per call

There is no parent implementation to compare with: the lines record samples/s, and for encode the bytes/s the shapes need
((4 S + 4 C) bytes per sample: every signal read once, every output row written once)."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECS, RATE, TRACE_CALLS = 60, 48000, 3


def legs():
    from spatialaudiogen_amd import sources
    from render_rate import seeded_hrirs
    r = np.random.RandomState(7)
    n = SECS * RATE
    sig = [(0.2 * r.normal(size=n)).astype(np.float32) for _ in range(4)]
    cps = [np.stack([r.uniform(-3., 3., 5), r.uniform(-1.4, 1.4, 5), r.uniform(0.8, 3., 5)], 1) for _ in range(4)]
    four, one = sources.SourceScene(sig, cps, RATE), sources.SourceScene(sig[:1], cps[:1], RATE)
    hset = seeded_hrirs()
    return [('encode', dict(order=2, S=4, P=5, channels=9), four, lambda: four.encode(2)),
            ('mic', dict(S=4, P=5), four, lambda: four.binauralize('mic')),
            ('hrir', dict(S=1, P=5, D=hset.directions.shape[0], K=hset.ntaps), one, lambda: one.binauralize('hrir', hset))]


def digest(trace_dir):
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_stats.csv'), recursive=True)
    assert files, 'no kernel_stats.csv under %s' % trace_dir
    rows = list(csv.DictReader(open(files[0])))
    n = SECS * RATE
    out = ['# rocprofv3 --kernel-trace --stats -- python tools/sources_rate.py --trace-run   (1x MI355X)',
           '# %d calls per leg over %d s at %d Hz (%d samples per call): encode order 2 S = 4 P = 5 | mic S = 4 | hrir S = 1 D = 1150 K = 200' % (TRACE_CALLS, SECS, RATE, n),
           '# kernel | calls | total us | mean us | min us | max us | Msamples/s (mean)']
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs'])):
        if 'sources_' not in r['Name']:
            continue
        mean_us = float(r['AverageNs']) * 1e-3
        out.append('%s | %s | %.1f | %.2f | %.2f | %.2f | %.1f' % (r['Name'][:100], r['Calls'], float(r['TotalDurationNs']) * 1e-3, mean_us,
                                                                     float(r['MinNs']) * 1e-3, float(r['MaxNs']) * 1e-3, n / mean_us))
    print('\n'.join(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sources_rate.jsonl'))
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--digest', default=None)
    args = ap.parse_args()
    if args.digest:
        return digest(args.digest)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('sources_rate: no GPU - a rate is measured on the device or not at all')
    torch.cuda.set_device(0)
    lines = []
    for name, shape, scene, fn in legs():
        if args.trace_run:
            for _ in range(TRACE_CALLS):
                y = fn()
            torch.cuda.synchronize()
            print('trace run: %s x %d -> %s' % (name, TRACE_CALLS, tuple(y.shape)))
            continue
        for _ in range(3):                    # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / args.reps * 1e3
        n = scene.length
        line = dict(leg=name, samples=n, audio_s=round(n / float(RATE), 3), reps=args.reps, us_per_call=round(us, 1),
                    msamples_per_s=round(n / us, 1), times_real_time=round(n / float(RATE) / (us * 1e-6), 0), **shape)
        if name == 'encode':
            line['shape_bytes_per_sample'] = 4 * shape['S'] + 4 * shape['channels']
            line['gb_per_s'] = round(n * line['shape_bytes_per_sample'] / us * 1e-3, 1)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if lines:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
