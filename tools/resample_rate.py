"""Rate of the polyphase resampler on the device (csrc/resample.hip), with device events after warm-up, and of the same call on
scipy.signal.resample_poly with the same taps in one host thread on the same box.

The calls measured are what the resample command lines make per block: Resampler.process of 480 000 rows of 4 channels in the middle
of a stream (history concatenated in front, the rows the next block needs cloned behind: `process`), and the one launch inside it
(ops.resample_fir on the same rows: `kernel`), for 44.1 -> 48 kHz and 48 -> 16 kHz at both presets.

    python tools/resample_rate.py [--reps 2000] [--regions 3] [--no-scipy] [--out profiles/resample_rate.jsonl]

One JSON line per (ratio, preset) is printed and appended to --out: ms per call (median / min / max over the regions) and
input-seconds per second for both, L, M and the taps per output T; for scipy one call to warm up and three timed ones
(time.perf_counter) on fp64 rows - the same fp64 arithmetic -, the median as the rate and the spread kept.  No rate is promised
anywhere and no test asserts one: the line says which side was faster on the box it ran on."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK, CHANNELS = 480000, 4
CASES = [(44100, 48000), (48000, 16000)]


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


def spread(ms):
    return {'median': round(float(np.median(ms)), 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3)}


def scipy_ms(x, rate_in, rate_out, quality):
    from scipy.signal import resample_poly
    from spatialaudiogen_amd import resample as R
    L, M, _, h = R.prototype(rate_in, rate_out, quality)
    x64 = x.astype(np.float64)
    resample_poly(x64, L, M, axis=0, window=h / L)
    s = []
    for _ in range(3):
        t0 = time.perf_counter()
        resample_poly(x64, L, M, axis=0, window=h / L)
        s.append(1e3 * (time.perf_counter() - t0))
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=2000)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--no-scipy', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_rate.jsonl'))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures the device: there is none'
    torch.cuda.set_device(0)
    from spatialaudiogen_amd import ops, resample as R
    x = np.random.RandomState(3).uniform(-1., 1., (BLOCK, CHANNELS)).astype(np.float32)
    xd = torch.as_tensor(x).cuda()
    lines = []
    for rate_in, rate_out in CASES:
        for quality in ('best', 'fast'):
            r = R.Resampler(rate_in, rate_out, CHANNELS, quality=quality)
            r.process(xd)                                                # into the middle of a stream: a history in front from here on
            ms = measure(lambda: r.process(xd), args.reps, args.regions)
            n_out = R.output_length(BLOCK, r.L, r.M)
            mk = measure(lambda: ops.resample_fir(xd, 0, r.taps, r.L, r.M, r.H, 0, n_out), args.reps, args.regions)
            secs = BLOCK / float(rate_in)
            res = {'what': 'resample', 'rate_in': rate_in, 'rate_out': rate_out, 'quality': quality, 'channels': CHANNELS, 'block': BLOCK,
                   'L': r.L, 'M': r.M, 'T': int(r.taps.shape[1]), 'reps': args.reps, 'regions': args.regions,
                   'process_ms_per_call': spread(ms), 'kernel_ms_per_call': spread(mk),
                   'process_input_seconds_per_s': round(secs / float(np.median(ms)) * 1e3, 1),
                   'kernel_input_seconds_per_s': round(secs / float(np.median(mk)) * 1e3, 1)}
            if not args.no_scipy:
                s = scipy_ms(x, rate_in, rate_out, quality)
                res['scipy_ms_per_call'] = [round(v, 1) for v in sorted(s)]
                res['scipy_input_seconds_per_s'] = round(secs / float(np.median(s)) * 1e3, 1)
                res['device_over_scipy'] = round(res['process_input_seconds_per_s'] / res['scipy_input_seconds_per_s'], 2)
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
