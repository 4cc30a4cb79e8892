"""Frames per second of the ways to turn frames that are ON THE DEVICE into JPEG files' bytes on the host, on the same frames and box:

  host_1      frames.cpu().numpy() + PIL's save into memory, one thread: what project / flow do by default (frames.FrameWriter, encode='host')
  host_16     the same copy, then PIL's save in a pool of 16 threads (PIL releases the GIL while it encodes)
  device      jpeg.JpegEncoder.encode (csrc/jpeg_enc.hip) in blocks of 16, 64, 256 and 640 frames, up to the bytes on the host

    python tools/jpeg_encode_rate.py [--frames 640] [--repeats 3] [--blocks 16 64 256 640] [--out profiles/jpeg_encode_rate.jsonl]

The frames are the 224 x 448 ones tools/jpeg_rate.py synthesises (smooth gradients that move + noise of +-12 levels), quality 95,
4:2:0.  Every way is run once to warm up, then `repeats` times over ALL frames; the line holds the median and the spread.  Writing the
files is left out on both sides: it is the same bytes either way.  On libjpeg-turbo the device's files are compared with PIL's.

The split of the encode call into its kernels needs a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/jpeg_encode_rate.py --trace-run
    python tools/jpeg_encode_rate.py --digest DIR [--out profiles/jpeg_encode_rate.jsonl]

--trace-run encodes one block of 64 frames ten times and nothing else; --digest adds each kernel's time per launch and its share of
the call to --out, one line per kernel."""
import argparse
import csv
import glob
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 224, 448


def make_frames(n, seed=7):
    """the pixels tools/jpeg_rate.py writes to its folder"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((n, H, W, 3), np.uint8)
    for k in range(n):
        a = np.stack([127 + 100 * np.sin((x + 5 * k) / (W / 19.)), 127 + 100 * np.cos((y - 3 * k) / (H / 13.)), (255 * (x + 2 * y) // (W + 2 * H) + 9 * k) % 256], -1)
        out[k] = np.clip(a + rs.randint(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
    return out


def pil_bytes(frame):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(frame).save(b, 'JPEG', quality=95)
    return b.getvalue()


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    s = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    return s


def rate(n, s):
    return {'frames_per_s': round(n / float(np.median(s)), 1), 'seconds': [round(t, 4) for t in sorted(s)]}


def measure(n, repeats, blocks):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import features
    from spatialaudiogen_amd import jpeg
    frames = torch.as_tensor(make_frames(n)).to('cuda')
    pool = ThreadPoolExecutor(16)
    enc = jpeg.JpegEncoder('cuda', 95, '4:2:0')
    keep = {}

    def host_1():
        keep['a'] = [pil_bytes(f) for f in frames.cpu().numpy()]

    def host_16():
        keep['b'] = list(pool.map(pil_bytes, frames.cpu().numpy()))

    res = {'what': 'jpeg_encode', 'frames': '%dx%d' % (H, W), 'n_frames': n, 'quality': 95, 'subsampling': '4:2:0', 'repeats': repeats, 'raw_bytes': H * W * 3}
    res['host_1'] = rate(n, timed(host_1, repeats))
    res['host_16'] = rate(n, timed(host_16, repeats))
    res['file_bytes_mean'] = int(np.mean([len(d) for d in keep['a']]))
    res['device_by_block'] = {}
    for block in blocks:
        def device():
            keep['c'] = [d for i in range(0, n, block) for d in enc.encode(frames[i:i + block])]
        res['device_by_block'][str(block)] = rate(n, timed(device, repeats))
        if features.check_feature('libjpeg_turbo'):                     # (another JPEG library need not agree to the byte)
            assert keep['c'] == keep['a'] == keep['b']
    for block in blocks:
        fps = res['device_by_block'][str(block)]['frames_per_s']
        res['device_by_block'][str(block)].update(over_host_1=round(fps / res['host_1']['frames_per_s'], 2), over_host_16=round(fps / res['host_16']['frames_per_s'], 2))
    pool.shutdown()
    return res


def trace_run():
    import torch
    from spatialaudiogen_amd import jpeg
    frames = torch.as_tensor(make_frames(64)).to('cuda')
    enc = jpeg.JpegEncoder('cuda', 95, '4:2:0')
    for _ in range(10):
        enc.encode(frames)
    torch.cuda.synchronize()


def digest(folder, out):
    traces = glob.glob(os.path.join(folder, '**', '*kernel_trace.csv'), recursive=True)
    assert traces, 'no *kernel_trace.csv under %s' % folder
    per = {}
    for row in csv.DictReader(open(traces[0])):
        name = row['Kernel_Name']
        if 'jpeg_enc_' not in name:
            continue
        short = name[name.index('jpeg_enc_'):].split('(')[0]
        per.setdefault(short, []).append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3)
    launches = min(len(v) for v in per.values())
    total = sum(sum(v) for v in per.values()) / launches
    lines = []
    for short, us in sorted(per.items()):
        lines.append(json.dumps({'what': 'jpeg_encode_kernel', 'block': 64, 'kernel': short, 'launches': len(us), 'us_mean': round(float(np.mean(us)), 2),
                                 'us_min': round(min(us), 2), 'us_max': round(max(us), 2), 'share_of_kernels': round(sum(us) / launches / total, 3)}))
        print(lines[-1])
    lines.append(json.dumps({'what': 'jpeg_encode_kernels_total', 'block': 64, 'us_per_call': round(total, 1), 'us_per_frame': round(total / 64, 2)}))
    print(lines[-1])
    with open(out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=640)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--blocks', type=int, nargs='*', default=[16, 64, 256, 640], help='frames per device call')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_encode_rate.jsonl'))
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--digest', default=None, metavar='DIR')
    args = ap.parse_args()
    if args.digest:
        return digest(args.digest, args.out)
    import torch
    assert torch.cuda.is_available(), 'this tool measures the device: there is none'
    torch.cuda.set_device(0)
    if args.trace_run:
        return trace_run()
    res = measure(args.frames, args.repeats, args.blocks)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
