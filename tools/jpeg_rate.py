"""Frames per second of the three ways to get a folder of JPEG frames onto the device, on the same files and the same box:

  host_1      frames.load_frames (PIL, one thread) + .to(device): what project / flow / overlay do by default
  host_16     the same PIL decode in a pool of 16 threads (PIL releases the GIL while it decodes) + .to(device)
  device      jpeg.JpegDecoder.decode (csrc/jpeg.hip): the files' bytes go to the device, blocks of 64 frames (16 for the large size)

and, for `device`, where the time of a block goes: reading + parsing the files and packing the staging buffer (host clock), the
one host-to-device copy and the decode call (device events around each, the call = memset + the five kernels of jpeg.hip).

    python tools/jpeg_rate.py [--frames 640] [--large 16] [--repeats 3] [--blocks 256 640] [--out profiles/jpeg_rate.jsonl]

Frames are synthetic (smooth gradients that move + noise of +-12 levels), quality 95, 4:2:0, written to a temporary folder:
224 x 448 (what deploy reads) and 2160 x 3240.  Every way is run once to warm up (page cache, pinned buffers, code objects), then
`repeats` times over ALL files; the line holds the median and the spread.  One JSON line per size is printed and appended to --out.
The entropy stage runs one lane per frame, so its rate grows with the frames of a call: `device_by_block` repeats `device` for the
224 x 448 folder at the call sizes of --blocks.

The split of the decode call into its kernels needs a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/jpeg_rate.py --trace-run
    python tools/jpeg_rate.py --digest DIR [--out profiles/jpeg_rate.jsonl]

--trace-run decodes 10 blocks of 64 frames of 224 x 448 and 4 blocks of 16 of 2160 x 3240 and nothing else; --digest adds the
kernels' times per launch to --out, one line per kernel and grid size (the two sizes launch different grids)."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {'224x448': (224, 448, 64), '2160x3240': (2160, 3240, 16)}      # name -> (h, w, frames per device call)


def write_frames(folder, n, h, w, seed):
    from PIL import Image
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    names = []
    for k in range(n):
        a = np.stack([127 + 100 * np.sin((x + 5 * k) / (w / 19.)), 127 + 100 * np.cos((y - 3 * k) / (h / 13.)), (255 * (x + 2 * y) // (w + 2 * h) + 9 * k) % 256], -1)
        a = np.clip(a + rs.randint(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
        names.append(os.path.join(folder, '%06d.jpg' % k))
        Image.fromarray(a).save(names[-1], quality=95, subsampling=2)
    return names


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


def device_split(names, block):
    """Per block: host seconds of read + parse and of pack, device ms of the copy and of the call; summed over the folder."""
    import torch
    from spatialaudiogen_amd import jpeg
    tot = {'read_parse_s': 0., 'pack_s': 0., 'h2d_ms': 0., 'decode_call_ms': 0., 'bytes': 0}
    for i in range(0, len(names), block):
        t0 = time.perf_counter()
        datas = [open(n, 'rb').read() for n in names[i:i + block]]
        infos = [jpeg.parse(d) for d in datas]
        t1 = time.perf_counter()
        holder = {}

        def pinned(nbytes):
            holder['t'] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            return holder['t'].numpy()

        packed = jpeg.pack(datas, infos, pinned)
        t2 = time.perf_counter()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        staged = holder['t'].to('cuda', non_blocking=True)
        e[1].record()
        out, status = jpeg.decode_packed(packed, staged)
        e[2].record()
        torch.cuda.synchronize()
        assert not bool(status.any())
        tot['read_parse_s'] += t1 - t0
        tot['pack_s'] += t2 - t1
        tot['h2d_ms'] += e[0].elapsed_time(e[1])
        tot['decode_call_ms'] += e[1].elapsed_time(e[2])
        tot['bytes'] += packed.total_bytes
    return tot


def measure(name, n, repeats, tmp, more_blocks=()):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from spatialaudiogen_amd import jpeg
    from spatialaudiogen_amd.feeder import imread
    from spatialaudiogen_amd.frames import load_frames
    h, w, block = SIZES[name]
    folder = os.path.join(tmp, name)
    os.makedirs(folder)
    names = write_frames(folder, n, h, w, 7)
    blocks = [names[i:i + block] for i in range(0, n, block)]
    pool = ThreadPoolExecutor(16)
    dec = jpeg.JpegDecoder('cuda')
    keep = {}

    def host_1():
        for b in blocks:
            keep['a'] = torch.as_tensor(load_frames(b)).to('cuda')

    def host_16():
        for b in blocks:
            keep['b'] = torch.as_tensor(np.stack(list(pool.map(imread, b)), 0)).to('cuda')

    def device():
        for b in blocks:
            keep['c'] = dec.decode(b)

    res = {'what': 'jpeg_decode', 'frames': name, 'n_frames': n, 'block': block, 'quality': 95, 'subsampling': '4:2:0', 'repeats': repeats,
           'file_bytes_mean': int(np.mean([os.path.getsize(f) for f in names])), 'raw_bytes': h * w * 3}
    res['host_1'] = rate(n, timed(host_1, repeats))
    res['host_16'] = rate(n, timed(host_16, repeats))
    res['device'] = rate(n, timed(device, repeats))
    from PIL import features
    if features.check_feature('libjpeg_turbo'):                         # (another JPEG library need not agree to the byte)
        assert torch.equal(keep['a'], keep['c']) and torch.equal(keep['b'], keep['c'])
    res['device_by_block'] = {}
    for bigger in more_blocks:
        def device_bigger():
            for i in range(0, n, bigger):
                keep['c'] = dec.decode(names[i:i + bigger])
        res['device_by_block'][str(bigger)] = rate(n, timed(device_bigger, repeats))
    device_split(names[:block], block)                                  # warm-up of this path's own buffers
    splits = [device_split(names, block) for _ in range(repeats)]
    med = lambda k: float(np.median([s[k] for s in splits]))
    res['device_split_per_frame_us'] = {'read_parse': round(1e6 * med('read_parse_s') / n, 1), 'pack': round(1e6 * med('pack_s') / n, 1),
                                        'h2d': round(1e3 * med('h2d_ms') / n, 2), 'decode_call': round(1e3 * med('decode_call_ms') / n, 2)}
    res['device_over_host_1'] = round(res['device']['frames_per_s'] / res['host_1']['frames_per_s'], 2)
    res['device_over_host_16'] = round(res['device']['frames_per_s'] / res['host_16']['frames_per_s'], 2)
    pool.shutdown()
    return res


def trace_run():
    import torch
    from spatialaudiogen_amd import jpeg
    with tempfile.TemporaryDirectory() as tmp:
        for name, calls in (('224x448', 10), ('2160x3240', 4)):
            h, w, block = SIZES[name]
            os.makedirs(os.path.join(tmp, name))
            names = write_frames(os.path.join(tmp, name), block, h, w, 7)
            dec = jpeg.JpegDecoder('cuda')
            for _ in range(calls):
                dec.decode(names)
            torch.cuda.synchronize()


def digest(folder, out):
    files = glob.glob(os.path.join(folder, '**', '*kernel_stats.csv'), recursive=True)
    assert files, 'no *kernel_stats.csv under %s' % folder
    # the two sizes run the same kernels: per-launch times come from the trace, split by grid size
    traces = glob.glob(os.path.join(folder, '**', '*kernel_trace.csv'), recursive=True)
    assert traces, 'no *kernel_trace.csv under %s' % folder
    per = {}
    for row in csv.DictReader(open(traces[0])):
        name = row['Kernel_Name']
        if 'jpeg_' not in name:
            continue
        short = name[name.index('jpeg_'):].split('(')[0]
        per.setdefault((short, int(row['Grid_Size_X']) * int(row['Grid_Size_Y'])), []).append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3)
    lines = []
    for (short, grid), us in sorted(per.items()):
        lines.append(json.dumps({'what': 'jpeg_decode_kernel', 'kernel': short, 'grid_threads': grid, 'launches': len(us), 'us_mean': round(float(np.mean(us)), 2),
                                 'us_min': round(min(us), 2), 'us_max': round(max(us), 2)}))
        print(lines[-1])
    with open(out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=640)
    ap.add_argument('--large', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--blocks', type=int, nargs='*', default=[256, 640], help='further frames-per-call settings for the 224 x 448 folder')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_rate.jsonl'))
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
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, n in (('224x448', args.frames), ('2160x3240', args.large)):
            res = measure(name, n, args.repeats, tmp, args.blocks if name == '224x448' else ())
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
