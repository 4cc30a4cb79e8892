"""What the split entropy decode (sagen_jpeg_decode_split, csrc/jpeg_split.hip) buys jpeg.JpegDecoder on files WITHOUT restart markers, on
the same files and the same box as tools/jpeg_rate.py and by its protocol: every way warmed once, the median of `repeats` passes over
all files, the host clock around work that ends in a synchronise, everything in one process.

  workloads   640 frames of 224 x 448 in calls of 16 / 64 / 256 / 640 frames; 16 frames of 2160 x 3240 in calls of 16 (tools/jpeg_rate.py's
              files: smooth + noise, quality 95, 4:2:0); the 224 x 448 frames written by the device encoder with one and two rows of MCUs
              per restart interval (tools/jpeg_restart_rate.py's folders) in calls of 64, to see that the split does not hurt them
  ways        host_1 / host_16: PIL in 1 and 16 threads + copy; lane: JpegDecoder(); split: JpegDecoder(entropy='split') over
              chunk_bytes in --chunks x rounds in --rounds, with the share of frames per `path` value of every cell

    python tools/jpeg_split_rate.py [--frames 640] [--large 16] [--repeats 3] [--out profiles/jpeg_split_rate.jsonl]

One JSON line per workload is printed and appended to --out; its 'best' names the fastest cell whose UNSETTLED share is 0.  The
baseline for "faster than before" is the parent commit's tools/jpeg_rate.py in the same session, not this file's `lane` row, which
must merely reproduce it.

The split of a call into its kernels needs a profiler run of its own, combined with nothing else:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/jpeg_split_rate.py --trace-run [--cell 256 8]
    python tools/jpeg_split_rate.py --digest DIR [--out profiles/jpeg_split_rate.jsonl]

--trace-run decodes 64 frames of 224 x 448 and 16 of 2160 x 3240 three times each with `lane` and with `split` at --cell and nothing
else; --digest adds the kernels' times per launch to --out, one line per kernel and grid size."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from jpeg_rate import SIZES, rate, timed, write_frames      # noqa: E402

CHUNKS = (128, 256, 512, 1024, 2048)
ROUNDS = (2, 3, 4, 6, 8)


def decode_all(dec, names, block, keep, shares=None):
    for i in range(0, len(names), block):
        keep['out'] = dec.decode(names[i:i + block])
        if shares is not None:
            for v, c in dec.last_paths.items():
                shares[v] = shares.get(v, 0) + c


def measure(what, names, blocks, repeats, chunks, rounds, hosts=True):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from spatialaudiogen_amd import jpeg
    from spatialaudiogen_amd.feeder import imread
    from spatialaudiogen_amd.frames import load_frames
    n = len(names)
    info = jpeg.parse(open(names[0], 'rb').read())
    lines, keep = [], {}
    for block in blocks:
        res = {'what': 'jpeg_split_decode', 'frames': what, 'n_frames': n, 'block': block, 'repeats': repeats, 'segments_per_frame': int(info.segments.size),
               'scan_bytes_mean': int(np.mean([jpeg.parse(open(f, 'rb').read()).scan_bytes for f in names[:16]]))}
        if hosts:
            pool = ThreadPoolExecutor(16)

            def host_1():
                for i in range(0, n, block):
                    keep['a'] = torch.as_tensor(load_frames(names[i:i + block])).to('cuda')

            def host_16():
                for i in range(0, n, block):
                    keep['a'] = torch.as_tensor(np.stack(list(pool.map(imread, names[i:i + block])), 0)).to('cuda')
            res['host_1'] = rate(n, timed(host_1, repeats))
            res['host_16'] = rate(n, timed(host_16, repeats))
            pool.shutdown()
        lane = jpeg.JpegDecoder('cuda')
        res['lane'] = rate(n, timed(lambda: decode_all(lane, names, block, keep), repeats))
        want = keep['out'].clone()
        res['split'], best = {}, None
        for cb in chunks:
            for r in rounds:
                dec = jpeg.JpegDecoder('cuda', entropy='split', chunk_bytes=cb, rounds=r)
                cell = rate(n, timed(lambda: decode_all(dec, names, block, keep), repeats))
                assert torch.equal(keep['out'], want)                   # (the last call's frames: the same pixels)
                shares = {}
                decode_all(dec, names, block, keep, shares)
                cell['path_share'] = {str(v): round(c / float(n), 4) for v, c in sorted(shares.items())}
                cell['over_lane'] = round(cell['frames_per_s'] / res['lane']['frames_per_s'], 2)
                res['split']['%dx%d' % (cb, r)] = cell
                if not shares.get(1) and (best is None or cell['frames_per_s'] > best[1]):
                    best = ('%dx%d' % (cb, r), cell['frames_per_s'])
        res['best'] = {'cell': best[0], 'frames_per_s': best[1]} if best else None
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    return lines


def segmented_folders(tmp, names):
    """tools/jpeg_restart_rate.py's folders: the same pixels written by the device encoder with 1 and 2 rows of MCUs per interval"""
    import torch
    from spatialaudiogen_amd import jpeg
    from spatialaudiogen_amd.frames import load_frames
    dev = torch.as_tensor(load_frames(names)).to('cuda')
    folders = {}
    for rows in (1, 2):
        os.makedirs(os.path.join(tmp, 'rows%d' % rows))
        files = jpeg.JpegEncoder('cuda', 95, '4:2:0', restart_rows=rows).encode(dev)
        folders[rows] = [os.path.join(tmp, 'rows%d' % rows, '%06d.jpg' % k) for k in range(len(files))]
        for name, d in zip(folders[rows], files):
            with open(name, 'wb') as f:
                f.write(d)
    return folders


def trace_run(cell):
    import torch
    from spatialaudiogen_amd import jpeg
    with tempfile.TemporaryDirectory() as tmp:
        for name in ('224x448', '2160x3240'):
            h, w, block = SIZES[name]
            os.makedirs(os.path.join(tmp, name))
            names = write_frames(os.path.join(tmp, name), block, h, w, 7)
            for dec in (jpeg.JpegDecoder('cuda'), jpeg.JpegDecoder('cuda', entropy='split', chunk_bytes=cell[0], rounds=cell[1])):
                for _ in range(3):
                    dec.decode(names)
            torch.cuda.synchronize()


def digest(folder, out):
    import csv
    import glob
    traces = glob.glob(os.path.join(folder, '**', '*kernel_trace.csv'), recursive=True)
    assert traces, 'no *kernel_trace.csv under %s' % folder
    per = {}
    for row in csv.DictReader(open(traces[0])):
        name = row['Kernel_Name']
        if 'jpeg_' not in name:
            continue
        short = name[name.index('jpeg_'):].split('(')[0]
        per.setdefault((short, int(row['Grid_Size_X']) * int(row['Grid_Size_Y']) * int(row.get('Grid_Size_Z', 1) or 1)), []).append(
            (int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3)
    lines = []
    for (short, grid), us in sorted(per.items()):
        lines.append(json.dumps({'what': 'jpeg_split_decode_kernel', 'kernel': short, 'grid_threads': grid, 'launches': len(us),
                                 'us_mean': round(float(np.mean(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2)}))
        print(lines[-1])
    with open(out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=640)
    ap.add_argument('--large', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--blocks', type=int, nargs='*', default=[16, 64, 256, 640])
    ap.add_argument('--chunks', type=int, nargs='*', default=list(CHUNKS))
    ap.add_argument('--rounds', type=int, nargs='*', default=list(ROUNDS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_split_rate.jsonl'))
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--cell', type=int, nargs=2, default=[256, 8], metavar=('CHUNK_BYTES', 'ROUNDS'))
    ap.add_argument('--digest', default=None, metavar='DIR')
    args = ap.parse_args()
    if args.digest:
        return digest(args.digest, args.out)
    import torch
    assert torch.cuda.is_available(), 'this tool measures the device: there is none'
    torch.cuda.set_device(0)
    if args.trace_run:
        return trace_run(args.cell)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'small'))
        os.makedirs(os.path.join(tmp, 'large'))
        small = write_frames(os.path.join(tmp, 'small'), args.frames, 224, 448, 7)
        lines += measure('224x448', small, args.blocks, args.repeats, args.chunks, args.rounds)
        large = write_frames(os.path.join(tmp, 'large'), args.large, 2160, 3240, 7)
        lines += measure('2160x3240', large, [16], args.repeats, args.chunks, args.rounds)
        for rows, names in sorted(segmented_folders(tmp, small).items()):
            lines += measure('224x448 restart_rows %d' % rows, names, [64], args.repeats, args.chunks, args.rounds, hosts=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
