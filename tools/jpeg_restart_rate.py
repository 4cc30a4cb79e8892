"""What restart intervals buy the device JPEG decoder, and what they cost the device encoder, on the same frames and the same box.

The frames are the 224 x 448 ones tools/jpeg_rate.py synthesises (quality 95, 4:2:0).  They are written three times by
jpeg.JpegEncoder: as today (restart_rows 0), with one row of MCUs per restart interval (14 segments a frame) and with two (7 segments).

  decode   per folder and call size (--blocks): frames per second of jpeg.JpegDecoder.decode over ALL files (paths in, pixels on the
           device: read + parse + pack + copy + the call), and the time of the decode call alone (device events, tools/jpeg_rate.py:
           device_split); host_1 / host_16 (PIL, one thread / a pool of 16, + the copy) for the same folders
  encode   per setting and call size: frames per second of jpeg.JpegEncoder.encode up to the bytes on the host; restart_rows 0 is the
           path of sagen_jpeg_encode unchanged
  bytes    mean file size per setting: what markers, fill bits and DC resets add
  restart  `python -m spatialaudiogen_amd.jpeg restart` (jpeg.transcode_files: sagen_jpeg_transcode, no pixel computed) over the folder
           written as today and over the same pixels saved by PIL with optimize=True (tables of their own), at --rows 1 and 2, in blocks
           of 256: files per second from the files on disk to the files on disk, the bytes before and after, and what the device call
           alone takes (device events around jpeg.transcode_streams for one block of 256)

    python tools/jpeg_restart_rate.py [--frames 640] [--repeats 5] [--blocks 16 64 256 640] [--out profiles/jpeg_restart_rate.jsonl]

Every way is run once to warm up, then `repeats` times; a line holds the median and the sorted times.  One process, the host clock
around a device synchronise.  The split of the decode call into its kernels needs a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/jpeg_restart_rate.py --trace-run
    python tools/jpeg_restart_rate.py --digest DIR [--out profiles/jpeg_restart_rate.jsonl]

--trace-run decodes one block of 64 frames of each folder ten times and nothing else; the three folders launch the entropy kernel
with different grids (64, 448 and 896 segments), which is how --digest tells them apart."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
ROWS = (0, 1, 2)


def write_folders(tmp, n):
    """{restart_rows: [paths]}: the same pixels, written by the device encoder; rows 0 compared with PIL's files on libjpeg-turbo"""
    import torch
    from PIL import features
    from jpeg_encode_rate import make_frames, pil_bytes
    from spatialaudiogen_amd import jpeg
    frames = make_frames(n)
    dev = torch.as_tensor(frames).to('cuda')
    folders = {}
    for rows in ROWS:
        enc = jpeg.JpegEncoder('cuda', 95, '4:2:0', restart_rows=rows)
        files = [d for i in range(0, n, 64) for d in enc.encode(dev[i:i + 64])]
        if rows == 0 and features.check_feature('libjpeg_turbo'):
            assert files[:8] == [pil_bytes(f) for f in frames[:8]]
        os.makedirs(os.path.join(tmp, 'rows%d' % rows))
        folders[rows] = [os.path.join(tmp, 'rows%d' % rows, '%06d.jpg' % k) for k in range(n)]
        for name, d in zip(folders[rows], files):
            with open(name, 'wb') as f:
                f.write(d)
    return dev, folders


def measure_decode(folders, n, repeats, blocks):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from jpeg_rate import device_split, rate, timed
    from spatialaudiogen_amd import jpeg
    from spatialaudiogen_amd.feeder import imread
    from spatialaudiogen_amd.frames import load_frames
    pool = ThreadPoolExecutor(16)
    dec = jpeg.JpegDecoder('cuda')
    keep, lines = {}, []
    for rows in ROWS:
        names = folders[rows]
        res = {'what': 'jpeg_restart_decode', 'restart_rows': rows, 'segments_per_frame': jpeg.parse(open(names[0], 'rb').read()).segments.size,
               'frames': '224x448', 'n_frames': n, 'repeats': repeats, 'file_bytes_mean': int(np.mean([os.path.getsize(f) for f in names]))}

        def host_1():
            for i in range(0, n, 64):
                keep['a'] = torch.as_tensor(load_frames(names[i:i + 64])).to('cuda')

        def host_16():
            for i in range(0, n, 64):
                keep['b'] = torch.as_tensor(np.stack(list(pool.map(imread, names[i:i + 64])), 0)).to('cuda')

        res['host_1'] = rate(n, timed(host_1, repeats))
        res['host_16'] = rate(n, timed(host_16, repeats))
        res['device_by_block'] = {}
        for block in blocks:
            def device():
                for i in range(0, n, block):
                    keep['c'] = dec.decode(names[i:i + block])
            r = rate(n, timed(device, repeats))
            device_split(names[:block], block)
            splits = [device_split(names, block) for _ in range(repeats)]
            calls = -(-n // block)
            r['decode_call_ms'] = round(float(np.median([s['decode_call_ms'] for s in splits])) / calls, 3)
            r['read_parse_pack_ms_per_call'] = round(1e3 * float(np.median([s['read_parse_s'] + s['pack_s'] for s in splits])) / calls, 3)
            r.update(over_host_1=round(r['frames_per_s'] / res['host_1']['frames_per_s'], 2), over_host_16=round(r['frames_per_s'] / res['host_16']['frames_per_s'], 2))
            res['device_by_block'][str(block)] = r
        if rows:
            assert torch.equal(keep['c'], keep['first']) and torch.equal(keep['a'][-1], keep['c'][-1])       # the same pixels from every folder
        else:
            keep['first'] = keep['c'].clone()
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    pool.shutdown()
    return lines


def measure_encode(dev, n, repeats, blocks):
    from jpeg_rate import rate, timed
    from spatialaudiogen_amd import jpeg
    lines, keep = [], {}
    encs = {rows: jpeg.JpegEncoder('cuda', 95, '4:2:0', restart_rows=rows) for rows in ROWS}
    res = {rows: {'what': 'jpeg_restart_encode', 'restart_rows': rows, 'frames': '224x448', 'n_frames': n, 'repeats': repeats, 'device_by_block': {}} for rows in ROWS}
    for block in blocks:
        for rows in ROWS:                                               # the settings alternate inside a call size
            def device():
                keep['c'] = [d for i in range(0, n, block) for d in encs[rows].encode(dev[i:i + block])]
            res[rows]['device_by_block'][str(block)] = rate(n, timed(device, repeats))
            res[rows]['file_bytes_mean'] = int(np.mean([len(d) for d in keep['c']]))
    for rows in ROWS:
        for block in blocks:
            r = res[rows]['device_by_block'][str(block)]
            r['over_rows_0'] = round(r['frames_per_s'] / res[0]['device_by_block'][str(block)]['frames_per_s'], 3)
        print(json.dumps(res[rows]), flush=True)
        lines.append(json.dumps(res[rows]))
    return lines


def measure_restart(tmp, folders, n, repeats):
    import shutil
    import time
    import torch
    from PIL import Image
    from jpeg_encode_rate import make_frames
    from spatialaudiogen_amd import jpeg
    opt = os.path.join(tmp, 'optimised')
    os.makedirs(opt)
    for k, f in enumerate(make_frames(n)):
        Image.fromarray(f).save(os.path.join(opt, '%06d.jpg' % k), quality=95, optimize=True)
    lines = []
    for source, folder in (('as today (standard tables)', os.path.dirname(folders[0][0])), ('PIL optimize=True', opt)):
        for rows in (1, 2):
            out = os.path.join(tmp, 'restart_out')
            times = []
            for r in range(repeats + 1):
                shutil.rmtree(out, ignore_errors=True)
                t0 = time.perf_counter()
                jpeg.main(['restart', folder, out, '--rows', str(rows), '--block', '256'])
                torch.cuda.synchronize()
                if r:
                    times.append(time.perf_counter() - t0)
            names = sorted(os.listdir(folder))
            before = sum(os.path.getsize(os.path.join(folder, f)) for f in names)
            after = sum(os.path.getsize(os.path.join(out, f)) for f in names)
            datas = [open(os.path.join(folder, f), 'rb').read() for f in names[:256]]
            infos = [jpeg.parse(d) for d in datas]
            packed = jpeg.pack(datas, infos)
            staged = torch.as_tensor(packed.buffer).to('cuda')
            ms = []
            for r in range(repeats + 1):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                o, sizes, status = jpeg.transcode_streams(packed, staged, rows * 28, 96 * 1024)
                e[1].record()
                torch.cuda.synchronize()
                assert not bool(status.any())
                if r:
                    ms.append(e[0].elapsed_time(e[1]))
            same = jpeg.JpegDecoder('cuda').decode([os.path.join(out, f) for f in names[:64]])
            assert torch.equal(same, jpeg.JpegDecoder('cuda').decode([os.path.join(folder, f) for f in names[:64]]))     # the same pixels
            res = {'what': 'jpeg_restart_transcode', 'source': source, 'rows': rows, 'n_files': n, 'block': 256, 'repeats': repeats,
                   'files_per_s': round(n / float(np.median(times)), 1), 'seconds': [round(t, 4) for t in sorted(times)], 'bytes_before': before,
                   'bytes_after': after, 'growth_percent': round(100. * (after - before) / before, 3),
                   'device_call_ms_256_files': round(float(np.median(ms)), 3)}
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
    return lines


def trace_run():
    import torch
    from spatialaudiogen_amd import jpeg
    with tempfile.TemporaryDirectory() as tmp:
        dev, folders = write_folders(tmp, 64)
        dec = jpeg.JpegDecoder('cuda')
        for rows in ROWS:
            for _ in range(10):
                dec.decode(folders[rows])
        torch.cuda.synchronize()


def digest(folder, out):
    traces = glob.glob(os.path.join(folder, '**', '*kernel_trace.csv'), recursive=True)
    assert traces, 'no *kernel_trace.csv under %s' % folder
    per = {}
    for row in csv.DictReader(open(traces[0])):
        name = row['Kernel_Name']
        if 'jpeg_' not in name or 'jpeg_enc_' in name:
            continue
        short = name[name.index('jpeg_'):].split('(')[0]
        per.setdefault((short, int(row['Grid_Size_X']) * int(row['Grid_Size_Y'])), []).append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3)
    lines = []
    for (short, grid), us in sorted(per.items()):
        lines.append(json.dumps({'what': 'jpeg_restart_decode_kernel', 'block': 64, 'kernel': short, 'grid_threads': grid, 'launches': len(us),
                                 'us_mean': round(float(np.mean(us)), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2)}))
        print(lines[-1])
    with open(out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=640)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--blocks', type=int, nargs='*', default=[16, 64, 256, 640], help='frames per device call')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_restart_rate.jsonl'))
    ap.add_argument('--restart-only', action='store_true', help='the restart section alone')
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
    with tempfile.TemporaryDirectory() as tmp:
        dev, folders = write_folders(tmp, args.frames)
        lines = [] if args.restart_only else measure_decode(folders, args.frames, args.repeats, args.blocks)
        if not args.restart_only:
            lines += measure_encode(dev, args.frames, args.repeats, args.blocks)
        lines += measure_restart(tmp, folders, args.frames, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
