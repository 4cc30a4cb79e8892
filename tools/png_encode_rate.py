"""Frames per second of the ways to turn frames that are ON THE DEVICE into PNG files' bytes on the host, on the same frames and box:

  host_1      frames.cpu().numpy() + PIL's save into memory, one thread: what overlay / deploy --overlay_dir do by default (frames.FrameWriter, encode='host')
  host_16     the same copy, then PIL's save in a pool of 16 threads (PIL releases the GIL while zlib runs)
  device      png.PngEncoder.encode (csrc/png.hip) in blocks of 16, 50, 64 and 256 frames, up to the bytes on the host

    python tools/png_encode_rate.py [--frames 256] [--repeats 3] [--blocks 16 50 64 256] [--out profiles/png_encode_rate.jsonl]

The frames are 224 x 448 with the spectrum of photographs (tests/png_oracle.py: natural, sixteen of them, rolled).  Every way is run once
to warm up, then `repeats` times over ALL frames; the line holds the median and the spread.  Writing the files is left out on both
sides.  Every device file is decoded with PIL and compared with its frame once, outside the timing.

    python tools/png_encode_rate.py --clip 20

adds the wall time of `overlay` and of `deploy --overlay_dir` on one synthetic clip of that many seconds (an audio-only model with
seeded weights; each command is run twice per mode and the second run is taken), --encode host against --encode device.

The split of the encode call into its kernels needs a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/png_encode_rate.py --trace-run
    python tools/png_encode_rate.py --digest DIR [--out profiles/png_encode_rate.jsonl]

--trace-run encodes one block of 64 frames ten times and nothing else; --digest adds each kernel's time per launch and its share of
the call to --out, one line per kernel."""
import argparse
import csv
import glob
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
H, W = 224, 448
KERNELS = ('png_filter_kernel', 'deflate_plan_kernel', 'deflate_place_kernel', 'deflate_bits_kernel', 'deflate_copy_kernel')


def make_frames(n):
    import png_oracle as PO
    base = [PO.natural(s) for s in range(1, 17)]
    return np.stack([np.roll(base[k % 16], 13 * (k // 16), 1) for k in range(n)], 0)


def pil_bytes(frame):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(frame).save(b, 'PNG')
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
    from PIL import Image
    from spatialaudiogen_amd import png
    host = make_frames(n)
    frames = torch.as_tensor(host).to('cuda')
    pool = ThreadPoolExecutor(16)
    enc = png.PngEncoder('cuda')
    keep = {}

    def host_1():
        keep['a'] = [pil_bytes(f) for f in frames.cpu().numpy()]

    def host_16():
        keep['b'] = list(pool.map(pil_bytes, frames.cpu().numpy()))

    res = {'what': 'png_encode', 'frames': '%dx%d' % (H, W), 'n_frames': n, 'repeats': repeats, 'raw_bytes': H * (1 + W * 3)}
    res['host_1'] = rate(n, timed(host_1, repeats))
    res['host_16'] = rate(n, timed(host_16, repeats))
    res['pil_file_bytes_mean'] = int(np.mean([len(d) for d in keep['a']]))
    res['device_by_block'] = {}
    for block in blocks:
        def device():
            keep['c'] = [d for i in range(0, n, block) for d in enc.encode(frames[i:i + block])]
        res['device_by_block'][str(block)] = rate(n, timed(device, repeats))
    res['device_file_bytes_mean'] = int(np.mean([len(d) for d in keep['c']]))
    for k, d in enumerate(keep['c']):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(d))), host[k]), k
    for block in blocks:
        fps = res['device_by_block'][str(block)]['frames_per_s']
        res['device_by_block'][str(block)].update(over_host_1=round(fps / res['host_1']['frames_per_s'], 2), over_host_16=round(fps / res['host_16']['frames_per_s'], 2))
    pool.shutdown()
    return res


def make_clip(root, secs):
    """A clip folder as deploy reads it (ambix/%06d.wav of one second each, video/%06d.jpg at 10 a second, audio_pow.lst): seeded noise to
    hear, the frames of make_frames to see."""
    from PIL import Image
    from spatialaudiogen_amd.feeder import save_wav
    rs = np.random.RandomState(0)
    os.makedirs(os.path.join(root, 'ambix'))
    os.makedirs(os.path.join(root, 'video'))
    for i in range(secs):
        save_wav(os.path.join(root, 'ambix', '%06d.wav' % i), np.clip(0.3 * rs.randn(48000, 4), -1, 1), 48000)
    with open(os.path.join(root, 'audio_pow.lst'), 'w') as f:
        for i in range((secs - 1) * 10):
            f.write('{} {}\n'.format(i / 10. + 0.5, 0.1 + 0.01 * i))
    for i, fr in enumerate(make_frames(secs * 10)):
        Image.fromarray(fr).save(os.path.join(root, 'video', '%06d.jpg' % i), quality=95)


def clip_run(secs):
    """overlay and deploy --overlay_dir on one clip, --encode host against device: the second of two runs each."""
    from spatialaudiogen_amd import deploy, overlay
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    tmp = tempfile.mkdtemp(prefix='png_clip_')
    try:
        model_dir, clip_dir, wav = os.path.join(tmp, 'model'), os.path.join(tmp, 'clip'), os.path.join(tmp, 'ambi.wav')
        os.makedirs(model_dir)
        np.savez(os.path.join(model_dir, 'variables.npz'), **init_weights(variable_specs(['audio']), seed=8, mode='test'))
        with open(os.path.join(model_dir, 'train-params.txt'), 'w') as f:
            f.write("encoders: ['audio']\nseparation: unet_mask\nambi_order: 1\naudio_rate: 48000\nvideo_rate: 10\ncontext: 1.0\n"
                    "num_sep_tracks: 32\nloc_units: [512, 512]\n")
        make_clip(clip_dir, secs + 2)
        res = {'what': 'png_clip', 'clip_seconds': secs}
        for tool in ('deploy', 'overlay'):
            for mode in ('host', 'device'):
                out = os.path.join(tmp, '%s_%s' % (tool, mode))
                for _ in range(2):
                    t0 = time.perf_counter()
                    if tool == 'deploy':
                        deploy.main([model_dir, clip_dir, '--deploy_duration', str(secs), '--output_fn', wav, '--overlay_dir', out, '--overwrite', '--encode', mode])
                    else:
                        overlay.main([wav, os.path.join(clip_dir, 'video'), out, '--overwrite', '--encode', mode])
                    took = time.perf_counter() - t0
                res['%s_%s_s' % (tool, mode)] = round(took, 3)
                res['%s_frames' % tool] = len(os.listdir(out))
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def trace_run():
    import torch
    from spatialaudiogen_amd import png
    frames = torch.as_tensor(make_frames(64)).to('cuda')
    enc = png.PngEncoder('cuda')
    for _ in range(10):
        enc.encode(frames)
    torch.cuda.synchronize()


def digest(folder, out):
    traces = glob.glob(os.path.join(folder, '**', '*kernel_trace.csv'), recursive=True)
    assert traces, 'no *kernel_trace.csv under %s' % folder
    per = {}
    for row in csv.DictReader(open(traces[0])):
        for short in KERNELS:
            if short in row['Kernel_Name']:
                per.setdefault(short, []).append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3)
    launches = min(len(v) for v in per.values())
    total = sum(sum(v) for v in per.values()) / launches
    lines = []
    for short, us in sorted(per.items()):
        lines.append(json.dumps({'what': 'png_encode_kernel', 'block': 64, 'kernel': short, 'launches': len(us), 'us_mean': round(float(np.mean(us)), 2),
                                 'us_min': round(min(us), 2), 'us_max': round(max(us), 2), 'share_of_kernels': round(sum(us) / launches / total, 3)}))
        print(lines[-1])
    lines.append(json.dumps({'what': 'png_encode_kernels_total', 'block': 64, 'us_per_call': round(total, 1), 'us_per_frame': round(total / 64, 2)}))
    print(lines[-1])
    with open(out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--blocks', type=int, nargs='*', default=[16, 50, 64, 256], help='frames per device call')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_encode_rate.jsonl'))
    ap.add_argument('--clip', type=int, default=None, metavar='SECONDS', help='time overlay and deploy --overlay_dir on a clip of this length instead')
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
    res = clip_run(args.clip) if args.clip else measure(args.frames, args.repeats, args.blocks)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
