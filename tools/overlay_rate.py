"""Cost of the power-map overlay on the device (csrc/overlay.hip), with device events after warm-up:

  - the 5-degree maps of a 10 s stream (480 000 rows, stride 5, 20 windows of 4800) at orders 1 and 2;
  - the blend of 100 frames of 224 x 448 over 37 x 72 maps: time, and the bytes/s of frames read + frames written;
  - W2XYZ.deploy_and_overlay against W2XYZ.deploy on the same seeded 60 s audio + video clip (--groups 10), alternating regions;
  - tests/overlay_oracle.py on the host for the same maps and frames: the thing replaced.

    python tools/overlay_rate.py [--reps 20] [--regions 3] [--no-host] [--no-deploy]       # one JSON line per measurement
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/overlay_rate.py --trace-run
    python tools/overlay_rate.py --digest DIR                                             # the overlay kernels of that trace

--trace-run performs 8 calls (3 warm-up + 5) of the maps at both orders and of the 100-frame blend, and nothing else."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ROWS, FRAMES, H, W = 480000, 100, 224, 448


def inputs(channels, seed=7):
    r = np.random.RandomState(seed)
    x = (0.3 * r.normal(size=(ROWS, channels))).astype(np.float32)
    frames = r.randint(0, 256, size=(FRAMES, H, W, 3)).astype(np.uint8)
    maps = (0.05 + r.uniform(size=(FRAMES // 5 + 1, 37, 72))).astype(np.float32)
    return x, frames, maps


def timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def digest(trace_dir):
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_stats.csv'), recursive=True)
    assert files, 'no kernel_stats.csv under %s' % trace_dir
    rows = [r for r in csv.DictReader(open(files[0])) if 'overlay_' in r['Name']]
    out = ['# rocprofv3 --kernel-trace --stats -- python tools/overlay_rate.py --trace-run   (1x MI355X)',
           '# 8 calls each of: the 5-degree maps of a 10 s stream (20 windows of 4800 samples at stride 5, 2664 nodes) at 4 and at 9 channels,',
           '# and the blend of 100 frames of 224 x 448 over 37 x 72 maps (grid pass: 100 workgroups; pixel pass: 1 x 224 x 100 of 128 threads)',
           '# kernel | calls | total us | mean us | min us | max us']
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs'])):
        out.append('%s | %s | %.1f | %.2f | %.2f | %.2f' % (r['Name'][:120], r['Calls'], float(r['TotalDurationNs']) * 1e-3, float(r['AverageNs']) * 1e-3,
                                                            float(r['MinNs']) * 1e-3, float(r['MaxNs']) * 1e-3))
    for r in rows:
        if 'overlay_pixel_kernel' in r['Name']:
            byts = 2. * FRAMES * H * W * 3
            out.append('# pixel pass: %.1f MB of frames read + written per call -> %.2f TB/s at the mean, %.2f TB/s at the best call'
                       % (byts * 1e-6, byts / float(r['AverageNs']) * 1e-3, byts / float(r['MinNs']) * 1e-3))
    print('\n'.join(out))


class Params(object):
    ambi_order, audio_rate, video_rate, context, sample_dur = 1, 48000, 10, 1.0, 0.1
    separation, num_sep_tracks, fft_window = 'unet_mask', 32, 0.025
    context_units, freq_mask_units, loc_units = [64, 128, 128], [], [512, 512]
    encoders = ['audio', 'video']


def deploy_rates(regions):
    import torch
    from spatialaudiogen_amd import overlay
    from spatialaudiogen_amd.deploy import W2XYZ, ClipArrays
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    secs = 60
    r = np.random.Generator(np.random.PCG64(60))
    audio = (0.3 * r.normal(size=(secs * 48000, 4))).astype(np.float32)
    video = r.integers(0, 256, size=(secs * 10, 224, 448, 3), dtype=np.uint8)
    model = W2XYZ(params=Params(), variables=init_weights(variable_specs(Params.encoders), seed=4, mode='test'))
    model.groups = 10
    ov = overlay.Overlay(4)
    clip = lambda: ClipArrays(audio, video, frames=video)
    plain = lambda: model.deploy(clip(), 0., None)
    painted = lambda: model.deploy_and_overlay(clip(), 0., None, ov)[0]
    for fn in (plain, painted):
        n = fn().shape[0]
    rates = {'plain': [], 'overlay': []}
    for i in range(regions):
        for name, fn in (('plain', plain), ('overlay', painted)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            rates[name].append(2 * n / 48000. / (time.perf_counter() - t0))
    res = {'what': 'deploy_and_overlay vs deploy, 60 s audio + video clip, groups 10 (the painted frames are copied to the host as well)',
           'regions': regions}
    for name, v in rates.items():
        res[name + '_ambisonic_s_per_s'] = {'median': round(float(np.median(v)), 1), 'min': round(min(v), 1), 'max': round(max(v), 1)}
    res['overlay_over_plain_median'] = round(res['overlay_ambisonic_s_per_s']['median'] / res['plain_ambisonic_s_per_s']['median'], 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--no-deploy', action='store_true')
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--digest', default=None)
    args = ap.parse_args()
    if args.digest:
        return digest(args.digest)
    import torch
    from spatialaudiogen_amd import ops, overlay
    torch.cuda.set_device(0)
    lut = torch.as_tensor(overlay.ylorrd_table()).cuda()
    work = {}
    for channels in (4, 9):
        x, frames, maps = inputs(channels)
        sh = torch.as_tensor(overlay.overlay_sh({4: 1, 9: 2}[channels]).astype(np.float32)).cuda()
        xd = torch.as_tensor(x).cuda()
        out = torch.empty(ROWS // 5 // 4800, sh.shape[0], dtype=torch.float32, device='cuda')
        work[channels] = lambda xd=xd, sh=sh, out=out: ops.power_map_windows(xd, sh, 5, 4800, out=out)
    fd, md = torch.as_tensor(frames).cuda(), torch.as_tensor(maps).cuda()
    blend = lambda: ops.overlay_blend(md, 0, lut, fd, 0, 5)
    if args.trace_run:
        for _ in range(8):
            work[4](); work[9](); blend()
        torch.cuda.synchronize()
        print('trace run: 8 calls each')
        return
    for channels in (4, 9):
        ms = timed(work[channels], args.reps)
        print(json.dumps({'what': '5-degree maps of a 10 s stream', 'channels': channels, 'maps': 20, 'nodes': 2664, 'rows_read': ROWS // 5,
                          'ms': round(ms, 4)}), flush=True)
    ms = timed(blend, args.reps)
    byts = 2. * FRAMES * H * W * 3
    print(json.dumps({'what': 'blend of 100 frames of 224x448 over 37x72 maps (grid pass + pixel pass + output allocation)', 'ms': round(ms, 4),
                      'frame_MB_read_and_written': round(byts * 1e-6, 1), 'TB_per_s': round(byts / ms * 1e-9, 3)}), flush=True)
    if not args.no_deploy:
        deploy_rates(args.regions)
    if not args.no_host:
        import overlay_oracle as OO
        x, frames, maps = inputs(4)
        t0 = time.perf_counter()
        OO.maps(x, 1)
        t_maps = time.perf_counter() - t0
        t0 = time.perf_counter()
        OO.blend(maps, frames, OO.ylorrd_table(), 5)
        print(json.dumps({'what': 'tests/overlay_oracle.py on the host (numpy fp64, one process)', 'maps_order1_ms': round(t_maps * 1e3, 1),
                          'blend_100_frames_ms': round((time.perf_counter() - t0) * 1e3, 1)}), flush=True)


if __name__ == '__main__':
    main()
