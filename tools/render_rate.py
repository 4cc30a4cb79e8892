"""Cost of rendering on the device: W2XYZ.deploy (--groups 10) with and without the HRIR rendering, on a seeded 60 s audio + video
clip and a seeded HRIR set (nothing is read from disk).

    python tools/render_rate.py [--regions 5] [--clips 8]   # end-to-end rate, alternating plain / rendered regions of --clips deploys each,
                                                            # one JSON line per region + a summary, then the kernel alone per tap table
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/render_rate.py --trace-run
    python tools/render_rate.py --digest DIR            # the render kernel against the forward kernels in that trace

--trace-run performs two deploy_and_render calls over the clip (59 s of ambisonics each) and nothing else."""
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

SECS, TRACE_CALLS = 60, 2
NOT_FORWARD = ('render_fir_kernel', 'assemble_wyzx_kernel', '__amd_rocclr', 'at::native')    # everything else in the trace is the forward


class Params(object):                     # what train-params.txt of an audio + video model holds (deploy.load_params)
    ambi_order, audio_rate, video_rate, context, sample_dur = 1, 48000, 10, 1.0, 0.1
    separation, num_sep_tracks, fft_window = 'unet_mask', 32, 0.025
    context_units, freq_mask_units, loc_units = [64, 128, 128], [], [512, 512]
    encoders = ['audio', 'video']


def seeded_hrirs(seed=41, ntaps=200):
    """A stand-in for a measured CIPIC set: decaying random responses at the set's 23 x 50 directions."""
    from spatialaudiogen_amd import render as R
    r = np.random.RandomState(seed)
    env = np.exp(-np.arange(ntaps) / (ntaps / 6.))
    dirs = [(np.cos(e) * np.cos(a), -np.cos(e) * np.sin(a), np.sin(e)) for a in np.radians(R.CIPIC_AZIMUTHS) for e in np.radians(R.CIPIC_ELEVATIONS)]
    left, right = 0.3 * r.normal(size=(len(dirs), ntaps)) * env, 0.3 * r.normal(size=(len(dirs), ntaps)) * env
    return R.HrirSet(np.array(dirs), left, right, 48000)


def setup():
    import torch
    from spatialaudiogen_amd import render as R
    from spatialaudiogen_amd.deploy import W2XYZ, ClipArrays
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    torch.cuda.set_device(0)
    r = np.random.Generator(np.random.PCG64(60))
    audio = (0.3 * r.normal(size=(SECS * 48000, 4))).astype(np.float32)
    video = r.integers(0, 256, size=(SECS * 10, 224, 448, 3), dtype=np.uint8)
    model = W2XYZ(params=Params(), variables=init_weights(variable_specs(Params.encoders), seed=4, mode='test'))
    model.groups = 10
    taps, zb = R.build_taps('hrir', 1, 48000, hrir=seeded_hrirs())
    return model, (lambda: ClipArrays(audio, video)), R.Renderer(taps, zb)


def digest(trace_dir):
    """Per 10 s of ambisonics: the render kernel's time, its FLOP and bytes from the shapes, its share of the fp32 vector rate
    without packed instructions (256 CUs x 4 SIMDs x 16 lanes x 2 FLOP x 2.4 GHz = 78.6 TFLOP/s, half the 157.3 TFLOP/s the
    v_pk_fma_f32 peak quotes: this library may not use packed fp32), and the forward kernels' time in the same trace."""
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_stats.csv'), recursive=True)
    assert files, 'no kernel_stats.csv under %s' % trace_dir
    rows = list(csv.DictReader(open(files[0])))
    tot = lambda pred: sum(float(r['TotalDurationNs']) for r in rows if pred(r['Name'])) * 1e-3
    calls = lambda pred: sum(int(r['Calls']) for r in rows if pred(r['Name']))
    is_render = lambda n: 'render_fir_kernel' in n
    is_forward = lambda n: not any(k in n for k in NOT_FORWARD)
    audio_s = TRACE_CALLS * (SECS - 1)                    # 590 windows of 0.1 s per call
    per10 = 10. / audio_s
    C, O, K = 4, 2, 200
    flop = 2. * O * C * K * 480000
    byts = 480000 * (C + O) * 4.
    out = ['# rocprofv3 --kernel-trace --stats -- python tools/render_rate.py --trace-run   (1x MI355X)',
           '# %d deploy_and_render calls, --groups 10, hrir rendering (C = 4, O = 2, K = 200), 60 s audio + video clip: %d s of ambisonics' % (TRACE_CALLS, audio_s),
           'render_fir_kernel: %d calls, %.1f us total' % (calls(is_render), tot(is_render)),
           'forward kernels: %d calls, %.1f us total' % (calls(is_forward), tot(is_forward))]
    r10, f10 = tot(is_render) * per10, tot(is_forward) * per10
    out += ['per 10 s of ambisonics: render %.1f us, forward %.1f us, render / forward = %.2f %% (condition: <= 10 %%)' % (r10, f10, 100. * r10 / f10),
            'render per 10 s: %.3f GFLOP, %.2f MB (x + y, shapes) -> %.2f TFLOP/s = %.1f %% of 78.6 TFLOP/s (fp32 VALU without packed '
            'instructions; 157.3 TFLOP/s is the v_pk_fma_f32 peak), %.1f GB/s' % (flop * 1e-9, byts * 1e-6, flop / r10 * 1e-6, 100. * flop / r10 * 1e-6 / 78.6,
                                                                                 byts / r10 * 1e-3),
            '# kernel | calls | total us | mean us | min us | max us']
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:24]:
        out.append('%s | %s | %.1f | %.2f | %.2f | %.2f' % (r['Name'][:120], r['Calls'], float(r['TotalDurationNs']) * 1e-3, float(r['AverageNs']) * 1e-3,
                                                            float(r['MinNs']) * 1e-3, float(r['MaxNs']) * 1e-3))
    print('\n'.join(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--clips', type=int, default=8, help='deploys of the 60 s clip per timed region')
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--digest', default=None)
    args = ap.parse_args()
    if args.digest:
        return digest(args.digest)
    import torch
    model, clip, renderer = setup()
    if args.trace_run:
        for _ in range(TRACE_CALLS):
            ambi, ren = model.deploy_and_render(clip(), 0., None, renderer)
        torch.cuda.synchronize()
        print('trace run: %d calls, ambi %s rendered %s' % (TRACE_CALLS, ambi.shape, ren.shape))
        return
    plain = lambda: model.deploy(clip(), 0., None)
    rendered = lambda: model.deploy_and_render(clip(), 0., None, renderer)[0]
    for fn in (plain, rendered):                  # warm-up: contexts, plans, pinned buffers
        n = fn().shape[0]
    rates = {'plain': [], 'render_hrir': []}
    for i in range(args.regions):
        for name, fn in (('plain', plain), ('render_hrir', rendered)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.clips):
                fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rates[name].append(args.clips * n / 48000. / dt)
            print(json.dumps({'region': i, 'mode': name, 'clips': args.clips, 'seconds': round(dt, 4), 'ambisonic_s_per_s': round(rates[name][-1], 1)}), flush=True)
    summ = {'summary': True, 'clip_s': SECS, 'groups': 10, 'regions': args.regions, 'clips_per_region': args.clips}
    for name, v in rates.items():
        summ[name] = {'median': round(float(np.median(v)), 1), 'min': round(min(v), 1), 'max': round(max(v), 1)}
    summ['render_over_plain_median'] = round(summ['render_hrir']['median'] / summ['plain']['median'], 4)
    print(json.dumps(summ), flush=True)
    kernel_times()


def kernel_times(n=480000, reps=20):
    """The kernel alone (device events, one call of 10 s of audio) for each tap table: the output is stored 4 bytes at a time at
    stride O, so the wide tables (18 speaker feeds at order 2; O = 32, the widest the entry takes) are where that would show."""
    import torch
    from spatialaudiogen_amd import ops, render as R
    hset = seeded_hrirs()
    r = np.random.RandomState(1)
    cases = [('hrir', 1, None), ('hrir', 2, None), ('mic', 1, None), ('speakers', 1, None), ('speakers', 2, None),
             ('speakers-32', 2, r.normal(size=(32, 3)))]
    for mode, order, pos in cases:
        taps, zb = R.build_taps(mode.split('-')[0], order, 48000, hrir=hset, positions=pos)
        C = taps.shape[1]
        x = torch.as_tensor((0.2 * r.normal(size=(n, C))).astype(np.float32)).cuda()
        t = torch.as_tensor(taps.astype(np.float32)).cuda()
        for _ in range(3):
            ops.render_fir(x, 0, t, None, 4800, 0, zb)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.render_fir(x, 0, t, None, 4800, 0, zb)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        O, K = taps.shape[0], taps.shape[2]
        print(json.dumps({'kernel': mode, 'order': order, 'outputs': O, 'channels': C, 'taps': K, 'samples': n, 'us_per_call': round(us, 1),
                          'tflops': round(2. * O * C * K * n / us * 1e-6, 2), 'gb_per_s': round(n * (C + O) * 4. / us * 1e-3, 1)}), flush=True)

if __name__ == '__main__':
    main()
