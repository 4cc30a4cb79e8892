"""What the device-side feed of `deploy` costs and saves, on one box in one session:

  deploy      wall seconds of W2XYZ.deploy over a synthetic clip folder (made as tests/test_feeder.make_clip makes one: noise frames of
              224 x 448 in 8 levels, quality 95, a flow folder with float64 limits), decode='host' against decode='device', for an
              audio + video and an audio + video + flow model at batch 32 with --groups 10.  Each way runs once to warm up (page
              cache, code objects, the grouped contexts) and then `repeats` times; the line holds the median and every run.
  op          sagen_assemble_frames alone at 32 x 224 x 448 over 64 resident frames, modes 0 (uint8) and 2 (flow), with a roll per
              item: microseconds per call (device events around `calls` launches) and the achieved GB/s over the bytes the call
              reads and writes (3 in + 3 out per pixel in mode 0, 3 in + 12 out in mode 2)

    python tools/feed_rate.py [--secs 60] [--repeats 3] [--calls 200] [--only deploy|op] [--tag NAME] [--clip DIR] [--out profiles/feed_rate.jsonl]

A tree without the device feed (the parent commit) runs the `deploy` part with decode='host' only: --tag names the tree in the line, so
that the parent's deploy on the same clip stands next to the branch's.  One JSON line per measurement is printed and appended to --out."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_clip(root, secs, seed=0):
    """tests/test_feeder.make_clip(root, secs, flow=True)"""
    from PIL import Image
    from spatialaudiogen_amd import feeder as F
    r = np.random.Generator(np.random.PCG64(seed))
    for d in ('ambix', 'video', 'flow'):
        os.makedirs(os.path.join(root, d))
    audio = np.clip(0.3 * r.normal(size=(secs * 48000, 4)), -1, 1)
    for i in range(secs):
        F.save_wav(os.path.join(root, 'ambix', '%06d.wav' % i), audio[i * 48000:(i + 1) * 48000], 48000)
    with open(os.path.join(root, 'audio_pow.lst'), 'w') as f:
        for i in range((secs - 1) * 10):
            f.write('{} {}\n'.format(i / 10. + 0.5, 0.1 + 0.01 * i))
    frames = (r.integers(0, 256, size=(secs * 10, 224, 448, 3)).astype(np.uint8) // 32) * 32
    for i, fr in enumerate(frames):
        Image.fromarray(fr).save(os.path.join(root, 'video', '%06d.jpg' % i), quality=95)
        Image.fromarray(frames[(i * 7) % len(frames)]).save(os.path.join(root, 'flow', '%06d.jpg' % i), quality=95)
    np.save(os.path.join(root, 'flow', 'flow_limits.npy'), np.stack([np.zeros(secs * 10), np.linspace(1, 4, secs * 10)], 1))


class Params(object):
    ambi_order, audio_rate, video_rate, context, sample_dur = 1, 48000, 10, 1.0, 0.1
    separation, num_sep_tracks, fft_window = 'unet_mask', 32, 0.025
    context_units, freq_mask_units, loc_units = [64, 128, 128], [], [512, 512]

    def __init__(self, encoders):
        self.encoders = encoders


def measure_deploy(clip, secs, enc, repeats, tag, batch=32, groups=10):
    import inspect
    import torch
    from spatialaudiogen_amd.deploy import W2XYZ
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    P = init_weights(variable_specs(enc), seed=8, mode='test')
    ways = ['host', 'device'] if 'decode' in inspect.signature(W2XYZ.__init__).parameters else ['host']
    res = {'what': 'deploy', 'tree': tag, 'encoders': '+'.join(enc), 'clip_seconds': secs, 'batch': batch, 'groups': groups, 'repeats': repeats}
    outs = {}
    for way in ways:
        model = W2XYZ(params=Params(enc), variables=P, **({'decode': way} if len(ways) > 1 else {}))
        model.batch_size, model.groups = batch, groups
        s = []
        for k in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[way] = model.deploy(clip, 0., float(secs))
            torch.cuda.synchronize()
            s.append(time.perf_counter() - t0)
        n = outs[way].shape[0] // 4800
        res['windows'] = n
        res[way] = {'seconds': round(float(np.median(s[1:])), 4), 'windows_per_s': round(n / float(np.median(s[1:])), 1),
                    'first_run_seconds': round(s[0], 4), 'runs': [round(t, 4) for t in s[1:]]}
        del model
    if len(ways) > 1:
        res['same_bits'] = bool(np.array_equal(outs['host'].view(np.uint32), outs['device'].view(np.uint32)))
        res['device_over_host'] = round(res['host']['seconds'] / res['device']['seconds'], 3)
    return res


def measure_op(mode, calls, n_out=32, n_frames=64, h=224, w=448):
    import torch
    from spatialaudiogen_amd import _lib
    from spatialaudiogen_amd.ops import _ptr, _stream
    r = np.random.Generator(np.random.PCG64(mode))
    up = lambda a: torch.as_tensor(a).to('cuda')
    frames = up(r.integers(0, 256, size=(n_frames, h, w, 3)).astype(np.uint8))
    index, shift = up(r.integers(0, n_frames, size=n_out).astype(np.int32)), up(r.integers(-w, w, size=n_out).astype(np.int32))
    a = np.arange(256).astype(np.float32)
    a *= (2 * np.pi) / 255.
    table = up(np.concatenate([np.cos(a), np.sin(a)]))
    scale_lo = up(np.stack([np.linspace(1, 4, n_frames) / 255., np.zeros(n_frames)], 1))
    out = torch.empty((n_out, h, w, 3), dtype=torch.uint8 if mode == 0 else torch.float32, device='cuda')
    l = _lib.lib()

    def launch():
        _lib.check(l.sagen_assemble_frames(_ptr(frames), n_frames, h, w, _ptr(index), _ptr(shift), n_out, mode, _ptr(table), _ptr(scale_lo), _ptr(out),
                                           _stream()))
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            launch()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / calls)
    moved = n_out * h * w * (3 + (3 if mode == 0 else 12))
    med = float(np.median(us))
    return {'what': 'assemble_frames', 'mode': mode, 'n_out': n_out, 'n_frames': n_frames, 'h': h, 'w': w, 'calls': calls, 'bytes_moved': moved,
            'us_per_call': round(med, 2), 'us_runs': [round(u, 2) for u in sorted(us)], 'gb_per_s': round(moved / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--secs', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--only', choices=('deploy', 'op'), default=None)
    ap.add_argument('--tag', default='branch')
    ap.add_argument('--clip', default=None, help='the clip folder, made there if it does not exist and kept (default: a temporary one)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'feed_rate.jsonl'))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures the device: there is none'
    torch.cuda.set_device(0)
    lines = []

    def add(res):
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if args.only != 'op':
        with tempfile.TemporaryDirectory() as tmp:
            clip = args.clip or os.path.join(tmp, 'clip')
            if not os.path.isdir(clip):
                make_clip(clip, args.secs)
            for enc in (['audio', 'video'], ['audio', 'video', 'flow']):
                add(measure_deploy(clip, args.secs, enc, args.repeats, args.tag))
    if args.only != 'deploy':
        for mode in (0, 2):
            add(measure_op(mode, args.calls))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
