"""What the device-side audio feed costs and saves, on one box in one session:

  op          sagen_assemble_audio alone over a resident 60 s int16 clip of 4 channels: 16 x 52799 windows with mono + target (one
              forward call of evaluate) and 320 x 52799 mono only (one grouped call of deploy at batch 32, --groups 10), consecutive
              windows 4800 samples apart: microseconds per call (device events around `calls` launches, five times) and the achieved
              GB/s over the bytes the call writes, and over those it reads and writes (8 per window row in)
  evaluate    wall seconds of evaluate() from clip folders - a synthetic database of `--clips` clips of `--clip_secs` seconds, every
              10th window, of whose frames only the ones those windows name exist -, decode='host' against decode='device', for an
              audio + video and an audio + video + flow model, with groups 1 and 10 (--groups).  Each way runs once to warm up (page cache, code
              objects, grouped contexts) and then `repeats` times; the line holds the median and every run, and whether the two
              eval-detailed.txt are the same text
  deploy      wall seconds of W2XYZ.deploy over the 60 s clip folder of tools/feed_rate.py at batch 32 with --groups 10, decode='host'
              against decode='device', as that tool measures them (the same function): on a tree that has the device feed of the
              frames but not this one of the audio (the parent commit) it gives that tree's figures, --tag names the tree

    python tools/audio_feed_rate.py [--groups 1 10] [--repeats 3] [--calls 200] [--only op|evaluate|deploy] [--tag NAME] [--clip DIR] [--out profiles/audio_feed_rate.jsonl]

One JSON line per measurement is printed and appended to --out."""
import argparse
import inspect
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from feed_rate import Params, make_clip, measure_deploy  # noqa: E402

SIZE, RATE = 52799, 48000


def measure_op(n_out, want, calls, secs=60):
    import torch
    from spatialaudiogen_amd import _lib
    from spatialaudiogen_amd.ops import _ptr, _stream
    r = np.random.Generator(np.random.PCG64(n_out))
    up = lambda a: torch.as_tensor(a).to('cuda')
    samples = up(r.integers(-32768, 32768, size=(secs * RATE, 4)).astype(np.int16))
    lead = up(np.zeros(n_out, np.int32))
    read_from = up((4800 * np.arange(n_out)).astype(np.int64))
    count = up(np.full(n_out, SIZE, np.int32))
    mono = torch.empty((n_out, SIZE), dtype=torch.float32, device='cuda') if 'mono' in want else None
    target = torch.empty((n_out, 4800, 3), dtype=torch.float32, device='cuda') if 'target' in want else None
    full = torch.empty((n_out, SIZE, 4), dtype=torch.float32, device='cuda') if 'full' in want else None
    l = _lib.lib()

    def launch():
        _lib.check(l.sagen_assemble_audio(_ptr(samples), 0, int(samples.shape[0]), 4, _ptr(lead), _ptr(read_from), _ptr(count), None, n_out, SIZE,
                                          24000, 4800, _ptr(full), _ptr(mono), _ptr(target), _stream()))
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
    written = sum(4 * t.numel() for t in (full, mono, target) if t is not None)
    read = n_out * SIZE * 8
    med = float(np.median(us))
    return {'what': 'assemble_audio', 'n_out': n_out, 'size': SIZE, 'channels': 4, 'sample_type': 'int16', 'outputs': '+'.join(want), 'calls': calls,
            'bytes_written': written, 'bytes_read': read, 'us_per_call': round(med, 2), 'us_runs': [round(u, 2) for u in sorted(us)],
            'written_gb_per_s': round(written / med / 1e3, 1), 'moved_gb_per_s': round((written + read) / med / 1e3, 1)}


def make_eval_db(root, clips, secs, seed=0):
    """clip folders for evaluate: wav pieces, the window list, and of the frames only those every 10th window names (5, 15, ...)"""
    from PIL import Image
    from spatialaudiogen_amd import feeder as F
    r = np.random.Generator(np.random.PCG64(seed))
    for c in range(clips):
        clip = os.path.join(root, 'clip%02d' % c)
        for d in ('ambix', 'video', 'flow'):
            os.makedirs(os.path.join(clip, d))
        audio = np.clip(0.3 * r.normal(size=(secs * RATE, 4)), -1, 1)
        for i in range(secs):
            F.save_wav(os.path.join(clip, 'ambix', '%06d.wav' % i), audio[i * RATE:(i + 1) * RATE], RATE)
        with open(os.path.join(clip, 'audio_pow.lst'), 'w') as f:
            for i in range((secs - 1) * 10):
                f.write('{} {}\n'.format(i / 10. + 0.5, 0.1 + 0.01 * i))
        for i in range(5, (secs - 1) * 10, 10):
            for d in ('video', 'flow'):
                fr = (r.integers(0, 256, size=(224, 448, 3)).astype(np.uint8) // 32) * 32
                Image.fromarray(fr).save(os.path.join(clip, d, '%06d.jpg' % i), quality=95)
        np.save(os.path.join(clip, 'flow', 'flow_limits.npy'), np.stack([np.zeros(secs * 10), np.linspace(1, 4, secs * 10)], 1))


def measure_evaluate(db, enc, groups, repeats, tag, tmp):
    import torch
    from spatialaudiogen_amd.evaluate import evaluate
    from spatialaudiogen_amd.weights import variable_specs, init_weights
    P = init_weights(variable_specs(enc), seed=8, mode='test')
    res = {'what': 'evaluate', 'tree': tag, 'encoders': '+'.join(enc), 'groups': groups, 'repeats': repeats}
    text = {}
    for way in ('host', 'device'):
        model_dir = os.path.join(tmp, 'model_%s_%d_%s' % ('_'.join(enc), groups, way))
        os.makedirs(model_dir)
        s = []
        for k in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, count = evaluate(model_dir, db, None, None, variables=P, params=Params(enc), groups=groups, decode=way)
            torch.cuda.synchronize()
            s.append(time.perf_counter() - t0)
        text[way] = open(os.path.join(model_dir, 'eval-detailed.txt')).read()
        med = float(np.median(s[1:]))
        res['windows'] = count
        res[way] = {'seconds': round(med, 4), 'windows_per_s': round(count / med, 1), 'first_run_seconds': round(s[0], 4),
                    'runs': [round(t, 4) for t in s[1:]]}
    res['same_text'] = text['host'] == text['device']
    res['device_over_host'] = round(res['host']['seconds'] / res['device']['seconds'], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--secs', type=int, default=60, help='seconds of the deploy clip')
    ap.add_argument('--clips', type=int, default=4)
    ap.add_argument('--clip_secs', type=int, default=81, help='seconds of each clip of the evaluate database (81 -> 80 windows)')
    ap.add_argument('--groups', type=int, nargs='+', default=[1, 10], help='the --groups values of the evaluate part')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--only', choices=('op', 'evaluate', 'deploy'), default=None)
    ap.add_argument('--tag', default='branch')
    ap.add_argument('--clip', default=None, help='the deploy clip folder, made there if it does not exist and kept (default: a temporary one)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'audio_feed_rate.jsonl'))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures the device: there is none'
    torch.cuda.set_device(0)
    from spatialaudiogen_amd import _lib
    from spatialaudiogen_amd.evaluate import evaluate
    has_op = 'sagen_assemble_audio' in _lib.SIGNATURES
    lines = []

    def add(res):
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if args.only in (None, 'op') and has_op:
        add(measure_op(16, ('mono', 'target'), args.calls))
        add(measure_op(320, ('mono',), args.calls))
    with tempfile.TemporaryDirectory() as tmp:
        if args.only in (None, 'evaluate') and 'decode' in inspect.signature(evaluate).parameters:
            db = os.path.join(tmp, 'db')
            make_eval_db(db, args.clips, args.clip_secs)
            for enc in (['audio', 'video'], ['audio', 'video', 'flow']):
                for groups in args.groups:
                    add(measure_evaluate(db, enc, groups, args.repeats, args.tag, tmp))
        if args.only in (None, 'deploy'):
            clip = args.clip or os.path.join(tmp, 'clip')
            if not os.path.isdir(clip):
                make_clip(clip, args.secs)
            for enc in (['audio', 'video'], ['audio', 'video', 'flow']):
                res = measure_deploy(clip, args.secs, enc, args.repeats, args.tag)
                res['audio_on_device'] = has_op
                add(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
