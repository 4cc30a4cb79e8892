"""Mono sources at known, moving positions -> a sound field, its "true" binaural signal and its true source maps, on the device: the
front end of the reference's ambisonics toolbox (AmbiEncoder, SourceBinauralizer, SphericalSourceVisualizer over MovingSource) as
three operations per audio sample (include/sagen.h: sagen_encode_sources, sagen_binauralize_sources, sagen_source_track;
csrc/sources.hip).

    python -m spatialaudiogen_amd.sources encode POSITION_FN AMBI_ORDER OUTPUT_FN [--rate 24000] [--base_dir DIR] [--overwrite] [--resample [QUALITY]]
    python -m spatialaudiogen_amd.sources binauralize INPUT_FN POSITION_FN OUTPUT_FN [--use_hrtfs --hrtf_dir DIR] [--overwrite] [--resample [QUALITY]]
    python -m spatialaudiogen_amd.sources encode_and_binauralize INPUT_FN POSITION_FN AMBI_ORDER OUTPUT_FN [--overwrite]
    ... encode_xyz INPUT_FN X Y Z AMBI_ORDER OUTPUT_FN | binauralize_xyz INPUT_FN X Y Z OUTPUT_FN [--use_hrtfs --hrtf_dir DIR] |
        encode_and_binauralize_xyz INPUT_FN X Y Z AMBI_ORDER OUTPUT_FN

(the surfaces of pyutils/ambisonics/scripts/encode_to_ambisonics.py, binauralize_sources.py, encode_and_binauralize.py and their
_xyz variants, which place one static source at a cartesian position).  `encode` reads a position file with a header per source
(read_position_file), the wavs relative to --base_dir (default: the position file's directory); the other two read one mono wav and a
plain file of `phi nu r` lines.  Every command takes --overwrite, --gpu N and --float (a 32-bit float wav instead of PCM16).  A wav
whose rate differs from --rate is refused, and so are HRIRs that are not at the rate of the input, unless --resample [best|fast] is
given: then they go through the device's polyphase resampler (resample.py).  Samples a source's trajectory does not cover (position.py:82:
nframes = int(duration * rate) can be one short of the signal) stay zero.
"""
import os

import numpy as np

from . import ambisonics


def read_position_file(fn):
    """(ids, control_points, wav_fns, img_fns, bg_img) of a position file (pyutils/iolib/position.py:6-33): per source a header
    `id wav [img] npts` followed by npts lines `phi nu r`; a `<BGI>name<BGI>` line names the background image; reading stops at the
    first empty line.  control_points[id] is a [npts, 3] float64 array (npts == 0: an ambient source).  A file that holds nothing but
    `phi nu r` lines - what binauralize_sources.py:16 reads - comes back as the one source 'source' with no wav."""
    ids, points, wavs, imgs, bg = [], {}, {}, {}, None

    def numbers(line):
        try:
            v = [float(t) for t in line.split()]
        except ValueError:
            return None
        return v if len(v) == 3 else None

    with open(fn, 'r') as f:
        lines = [l.strip() for l in f]
    body = [l for l in lines if l and not l.startswith('<BGI>')]
    if body and all(numbers(l) is not None for l in body):
        return ['source'], {'source': np.array([numbers(l) for l in body], np.float64)}, {}, {}, None
    i = 0
    while i < len(lines) and lines[i]:
        line = lines[i]
        i += 1
        if line.startswith('<BGI>'):
            bg = line.split('<BGI>')[1]
            continue
        s = line.split()
        if len(s) not in (3, 4):
            raise ValueError('%s: line %d is not a source header `id wav [img] npts`: %r' % (fn, i, line))
        sid, npts = s[0], int(s[-1])
        ids.append(sid)
        wavs[sid] = s[1]
        if len(s) == 4:
            imgs[sid] = s[2]
        rows = [numbers(l) for l in lines[i:i + npts]]
        if len(rows) != npts or any(r is None for r in rows):
            raise ValueError('%s: source %s announces %d control points `phi nu r`' % (fn, sid, npts))
        points[sid] = np.array(rows, np.float64).reshape(npts, 3)
        i += npts
    return ids, points, wavs, imgs, bg


def trajectory(control_points, n_samples, rate, samples):
    """(phi, nu, r) [len(samples), 3] of MovingSource.tic (position.py:73-102) at the given sample indices, in numpy on the host -
    the arithmetic the device evaluates per sample (include/sagen.h), kept here for the checks that belong on the host."""
    p = np.asarray(control_points, np.float64).reshape(-1, 3)
    P, i = len(p), np.asarray(samples, np.int64)
    duration = int(n_samples) / float(rate)
    nframes = int(duration * rate)
    if P == 1:
        return np.broadcast_to(p[0], (len(i), 3)).copy()
    idx = np.where(i == nframes - 1, P - 1, np.floor(i * ((P - 1) / float(max(nframes - 1, 1)))).astype(np.int64))
    idx = np.clip(idx, 0, P - 1)
    t = np.arange(P) * (duration / (P - 1))
    t[-1] = duration
    lo = np.minimum(idx, P - 2)
    al = ((i * (1. / float(rate)) - t[lo]) / (t[lo + 1] - t[lo]))[:, None]
    return np.where((idx == P - 1)[:, None], p[-1][None, :], al * p[lo + 1] + (1. - al) * p[lo])


class SourceScene(object):
    """Mono sources with their control points, resident on the device.  signals: one 1-D array per source (any lengths);
    control_points: one [P, 3] array of (phi, nu, r) per source - P == 0 marks an ambient source, which encode() adds to W
    (encode_to_ambisonics.py:50-52) and everything else ignores.  `length` is the number of samples every positioned source covers,
    min_s nframes_s: where the scripts' `while all(tic())` loop stops."""

    def __init__(self, signals, control_points, rate, device=None):
        import torch
        from . import ops
        if len(signals) != len(control_points) or not len(signals):
            raise ValueError('SourceScene: one signal and one control-point array per source expected')
        self.device, self.rate = ops.default_device(device), rate
        sig = [np.asarray(s, np.float32).reshape(-1) for s in signals]
        pts = [np.asarray(p, np.float64).reshape(-1, 3) for p in control_points]
        placed = [k for k in range(len(sig)) if len(pts[k])]
        if not placed:
            raise ValueError('SourceScene: at least one source needs a control point')
        if any(len(sig[k]) < 1 for k in placed):
            raise ValueError('SourceScene: a positioned source has no samples')
        self.control_points = [pts[k] for k in placed]
        self.lengths = [len(sig[k]) for k in placed]
        self.table = ops.SourceTable(self.control_points, self.lengths, rate, self.device)
        self.length = int(self.table.nframes.min())
        if self.length < 1:
            raise ValueError('SourceScene: a source is too short for one frame at this rate')
        buf = np.zeros((len(placed), max(self.lengths)), np.float32)
        for row, k in enumerate(placed):
            buf[row, :len(sig[k])] = sig[k]
        self.signals = torch.as_tensor(buf).to(self.device)
        self.ambient = [torch.as_tensor(sig[k]).to(self.device) for k in range(len(sig)) if not len(pts[k])]

    def _range(self, t0, n):
        t0 = int(t0)
        n = self.length - t0 if n is None else int(n)
        if t0 < 0 or n < 1 or t0 + n > self.length:
            raise ValueError('samples %d..%d requested; the sources cover 0..%d' % (t0, t0 + n - 1, self.length - 1))
        return t0, n

    def encode(self, order, t0=0, n=None, distance_model=False, radius=1.):
        """[n, (order + 1)^2] float32 ambisonics (ACN / SN3D) of the samples t0 .. t0 + n - 1.  distance_model: encode_v2's delay and
        attenuation from the surface of a sphere of `radius`, per sample."""
        from . import ops
        t0, n = self._range(t0, n)
        if distance_model:
            if not radius > 0:
                raise ValueError('encode: distance_model needs radius > 0')
            at = np.arange(t0, t0 + n)
            for s, (p, N) in enumerate(zip(self.control_points, self.lengths)):
                if (np.abs(trajectory(p, N, self.rate, at)[:, 2]) <= radius).any():          # encoder.py:42-43
                    raise ValueError('encode: source %d comes within the radius %g of the origin' % (s, radius))
        ambi = ops.encode_sources(self.signals, self.table, ambisonics.num_channels(order), t0, n, distance_model, radius)
        for a in self.ambient:                      # one add per ambient source, on W only
            m = min(n, max(0, a.shape[0] - t0))
            ambi[:m, 0] += a[t0:t0 + m]
        return ambi

    def binauralize(self, mode, hrir=None, static=False, t0=0, n=None):
        """[n, 2] float32 (left, right).  mode 'mic': VirtualStereoMic; 'hrir': Convolvotron with a render.HrirSet, the closest
        response re-chosen per sample.  static: the form of Convolvotron.binauralize (a 'valid' convolution: the first K - 1 samples
        are zero) instead of binauralize_frame."""
        from . import ops
        import torch
        t0, n = self._range(t0, n)
        if mode == 'mic':
            return ops.binauralize_sources(self.signals, self.table, 'mic', t0, n)
        if mode != 'hrir':
            raise ValueError("binauralize: mode 'mic' or 'hrir' expected")
        if hrir is None:
            raise ValueError("the 'hrir' mode needs a render.HrirSet")
        if int(hrir.rate) != int(self.rate):
            raise ValueError('the HRIRs are sampled at %d Hz, the sources at %d Hz (no resampler available offline)' % (hrir.rate, self.rate))
        if getattr(self, '_hrir_of', None) is not hrir:
            taps = np.stack([hrir.left, hrir.right], 1).astype(np.float32)          # [D, 2, K]
            self._hrir_dev = (torch.as_tensor(hrir.directions).contiguous().to(self.device), torch.as_tensor(taps).contiguous().to(self.device))
            self._hrir_of = hrir
        dirs, taps = self._hrir_dev
        return ops.binauralize_sources(self.signals, self.table, 'hrir', t0, n, dirs, taps, hrir.ntaps - 1 if static else 0)

    def directions(self, stride=1):
        """[ceil(length / stride), S, 3] float64 unit directions of the samples 0, stride, 2 stride, ..."""
        from . import ops
        return ops.source_track(self.table, 0, -(-self.length // int(stride)), int(stride))[0]

    def source_maps(self, duration, rate=10., angular_res=5):
        """The maps of SphericalSourceVisualizer (distance.py:62-97): [n_frames, mh, mw] float64 with 1 / S added per source at the
        node of ambisonics.spherical_mesh(angular_res) closest to it, one frame per 1 / rate seconds of a trajectory that lasts
        `duration` seconds - the reference's (unflipped) mesh orientation."""
        import torch
        from . import ops
        phi, nu = ambisonics.spherical_mesh(angular_res)
        mesh = np.stack([np.cos(nu) * np.cos(phi), np.cos(nu) * np.sin(phi), np.sin(nu)], -1).reshape(-1, 3)
        S = len(self.control_points)
        table = ops.SourceTable(self.control_points, [int(duration * rate)] * S, rate, self.device)
        n_frames = int(table.nframes.min())
        if n_frames < 1:
            return np.zeros((0,) + phi.shape)
        near = ops.source_track(table, 0, n_frames, 1, torch.as_tensor(mesh).to(self.device), unit=False)[1].cpu().numpy()
        flat = (np.arange(n_frames)[:, None] * mesh.shape[0] + near).reshape(-1)
        return (np.bincount(flat, minlength=n_frames * mesh.shape[0]) / float(S)).reshape((n_frames,) + phi.shape)


# ---- command lines ------------------------------------------------------------------------------------------------------------
def _mono(fn, rate=None, resample=None):
    from .feeder import load_wav
    try:
        data, file_rate = load_wav(fn, rate, resample)
    except ValueError as e:
        raise SystemExit('sources: %s' % e)
    return data[:, 0], file_rate            # (the scripts keep the first channel of a file that is not mono)


def _plain_positions(fn):
    ids, points, wavs, _, _ = read_position_file(fn)
    if wavs or len(ids) != 1:
        raise SystemExit('sources: %s must hold `phi nu r` lines only' % fn)
    return points[ids[0]]


def _xyz_position(args):
    xyz = np.array([args.x, args.y, args.z], np.float64)
    phi, nu = ambisonics.to_polar(xyz)
    return np.array([[phi, nu, np.linalg.norm(xyz)]])


def _subtype(args):
    return 'FLOAT' if args.float_wav else 'PCM_16'


def _padded(y, rows):
    out = np.zeros((rows, y.shape[1]), np.float32)
    out[:y.shape[0]] = y
    return out


def run_encode(args):
    from .feeder import save_wav
    ids, points, wavs, _, _ = read_position_file(args.position_fn)
    if not wavs:
        raise SystemExit('sources encode: %s names no wav per source (header `id wav [img] npts`)' % args.position_fn)
    base = args.base_dir if args.base_dir is not None else os.path.dirname(os.path.abspath(args.position_fn))
    data = [_mono(os.path.join(base, wavs[k]), args.rate, args.resample)[0] for k in ids]
    scene = SourceScene(data, [points[k] for k in ids], args.rate)
    rows = max(len(d) for d in data)
    ambix = _padded(scene.encode(args.ambi_order).cpu().numpy(), rows).astype(np.float64)
    for d, k in zip(data, ids):               # what of an ambient source lies past the positioned ones
        if not len(points[k]):
            ambix[scene.length:len(d), 0] += d[scene.length:]
    ambix = ambix / ambix.max() * 0.95        # encode_to_ambisonics.py:53: the maximum, not the absolute maximum
    save_wav(args.output_fn, ambix, args.rate, subtype=_subtype(args))
    return ambix


def _single_source(args):
    mono, rate = _mono(args.input_fn)
    pts = _xyz_position(args) if args.command.endswith('_xyz') else _plain_positions(args.position_fn)
    return SourceScene([mono], [pts], rate), mono.shape[0], rate, len(pts) == 1


def run_binauralize(args):
    from .feeder import save_wav
    from .render import HrirSet
    hrir = None
    if args.use_hrtfs:
        if not args.hrtf_dir:
            raise SystemExit('sources binauralize: --use_hrtfs needs --hrtf_dir')
        try:
            hrir = HrirSet.from_cipic_dir(args.hrtf_dir)
        except (ValueError, IOError) as e:
            raise SystemExit('sources binauralize: %s' % e)
    scene, rows, rate, static = _single_source(args)
    if hrir is not None and args.resample is not None:
        hrir = hrir.resampled(rate, args.resample, scene.device)
    try:
        y = scene.binauralize('hrir' if args.use_hrtfs else 'mic', hrir, static=static)
    except ValueError as e:
        raise SystemExit('sources binauralize: %s' % e)
    stereo = _padded(y.cpu().numpy(), rows)
    save_wav(args.output_fn, stereo, rate, subtype=_subtype(args))
    return stereo


def run_encode_and_binauralize(args, binauralize=True):
    from .feeder import save_wav
    from .render import Renderer, taps_ears
    scene, rows, rate, _ = _single_source(args)
    ambi = scene.encode(args.ambi_order)
    if binauralize:                           # DirectAmbisonicBinauralizer(fmt, method='projection') (encode_and_binauralize.py:35-37)
        ambi = Renderer(taps_ears(args.ambi_order, 'projection'), device=scene.device).process(ambi)
    out = _padded(ambi.cpu().numpy(), rows)
    save_wav(args.output_fn, out, rate, subtype=_subtype(args))
    return out


def parse_arguments(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = parser.add_subparsers(dest='command')
    sub.required = True

    def add(name, *positional):
        p = sub.add_parser(name)
        for a in positional:
            if a == 'ambi_order':
                p.add_argument(a, type=int, help='Ambisonics order (1 or 2).')
            elif a in ('x', 'y', 'z'):
                p.add_argument(a, type=float, help='%s coordinate.' % a)
            else:
                p.add_argument(a)
        p.add_argument('--overwrite', action='store_true', help='Whether to overwrite the output file.')
        p.add_argument('--gpu', type=int, default=0, help='GPU id')
        from .resample import add_quality_flag
        add_quality_flag(p, '--resample', 'resample mono wavs (encode: to --rate) and HRIRs (binauralize: to the rate of the input) on the device')
        p.add_argument('--float', dest='float_wav', action='store_true', help='Write a 32-bit float wav instead of 16-bit PCM.')
        return p

    p = add('encode', 'position_fn', 'ambi_order', 'output_fn')
    p.add_argument('--rate', default=24000, type=int, help='Frame rate.')
    p.add_argument('--base_dir', default=None, help='Directory the wav names of the position file are relative to.')
    for name in ('binauralize', 'binauralize_xyz'):
        p = add(name, *(('input_fn', 'position_fn', 'output_fn') if name == 'binauralize' else ('input_fn', 'x', 'y', 'z', 'output_fn')))
        p.add_argument('--use_hrtfs', action='store_true', help='Whether to use hrtfs.')
        p.add_argument('--hrtf_dir', default='', help='Input hrtf directory (CIPIC layout).')
    add('encode_and_binauralize', 'input_fn', 'position_fn', 'ambi_order', 'output_fn')
    add('encode_xyz', 'input_fn', 'x', 'y', 'z', 'ambi_order', 'output_fn')
    add('encode_and_binauralize_xyz', 'input_fn', 'x', 'y', 'z', 'ambi_order', 'output_fn')
    return parser.parse_args(argv)


def main(argv=None):
    from . import ops
    args = parse_arguments(argv)
    if os.path.exists(args.output_fn) and not args.overwrite:
        raise SystemExit('sources: %s exists (--overwrite)' % args.output_fn)
    if getattr(args, 'ambi_order', 1) not in (1, 2):
        raise SystemExit('sources: ambisonic order %d is not supported (1 or 2)' % args.ambi_order)
    ops.select_device(args.gpu)
    if args.command == 'encode':
        out = run_encode(args)
    elif args.command.startswith('binauralize'):
        out = run_binauralize(args)
    else:
        out = run_encode_and_binauralize(args, binauralize=args.command.startswith('encode_and'))
    print('wrote %s: %d samples x %d channels (%s)' % (args.output_fn, out.shape[0], out.shape[1], args.command))


if __name__ == '__main__':
    main()
