"""Render ambisonics to something a person can listen to, on the device: the reference's output stage as ONE operation.

    python -m spatialaudiogen_amd.render IN_AMBIX.wav OUT.wav [--render {wy,ears,mic,hrir,speakers}] [--hrir_dir DIR]
           [--resample_hrir [QUALITY]] [--decode {projection,pseudoinv}] [--yaw DEG --pitch DEG --roll DEG] [--normalize PEAK] [--overwrite]

(the surface of pyutils/ambisonics/scripts/binauralize_ambisonics.py; the order is taken from the channel count, 4 or 9).

Every rendering the reference offers is a matrix of FIR filters applied to the (optionally rotated) ambisonic stream, so each is
a table of taps H [outputs, channels, taps] for the one kernel behind ops.render_fir (csrc/render.hip, include/sagen.h):

    wy        myutils.py:289                                 L = W + Y, R = W - Y                         (order 1 only)
    ears      DirectAmbisonicBinauralizer (binauralizer.py:156-166)   decode at the two ear positions (0, +-0.1, 0)
    speakers  AmbiDecoder.decode (decoder.py:24-28)          one output per loudspeaker
    mic       AmbisonicBinauralizer(use_hrtfs=False) -> VirtualStereoMic.binauralize (:18-36): ring of speakers, each delayed and
              attenuated per ear
    hrir      AmbisonicBinauralizer(use_hrtfs=True) -> Convolvotron.binauralize (:63-76): ring of speakers, each convolved with
              the closest HRIR pair; the first taps - 1 output samples are zero, as there

The speakers are folded into the taps on the host in fp64; the device sees fp32 taps.
"""
import os

import numpy as np

from . import ambisonics

SPEED_OF_SOUND = 343.                 # binauralizer.py:9
EAR_POSITIONS = np.array([[0., 0.1, 0.], [0., -0.1, 0.]])       # left, right (binauralizer.py:15-16, 162)
MODES = ('wy', 'ears', 'mic', 'hrir', 'speakers')
CIPIC_ELEVATIONS = (-45, -39, -34, -28, -23, -17, -11, -6, 0, 6, 11, 17, 23, 28, 34, 39, 45, 51, 56, 62, 68, 73, 79, 84, 90, 96, 101,
                    107, 113, 118, 124, 129, 135, 141, 146, 152, 158, 163, 169, 174, 180, 186, 191, 197, 203, 208, 214, 219, 225, 231)
CIPIC_AZIMUTHS = (-80, -65, -55, -45, -35, -30, -25, -20, -15, -10, -5, 0, 5, 10, 15, 20, 25, 30, 35, 45, 55, 65, 80)


def cipic_file_names(azimuth):
    """(left, right) file names of one azimuth (hrir.py:18-19)."""
    stem = ('neg' if azimuth < 0 else '') + str(abs(azimuth)) + 'az'
    return stem + 'left.wav', stem + 'right.wav'


class HrirSet(object):
    """Head-related impulse responses: directions [P, 3] (unit vectors, x front, y left, z up), left / right [P, K] impulse
    responses in time order, and their sample rate."""

    def __init__(self, directions, left, right, rate):
        self.directions = np.asarray(directions, np.float64)
        self.directions = self.directions / np.linalg.norm(self.directions, axis=1, keepdims=True)
        self.left, self.right = np.asarray(left, np.float64), np.asarray(right, np.float64)
        self.rate = int(rate)
        if not (self.left.shape == self.right.shape and self.left.shape[0] == self.directions.shape[0] and self.directions.shape[1] == 3):
            raise ValueError('HrirSet: directions [P, 3], left and right [P, K] expected')

    @property
    def ntaps(self):
        return self.left.shape[1]

    def closest(self, direction):
        """Index of the response closest to `direction` (any length): the maximum dot product with the unit directions, in fp64.
        The reference (hrir.py:35-41) leaves exact ties to a KD-tree, and its own loudspeaker ring has some: the speakers on the
        interaural axis are equally close to (az = -+80, el = 0) and (az = +-80, el = 180).  Here every candidate within 1e-12 of
        the maximum ties, and the LOWEST index wins (for a CIPIC set: azimuth-major, elevation-minor order)."""
        d = np.asarray(direction, np.float64).reshape(3)
        dots = self.directions @ (d / np.linalg.norm(d))
        return int(np.flatnonzero(dots >= dots.max() - 1e-12)[0])

    @classmethod
    def from_cipic_dir(cls, dirname):
        """The layout hrir.py:12-33 reads: per azimuth one `[neg]<az>azleft.wav` and one `...azright.wav`, each [samples, 50
        elevations]; the direction of (az, el) is (cos el cos az, -cos el sin az, sin el).  The reference flips each response
        when it loads it (hrir.py:20-21) and again when it uses it (binauralizer.py:70-71): a file's sample order IS the impulse
        response in time order."""
        from .feeder import load_wav
        if not os.path.isdir(dirname):
            raise IOError('HRIR directory %s does not exist' % dirname)
        dirs, left, right, rate = [], [], [], None
        for az in CIPIC_AZIMUTHS:
            fl, fr = cipic_file_names(az)
            (l, rl), (r, rr) = load_wav(os.path.join(dirname, fl)), load_wav(os.path.join(dirname, fr))
            if rate is None:
                rate = rl
            if rl != rate or rr != rate or l.shape != r.shape or l.shape[1] != len(CIPIC_ELEVATIONS):
                raise ValueError('%s: azimuth %d does not hold [samples, %d] responses at one rate' % (dirname, az, len(CIPIC_ELEVATIONS)))
            a = az * np.pi / 180.
            for j, el in enumerate(CIPIC_ELEVATIONS):
                e = el * np.pi / 180.
                dirs.append((np.cos(e) * np.cos(a), -np.cos(e) * np.sin(a), np.sin(e)))
                left.append(l[:, j])
                right.append(r[:, j])
        return cls(np.array(dirs), np.array(left), np.array(right), rate)

    def resampled(self, rate, quality='best', device=None):
        """The set at another sample rate: every response through resample.resample (the polyphase FIR of csrc/resample.hip, 64
        responses per call), scaled by rate_in / rate_out so that each response keeps its frequency response - an impulse response
        sampled more densely sums more samples per unit of time.  ceil(K L / M) taps."""
        from . import resample as R
        if int(rate) == self.rate:
            return self
        rows = np.concatenate([self.left, self.right], 0).T.astype(np.float32)               # [K, 2 P]
        out = [R.resample(np.ascontiguousarray(rows[:, i:i + 64]), self.rate, rate, quality=quality, device=device) for i in range(0, rows.shape[1], 64)]
        both = np.concatenate(out, 1).astype(np.float64).T * (self.rate / float(rate))
        P = self.left.shape[0]
        return HrirSet(self.directions, both[:P], both[P:], rate)


# ---- tap tables ---------------------------------------------------------------------------------------------------------------
def taps_wy(order=1):
    if order != 1:
        raise ValueError("the 'wy' fold-down is defined for first order only (W + Y, W - Y)")
    h = np.zeros((2, 4, 1))
    h[0, 0, 0] = h[0, 1, 0] = h[1, 0, 0] = 1.
    h[1, 1, 0] = -1.
    return h


def taps_ears(order, method='pseudoinv'):
    return ambisonics.decode_matrix(EAR_POSITIONS, order, method)[:, :, None]


def taps_speakers(order, positions=None, method='projection'):
    positions = ambisonics.ring_positions(order) if positions is None else positions
    return ambisonics.decode_matrix(positions, order, method)[:, :, None]


def taps_mic(order, rate):
    pos = ambisonics.ring_positions(order, 1.)
    D = ambisonics.decode_matrix(pos, order, 'projection')
    S = len(pos)
    dist = np.sqrt(((pos[:, None, :] - EAR_POSITIONS[None, :, :]) ** 2).sum(-1))        # [S, 2]
    delay = [[int(dist[s, e] / SPEED_OF_SOUND * rate) for e in range(2)] for s in range(S)]
    h = np.zeros((2, D.shape[1], max(max(d) for d in delay) + 1))
    for s in range(S):
        for e in range(2):
            h[e, :, delay[s][e]] += D[s] / (1. + dist[s, e]) / S
    return h


def taps_hrir(order, hrir):
    pos = ambisonics.ring_positions(order, 1.)
    D = ambisonics.decode_matrix(pos, order, 'projection')
    idx = [hrir.closest(p) for p in pos]
    h = np.stack([D.T @ hrir.left[idx], D.T @ hrir.right[idx]], 0)                        # [2, C, K] = sum_s D[s, c] h_s[k]
    return h


def build_taps(mode, order, rate=48000, hrir=None, decode=None, positions=None, resample=None, device=None):
    """(taps [O, C, K] fp64, zero_before) of one rendering.  decode: 'projection' | 'pseudoinv' for ears (default pseudoinv, what
    the reference's script uses) and speakers (default projection); mic and hrir decode by projection onto the ring as the
    reference does (its pseudoinv layouts come from a t-design table it does not ship).  resample: None refuses HRIRs that are not at
    `rate`; a quality ('best', 'fast' or a (zeros, beta, rolloff) tuple) resamples them on `device` (HrirSet.resampled)."""
    if mode not in MODES:
        raise ValueError('unknown rendering %r (one of %s)' % (mode, ', '.join(MODES)))
    if mode in ('wy', 'mic', 'hrir') and decode not in (None, 'projection'):
        raise ValueError("--decode applies to 'ears' and 'speakers' only")
    if mode == 'wy':
        return taps_wy(order), 0
    if mode == 'ears':
        return taps_ears(order, decode or 'pseudoinv'), 0
    if mode == 'speakers':
        return taps_speakers(order, positions, decode or 'projection'), 0
    if mode == 'mic':
        return taps_mic(order, rate), 0
    if hrir is None:
        raise ValueError("the 'hrir' rendering needs a set of HRIRs (--hrir_dir)")
    if int(hrir.rate) != int(rate):
        if resample is None:
            raise ValueError('the HRIRs are sampled at %d Hz, the audio at %d Hz (no resampler available offline)' % (hrir.rate, rate))
        hrir = hrir.resampled(rate, resample, device)
    h = taps_hrir(order, hrir)
    return h, h.shape[2] - 1


def head_trajectory(order, yaw_deg, pitch_deg=None, roll_deg=None):
    """[n_rot, C, C] control matrices for Renderer(rotation=...) from per-control-point head angles in degrees: the field is
    rotated by the inverse of the head's rotation."""
    yaw = np.atleast_1d(np.asarray(yaw_deg, np.float64))
    pitch = np.zeros_like(yaw) if pitch_deg is None else np.broadcast_to(np.asarray(pitch_deg, np.float64), yaw.shape)
    roll = np.zeros_like(yaw) if roll_deg is None else np.broadcast_to(np.asarray(roll_deg, np.float64), yaw.shape)
    rad = np.pi / 180.
    return np.stack([ambisonics.head_rotation_matrix(order, y * rad, p * rad, r * rad) for y, p, r in zip(yaw, pitch, roll)], 0)


class Renderer(object):
    """A stream renderer: process(x [n, C]) -> [n, O] on the device for any n >= 1, in stream order.  It keeps the last K - 1 input
    rows and the stream position between calls, so a stream cut into pieces gives the bits of the one-call result.
    rotation: one C x C matrix or an [n_rot, C, C] trajectory with one control point per rot_hop samples (linear in between,
    the last one held)."""

    def __init__(self, taps, zero_before=0, rotation=None, rot_hop=4800, device=None):
        import torch
        from . import ops
        taps = np.asarray(taps, np.float64)
        if taps.ndim != 3:
            raise ValueError('taps must be [outputs, channels, taps]')
        self.device = ops.default_device(device)
        self.outputs, self.channels, self.ntaps = taps.shape
        self.taps = torch.as_tensor(taps.astype(np.float32)).contiguous().to(self.device)
        self.zero_before, self.rot_hop = int(zero_before), int(rot_hop)
        self.rotation = None
        if rotation is not None:
            r = np.asarray(rotation, np.float64)
            r = r[None] if r.ndim == 2 else r
            if r.shape[1:] != (self.channels, self.channels):
                raise ValueError('rotation must be [%d, %d] or [n_rot, %d, %d]' % ((self.channels,) * 4))
            self.rotation = torch.as_tensor(r.astype(np.float32)).contiguous().to(self.device)
        self.reset()

    def reset(self):
        self.position, self.history = 0, None

    def process(self, x):
        import torch
        from . import ops
        if x.dim() != 2 or x.shape[1] != self.channels or x.shape[0] < 1:
            raise ValueError('process() takes [n >= 1, %d] rows' % self.channels)
        n = x.shape[0]
        buf = x if self.history is None else torch.cat([self.history, x], 0)
        n_hist = buf.shape[0] - n
        y = ops.render_fir(buf, n_hist, self.taps, self.rotation, self.rot_hop, self.position, self.zero_before)
        self.position += n
        if self.ntaps > 1:
            self.history = buf[-(self.ntaps - 1):].clone()          # (all of buf while the stream is shorter than that)
        return y


# ---- command lines ------------------------------------------------------------------------------------------------------------
def add_render_arguments(parser, default_mode=None):
    parser.add_argument('--render', choices=MODES, default=default_mode, help='rendering: W+-Y fold-down, decode at the ears, virtual '
                        'stereo microphone over a speaker ring, HRIRs over a speaker ring, or the speaker feeds themselves')
    parser.add_argument('--hrir_dir', default=None, help='directory of CIPIC-layout HRIR wavs ([neg]<az>az{left,right}.wav), for --render hrir')
    from .resample import add_quality_flag
    add_quality_flag(parser, '--resample_hrir', 'resample HRIRs that are not at the audio rate on the device')
    parser.add_argument('--decode', choices=('projection', 'pseudoinv'), default=None, help='decoder of ears (default pseudoinv) / speakers (default projection)')
    parser.add_argument('--yaw', type=float, default=0., help='head yaw in degrees (the field is rotated by the inverse)')
    parser.add_argument('--pitch', type=float, default=0.)
    parser.add_argument('--roll', type=float, default=0.)
    parser.add_argument('--normalize', type=float, default=None, metavar='PEAK', help='scale the finished rendering to this peak (myutils.py:290 uses 0.95)')


def check_render_arguments(args, channels, tool):
    """The refusals that need no device and no HRIR file: called before any other work."""
    if args.render is None:
        return
    if channels not in (4, 9):
        raise SystemExit('%s: %d channels is not first- or second-order ambisonics (4 or 9)' % (tool, channels))
    if args.render == 'wy' and channels != 4:
        raise SystemExit("%s: --render wy is the first-order W+-Y fold-down; %d channels given" % (tool, channels))
    if args.render == 'hrir' and not args.hrir_dir:
        raise SystemExit('%s: --render hrir needs --hrir_dir' % tool)
    if args.decode is not None and args.render not in ('ears', 'speakers'):
        raise SystemExit('%s: --decode applies to --render ears / speakers only' % tool)
    if args.normalize is not None and not args.normalize > 0:
        raise SystemExit('%s: --normalize takes a positive peak' % tool)


def rendering_from_arguments(args, channels, rate, tool):
    """Everything of a rendering that is made on the HOST: (taps, zero_before, rotation).  Reads the HRIR files; a missing directory
    or a rate mismatch is refused here, before the caller touches the device.  With --resample_hrir a rate mismatch is not refused:
    the HRIRs then go through the device's resampler here."""
    order = {4: 1, 9: 2}[channels]
    try:
        hrir = HrirSet.from_cipic_dir(args.hrir_dir) if args.render == 'hrir' else None
        quality = getattr(args, 'resample_hrir', None)
        device = None
        if quality is not None and hrir is not None and hrir.rate != int(rate):         # the one rendering that reaches the device here
            from . import ops
            ops.select_device(getattr(args, 'gpu', 0))                              # (what the caller does next anyway)
        taps, zero_before = build_taps(args.render, order, rate, hrir=hrir, decode=args.decode, resample=quality, device=device)
    except (ValueError, IOError) as e:
        raise SystemExit('%s: %s' % (tool, e))
    rotation = None
    if args.yaw or args.pitch or args.roll:
        rotation = head_trajectory(order, [args.yaw], [args.pitch], [args.roll])
    return taps, zero_before, rotation


def normalize_peak(y, peak):
    """myutils.py:290: stereo /= (abs(stereo).max() / 0.95); silence stays silence."""
    top = float(np.abs(y).max()) if y.size else 0.
    return y * (peak / top) if top > 0 else y


def parse_arguments(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('input_fn', help='Input ambisonics file (ACN / SN3D, 4 or 9 channels).')
    parser.add_argument('output_fn', help='Output file.')
    parser.add_argument('--overwrite', action='store_true', help='Whether to overwrite output file.')
    parser.add_argument('--gpu', type=int, default=0, help='GPU id')
    parser.add_argument('--block', type=int, default=480000, help='samples per device call')
    add_render_arguments(parser, default_mode='ears')
    return parser.parse_args(argv)


def main(argv=None):
    """scripts/binauralize_ambisonics.py:8-20, streamed through a Renderer in blocks."""
    import torch
    from . import ops
    from .feeder import load_wav, save_wav
    args = parse_arguments(argv)
    if os.path.exists(args.output_fn) and not args.overwrite:
        raise SystemExit('render: %s exists (--overwrite)' % args.output_fn)
    data, rate = load_wav(args.input_fn)
    check_render_arguments(args, data.shape[1], 'render')
    if args.block < 1:
        raise SystemExit('render: --block takes a positive count')
    taps, zero_before, rotation = rendering_from_arguments(args, data.shape[1], rate, 'render')      # host only: every refusal is behind us
    ops.select_device(args.gpu)
    r = Renderer(taps, zero_before, rotation)
    x = torch.as_tensor(data.astype(np.float32))
    out = [r.process(x[i:i + args.block].to(r.device)).cpu().numpy() for i in range(0, x.shape[0], args.block)]
    y = np.concatenate(out, 0) if out else np.zeros((0, r.outputs), np.float32)
    if args.normalize is not None:
        y = normalize_peak(y, args.normalize)
    save_wav(args.output_fn, y, rate)
    print('wrote %s: %d samples x %d channels (%s)' % (args.output_fn, y.shape[0], y.shape[1], args.render))


if __name__ == '__main__':
    main()
