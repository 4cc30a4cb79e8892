"""Resample audio on the device: a rational polyphase FIR, and the audio half of a clip folder.

    python -m spatialaudiogen_amd.resample convert IN.wav OUT.wav --rate 48000 [--quality best|fast] [--map C0 C1 ...]
           [--fuma_to_ambix] [--float] [--block N] [--overwrite] [--gpu I]
    python -m spatialaudiogen_amd.resample clip IN.wav CLIP_DIR [same options] [--overwrite]

The reference resamples with resampy's 'kaiser_fast' in load_wav(fname, rate) (pyutils/iolib/audio.py:23), with `ffmpeg -ar 48000` and
the `pan=4c|c0=c...` channel remap of prepare_ambisonics (scraping/preprocess.py:14-34), and in AmbisonicArray.convert(sample_rate,
ordering, normalization) (pyutils/ambisonics/common.py:34-59).  THIS IS A RESAMPLER OF OUR OWN: a Kaiser-windowed sinc in closed form,
not resampy's tabulated filter and not ffmpeg's swresample, and bit-compatible with neither.

The arithmetic, stated once (design() below, include/sagen.h: sagen_resample_fir, csrc/resample_core.h):

    g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, q = max(L, M)
    quality (zeros Z, beta, rolloff): 'best' = (64, 14.8, 0.9476), 'fast' = (16, 8.6, 0.85)    (after the two Kaiser filters resampy
                                      publishes; the reference uses the fast one)
    H = Z q, w = rolloff / q, h[k] = L w sinc(w k) I0(beta sqrt(1 - (k / H)^2)) / I0(beta), k = -H .. H, numpy.sinc, fp64
    y[n][o] = sum_m h[n M - m L] (sum_c mix[o][c] x[m][c])  over |n M - m L| <= H; x zero outside [0, N_in); zero phase
    fp64 sums, channels ascending inside, m ascending outside, one rounding to fp32; N_out = ceil(N_in L / M)

`clip` writes CLIP_DIR/ambix/%06d.wav (int(duration) chunks of 48 000 PCM16 samples) and CLIP_DIR/audio_pow.lst (extract_frames and
compute_audio_pow, scraping/preprocess.py:98-153): with `project` and `flow` a complete folder for deploy, evaluate and train.
Decoding and encoding wavs stay on the host; the stream goes through the device in blocks.
"""
import math
import os

import numpy as np

PRESETS = {'best': (64, 14.8, 0.9476), 'fast': (16, 8.6, 0.85)}
CLIP_RATE = 48000                     # the model's audio rate: chunk length and window arithmetic of a clip folder


def quality_tuple(quality):
    """(zeros, beta, rolloff) of a preset name or of a tuple."""
    if isinstance(quality, str):
        if quality not in PRESETS:
            raise ValueError('unknown resampling quality %r (one of %s, or a (zeros, beta, rolloff) tuple)' % (quality, ', '.join(sorted(PRESETS))))
        return PRESETS[quality]
    try:
        z, beta, rolloff = quality
    except (TypeError, ValueError):
        raise ValueError('quality must be a preset name or a (zeros, beta, rolloff) tuple, got %r' % (quality,))
    if int(z) != z or z < 1 or not beta >= 0 or not 0 < rolloff <= 1:
        raise ValueError('quality (zeros >= 1, beta >= 0, 0 < rolloff <= 1) expected, got %r' % (quality,))
    return int(z), float(beta), float(rolloff)


def ratio(rate_in, rate_out):
    """(L, M): rate_out / rate_in in lowest terms."""
    if int(rate_in) != rate_in or int(rate_out) != rate_out or rate_in < 1 or rate_out < 1:
        raise ValueError('rates must be positive integers, got %r -> %r' % (rate_in, rate_out))
    g = math.gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g


def prototype(rate_in, rate_out, quality='best'):
    """(L, M, H, h [2 H + 1] fp64): the prototype filter h[k], k = -H .. H, at L x the input rate."""
    L, M = ratio(rate_in, rate_out)
    zeros, beta, rolloff = quality_tuple(quality)
    q = max(L, M)
    H, w = zeros * q, rolloff / q
    k = np.arange(-H, H + 1, dtype=np.float64)
    h = L * w * np.sinc(w * k) * np.i0(beta * np.sqrt(1. - (k / H) ** 2)) / np.i0(beta)
    return L, M, H, h


def design(rate_in, rate_out, quality='best'):
    """(L, M, H, taps [L][T] fp64), T = ceil((2 H + 1) / L): row p holds the taps of the outputs of phase (n M) mod L = p in the order of
    the input rows they meet, taps[p][t] = h[kmax(p) - t L] with kmax(p) = p + L floor((H - p) / L), zero-filled where a phase has
    fewer taps; output n reads the rows ceil((n M - H) / L) + t."""
    L, M, H, h = prototype(rate_in, rate_out, quality)
    T = -(-(2 * H + 1) // L)
    p = np.arange(L, dtype=np.int64)[:, None]
    k = p + L * ((H - p) // L) - L * np.arange(T, dtype=np.int64)[None, :]
    taps = np.where(k >= -H, h[np.maximum(k + H, 0)], 0.)
    return L, M, H, np.ascontiguousarray(taps)


def output_length(n_in, L, M):
    return -(-int(n_in) * L // M)


# ---- channel mixes -------------------------------------------------------------------------------------------------------------
def mix_from_map(channel_map, c_in):
    """The selection matrix [len(map)][c_in] of a `pan=Nc|c0=c<map[0]>|c1=c<map[1]>...` remap (scraping/preprocess.py:22-28: [2, 1, 4, 0]
    for aac, [0, 1, 2, 3] for vorbis / opus): output o is input channel_map[o]."""
    m = np.zeros((len(channel_map), int(c_in)), np.float64)
    for o, c in enumerate(channel_map):
        if int(c) != c or not 0 <= c < c_in:
            raise ValueError('channel %r of the map is not one of the %d input channels' % (c, c_in))
        m[o, int(c)] = 1.
    return m


def mix_fuma_to_ambix(order=1):
    """First-order B-format (Furse-Malham: channels W X Y Z, W carrying 1 / sqrt(2), maxN) -> ambiX (ACN order n (n + 1) + m: W Y Z X;
    SN3D, whose first-order factors are all 1): what AmbisonicArray.convert(ordering='ACN', normalization='SN3D') does to a
    'FURSE_MALHAM' / 'MAX_N' array (pyutils/ambisonics/common.py:34-59)."""
    if order != 1:
        raise ValueError('the Furse-Malham <-> ambiX matrices are given for first order only')
    m = np.zeros((4, 4), np.float64)
    m[0, 0] = np.sqrt(2.)             # W
    m[1, 2] = 1.                      # ACN 1 = Y = FuMa channel 2
    m[2, 3] = 1.                      # ACN 2 = Z = FuMa channel 3
    m[3, 1] = 1.                      # ACN 3 = X = FuMa channel 1
    return m


def mix_ambix_to_fuma(order=1):
    """The inverse of mix_fuma_to_ambix: W / sqrt(2), then X Y Z from ACN 3, 1, 2."""
    if order != 1:
        raise ValueError('the Furse-Malham <-> ambiX matrices are given for first order only')
    m = np.zeros((4, 4), np.float64)
    m[0, 0] = 1. / np.sqrt(2.)
    m[1, 3] = 1.
    m[2, 1] = 1.
    m[3, 2] = 1.
    return m


# ---- the stream resampler ------------------------------------------------------------------------------------------------------
class Resampler(object):
    """A stream resampler: process(x [n >= 1, C_in] fp32 on the device) -> every output row that has become computable, in stream
    order (an output needs ceil(H / L) input rows of look-ahead, so the return may have 0 rows); flush() -> the rest, treating the
    stream as ended, after which the object stands at the start of a new stream, as after reset().  It keeps the input rows the next
    outputs still reach and the two stream positions between calls, so a stream cut into any pieces gives the bits of the one-call
    result.  mix: [C_out][C_in] fp64 or None (identity)."""

    def __init__(self, rate_in, rate_out, channels, mix=None, quality='best', device=None):
        import torch
        from . import ops
        self.L, self.M, self.H, taps = design(rate_in, rate_out, quality)
        self.channels = int(channels)
        self.outputs = self.channels
        self.device = ops.default_device(device)
        self.taps = torch.as_tensor(taps).to(self.device)
        self.mix = None
        if mix is not None:
            m = np.ascontiguousarray(np.asarray(mix, np.float64))
            if m.ndim != 2 or m.shape[1] != self.channels or m.shape[0] < 1:
                raise ValueError('mix must be [outputs, %d]' % self.channels)
            self.outputs = m.shape[0]
            self.mix = torch.as_tensor(m).to(self.device)
        self.reset()

    def reset(self):
        self.seen, self.position, self.history, self.history_start = 0, 0, None, 0

    def _emit(self, buf, upto):
        import torch
        from . import ops
        n = upto - self.position
        if n <= 0:
            return torch.empty(0, self.outputs, dtype=torch.float32, device=self.device)
        y = ops.resample_fir(buf, self.history_start, self.taps, self.L, self.M, self.H, self.position, n, self.mix)
        self.position = upto
        return y

    def process(self, x):
        import torch
        if x.dim() != 2 or x.shape[1] != self.channels or x.shape[0] < 1:
            raise ValueError('process() takes [n >= 1, %d] rows' % self.channels)
        buf = x if self.history is None else torch.cat([self.history, x], 0)
        self.seen += x.shape[0]
        # output n reaches the rows up to floor((n M + H) / L): computable while n M + H < seen L
        y = self._emit(buf, max(0, -(-(self.seen * self.L - self.H) // self.M)))
        keep_from = max(self.history_start, -(-(self.position * self.M - self.H) // self.L))       # first row the next output reaches
        self.history = buf[keep_from - self.history_start:].clone()
        self.history_start = keep_from
        return y

    def flush(self):
        import torch
        if self.history is None:
            y = torch.empty(0, self.outputs, dtype=torch.float32, device=self.device)
        else:
            y = self._emit(self.history, output_length(self.seen, self.L, self.M))
        self.reset()
        return y


def resample(x, rate_in, rate_out, mix=None, quality='best', device=None):
    """One-shot: x [n, C_in] (a numpy array, resampled through the device and returned as a float32 numpy array; or a float32 tensor
    on the device, returned as one) -> [ceil(n L / M), C_out].  A 1-D array is one channel.  Equal rates with no mix return the input
    unchanged, with no device call."""
    if int(rate_in) == int(rate_out) and mix is None:
        ratio(rate_in, rate_out)
        return x
    import torch
    from . import ops
    as_numpy = not isinstance(x, torch.Tensor)
    t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float32))) if as_numpy else x
    flat = t.dim() == 1
    if flat:
        t = t[:, None]
    if t.dim() != 2:
        raise ValueError('resample: x [n, C_in] expected')
    r = Resampler(rate_in, rate_out, t.shape[1], mix, quality, device if device is not None or as_numpy else t.device)
    n_out = output_length(t.shape[0], r.L, r.M)
    if n_out == 0:
        y = torch.empty(0, r.outputs, dtype=torch.float32, device=r.device)
    else:
        y = ops.resample_fir(t.to(r.device), 0, r.taps, r.L, r.M, r.H, 0, n_out, r.mix)
    if flat and r.outputs == 1:
        y = y[:, 0]
    return y.cpu().numpy() if as_numpy else y


def resample_stream(data, rate_in, rate_out, mix=None, quality='best', block=480000, device=None):
    """A host array [n, C_in] through a Resampler in blocks of `block` rows -> float32 [ceil(n L / M), C_out] on the host."""
    import torch
    r = Resampler(rate_in, rate_out, data.shape[1], mix, quality, device)
    x = torch.as_tensor(np.ascontiguousarray(data, np.float32))
    out = [r.process(x[i:i + block].to(r.device)).cpu().numpy() for i in range(0, x.shape[0], block)]
    out.append(r.flush().cpu().numpy())
    return np.concatenate(out, 0)


# ---- the audio half of a clip folder ---------------------------------------------------------------------------------------------
def pcm16_as_stored(y):
    """The samples as a PCM16 chunk written by feeder.save_wav and read back by feeder.load_wav holds them: save_wav's own expression
    on y as it is given (for float32 rows the product with 32767 is a float32 one, there as here), over 32768."""
    return np.rint(np.clip(np.asarray(y), -1.0, 1.0) * 32767.0).astype(np.int16) / 32768.


def pow_windows(n_chunks, rate=CLIP_RATE):
    """(times, first samples) of audio_pow.lst (scraping/preprocess.py:149-151): for i < (n_chunks - 1) * 10, t = i / 10. + 0.5, a window of
    rate / 10 samples from int(t * rate)."""
    times = [i / 10. + 0.5 for i in range(max(n_chunks - 1, 0) * 10)]
    return times, [int(t * rate) for t in times]


def format_pow_line(t, power):
    """One line of audio_pow.lst: '{} {}'.format(t, apow) under Python 2, whose str(float) is '%.12g'."""
    return '%.12g %.12g\n' % (t, power)


def window_powers(stored, starts, length, device=None):
    """RMS of channel 0 over the windows [start, start + length) of `stored` [n, C] (host, fp32-exact values) on the device: one
    ops.window_rms call per run of evenly spaced starts."""
    import torch
    from . import ops
    device = ops.default_device(device)
    x = torch.as_tensor(np.ascontiguousarray(stored[:, :1], np.float32)).to(device)
    out, i = [], 0
    while i < len(starts):
        j = i + 1
        hop = starts[j] - starts[i] if j < len(starts) else 0
        while j + 1 < len(starts) and starts[j + 1] - starts[j] == hop:
            j += 1
        count = min(j, len(starts) - 1) - i + 1                 # the windows i .. j, evenly spaced
        out.append(ops.window_rms(x, 0, starts[i], hop, length, count).cpu().numpy())
        i += count
    return np.concatenate(out) if out else np.zeros(0)


def write_clip_audio(y, clip_dir, rate=CLIP_RATE, device=None):
    """ambix/%06d.wav + audio_pow.lst of a clip folder from the resampled stream y [n, C] at `rate`; returns (n_chunks, n_lines)."""
    from .feeder import save_wav
    n_chunks = int(y.shape[0] / float(rate))
    audio_dir = os.path.join(clip_dir, 'ambix')
    os.makedirs(audio_dir, exist_ok=True)
    for i in range(n_chunks):
        save_wav(os.path.join(audio_dir, '%06d.wav' % i), y[i * rate:(i + 1) * rate], rate)
    times, starts = pow_windows(n_chunks, rate)
    powers = window_powers(pcm16_as_stored(y[:n_chunks * rate]), starts, rate // 10, device) if times else []
    with open(os.path.join(clip_dir, 'audio_pow.lst'), 'w') as f:
        for t, p in zip(times, powers):
            f.write(format_pow_line(t, p))
    return n_chunks, len(times)


# ---- command lines ---------------------------------------------------------------------------------------------------------------
def add_quality_flag(parser, flag, what):
    """An opt-in resampling flag: absent = None (the caller refuses a rate mismatch as before), bare = 'best'."""
    parser.add_argument(flag, nargs='?', const='best', default=None, choices=sorted(PRESETS), metavar='QUALITY',
                        help='%s (%s; default best). Without the flag a rate mismatch is refused.' % (what, ' | '.join(sorted(PRESETS))))


def mix_from_arguments(args, c_in, tool):
    mix = None
    try:
        if args.map is not None:
            mix = mix_from_map(args.map, c_in)
        if args.fuma_to_ambix:
            if (mix.shape[0] if mix is not None else c_in) != 4:
                raise ValueError('--fuma_to_ambix takes 4 channels (first-order B-format)')
            mix = mix_fuma_to_ambix(1) if mix is None else mix_fuma_to_ambix(1) @ mix
    except ValueError as e:
        raise SystemExit('%s: %s' % (tool, e))
    return mix


def parse_arguments(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = parser.add_subparsers(dest='command')
    sub.required = True
    for name, out, out_help in (('convert', 'output_fn', 'Output wav.'), ('clip', 'clip_dir', 'Clip folder: ambix/ and audio_pow.lst are written into it.')):
        p = sub.add_parser(name)
        p.add_argument('input_fn', help='Input wav.')
        p.add_argument(out, help=out_help)
        p.add_argument('--rate', type=int, default=CLIP_RATE, help='Output rate.')
        p.add_argument('--quality', choices=sorted(PRESETS), default='best')
        p.add_argument('--map', type=int, nargs='+', default=None, metavar='C', help='output channel o is input channel C_o (the `pan` remap; aac: 2 1 4 0)')
        p.add_argument('--fuma_to_ambix', action='store_true', help='first-order Furse-Malham (W X Y Z, maxN) to ambiX (W Y Z X, SN3D), after --map')
        p.add_argument('--float', dest='float_wav', action='store_true', help='convert: write a 32-bit float wav instead of 16-bit PCM')
        p.add_argument('--block', type=int, default=480000, help='input samples per device call')
        p.add_argument('--overwrite', action='store_true')
        p.add_argument('--gpu', type=int, default=0, help='GPU id')
    return parser.parse_args(argv)


def main(argv=None):
    from . import ops
    from .feeder import load_wav, save_wav
    args = parse_arguments(argv)
    tool = 'resample %s' % args.command
    if args.block < 1:
        raise SystemExit('%s: --block takes a positive count' % tool)
    if args.rate < 1:
        raise SystemExit('%s: --rate takes a positive rate' % tool)
    if args.command == 'convert':
        if os.path.exists(args.output_fn) and not args.overwrite:
            raise SystemExit('%s: %s exists (--overwrite)' % (tool, args.output_fn))
    else:
        if args.rate != CLIP_RATE:
            raise SystemExit('%s: a clip folder holds %d Hz audio (--rate %d)' % (tool, CLIP_RATE, args.rate))
        audio_dir, pow_fn = os.path.join(args.clip_dir, 'ambix'), os.path.join(args.clip_dir, 'audio_pow.lst')
        if ((os.path.isdir(audio_dir) and os.listdir(audio_dir)) or os.path.exists(pow_fn)) and not args.overwrite:
            raise SystemExit('%s: %s already holds audio (--overwrite)' % (tool, args.clip_dir))
    data, rate_in = load_wav(args.input_fn)
    mix = mix_from_arguments(args, data.shape[1], tool)
    ops.select_device(args.gpu)
    if int(rate_in) == args.rate and mix is None:
        y = data.astype(np.float32)
    else:
        y = resample_stream(data, rate_in, args.rate, mix, args.quality, args.block)
    if args.command == 'convert':
        save_wav(args.output_fn, y, args.rate, subtype='FLOAT' if args.float_wav else 'PCM_16')
        print('wrote %s: %d samples x %d channels at %d Hz (from %d Hz, %s)' % (args.output_fn, y.shape[0], y.shape[1], args.rate, rate_in, args.quality))
    else:
        if os.path.isdir(audio_dir):
            for f in os.listdir(audio_dir):
                if f.endswith('.wav'):
                    os.remove(os.path.join(audio_dir, f))
        n_chunks, n_lines = write_clip_audio(y, args.clip_dir, args.rate)
        print('wrote %s: %d chunks of %d samples x %d channels, %d lines of audio_pow.lst' % (args.clip_dir, n_chunks, args.rate, y.shape[1], n_lines))


if __name__ == '__main__':
    main()
