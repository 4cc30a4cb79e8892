"""Clip folders -> network inputs: the host side of the data path either end of the HIP forward.

Directory layout (what scraping/preprocess.py of the reference leaves behind, one folder per clip):

    ambix/%06d.wav      1-second pieces of the 4-channel first-order ambisonic track (W,Y,Z,X), 48 kHz PCM16
    video/%06d.jpg      224x448 RGB frames, 10 per second
    flow/%06d.jpg       optical flow, polar-coded in the R (angle) and B (magnitude) bytes, + flow/flow_limits.npy
    audio_pow.lst       one "<window time> <rms power>" line per 0.1 s window

This module is organised around a *window table*: for a list of window times it computes, in one vectorised pass,
which samples and which frame every window reads (`window_table`), and the stores below (`WavPieces`, `JpgFrames`,
`FlowFrames`) serve those reads from small decode caches, so consecutive windows - which overlap by 90 % - do not
decode the same wav piece or jpg twice.  `SampleReader` puts the reference's reader interface (constructor keywords,
`chunks_t`, `get()`, `loop_chunks()`; reference feeder.py:164-278) on top, because deploy.py / eval.py drive it.

What is pinned to the reference, and only that: the float arithmetic that decides WHICH samples and frame a window
gets -
    first sample of the padded window   int((t - context/2) * rate)                    feeder.py:66
    sample offset inside its 1-s piece  int((start - int(start)) * rate)               feeder.py:81
    frame index                         max(int(t * video_rate), 0)                    feeder.py:121
    time filters on audio_pow.lst       skip_rate, silence, start, duration, threads   feeder.py:222-238
- the truncations differ by one sample for about a fifth of the windows, and the network sees that.
Nothing here touches the GPU, except load_wav(..., resample=...) when it is asked to resample a file (resample.py),
`DeviceFrames`, the device-resident counterpart of `JpgFrames` / `FlowFrames` (jpeg.py decodes, sagen_assemble_frames batches), and
`DeviceAudio`, that of `WavPieces` (the pieces go up as stored, sagen_assemble_audio cuts the windows).
"""
import collections
import os
import random
import threading

import numpy as np

try:
    import queue
except ImportError:       # pragma: no cover
    import Queue as queue


# ------------------------------------------------------------------------------------------------
# file formats
# ------------------------------------------------------------------------------------------------
_PCM_SCALE = {np.dtype(np.int16): (0.0, 32768.0), np.dtype(np.int32): (0.0, 2147483648.0), np.dtype(np.uint8): (128.0, 128.0)}


def load_wav(fname, rate=None, resample=None):
    """(float64 [n, channels] in [-1, 1), rate) - integer PCM scaled by 1/2^(bits-1) the way libsndfile does for
    the reference (pyutils/iolib/audio.py:11-28).  resample=None: a rate mismatch raises.  resample='best' | 'fast' | (zeros, beta,
    rolloff): a file at another rate goes through the device's polyphase resampler (resample.resample, in place of the reference's
    resampy call, audio.py:23) and comes back as float64 rows at `rate`."""
    from scipy.io import wavfile
    file_rate, pcm = wavfile.read(fname)
    if rate is not None and int(rate) != int(file_rate) and resample is None:
        raise ValueError('%s is sampled at %d Hz, expected %d (no resampler available offline)' % (fname, file_rate, rate))
    pcm = pcm[:, None] if pcm.ndim == 1 else pcm
    offset, scale = _PCM_SCALE.get(pcm.dtype, (0.0, 1.0))
    data = (pcm.astype(np.float64) - offset) / scale
    if rate is not None and int(rate) != int(file_rate):
        from .resample import resample as resample_rows
        return resample_rows(data, file_rate, rate, quality=resample).astype(np.float64), int(rate)
    return data, file_rate


def save_wav(fname, signal, rate, subtype='PCM_16'):
    """[n, channels] float -> wav; 16-bit PCM by default (the reference's Format('wav'), pyutils/iolib/audio.py:31-34)."""
    from scipy.io import wavfile
    x = np.asarray(signal)
    if subtype == 'FLOAT':
        wavfile.write(fname, int(rate), x.astype(np.float32))
    elif subtype == 'PCM_16':
        wavfile.write(fname, int(rate), np.rint(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16))
    else:
        raise ValueError('unsupported wav subtype %r' % (subtype,))


def imread(fname):
    from PIL import Image
    with Image.open(fname) as im:
        return np.asarray(im.convert('RGB'))


def img_prep_fcn():
    """Pixel normalisation of the video encoder input, x/255 - 0.5 (myutils.py:88-89)."""
    return lambda x: x / 255. - 0.5


def frames_to_float(frames):
    """Decoded uint8 frames -> the float32 tensor the reference's feeder hands to the graph (img_prep_fcn in double precision, then the
    float32 cast of the batch assembly).  The readers of this package keep video frames as decoded (uint8: a quarter of the H2D bytes;
    sagen_forward_u8 / sagen_train_step_u8 apply the same normalisation on the device, bit-identical) - this is the host-side form
    for the one case that needs float frames: a zero-padded partial batch, whose padding is 0.0 AFTER normalisation (deploy.py:125-127),
    a value no uint8 pixel maps to."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        return frames.astype(np.float32)
    return (frames.astype(np.float64) / 255. - 0.5).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# window table: the pinned arithmetic, vectorised over the window times
# ------------------------------------------------------------------------------------------------
WindowTable = collections.namedtuple('WindowTable', 'lead read_from read_count trail frame')


def window_table(times, context, size, audio_rate, total_samples, video_rate=10):
    """For every window time t: `lead` zeros, then `read_count` samples starting at absolute sample `read_from`, then
    `trail` zeros make up the `size`-sample audio input; `frame` is the video / flow frame index.
    Float64 / truncation semantics are those of the reference lines quoted in the module docstring."""
    t = np.asarray(times, dtype=np.float64)
    rate = audio_rate
    start = t - context / 2
    first = np.trunc(start * rate).astype(np.int64)              # int() truncates toward zero
    lead = np.where(first < 0, -first, 0)
    start = np.where(first < 0, 0.0, start)
    first = np.maximum(first, 0)
    count = size - lead
    trail = np.maximum(first + count - int(total_samples), 0)
    count = np.maximum(count - trail, 0)
    whole = np.trunc(start)
    read_from = whole.astype(np.int64) * int(rate) + np.trunc((start - whole) * rate).astype(np.int64)
    frame = np.maximum(np.trunc(t * video_rate).astype(np.int64), 0)
    return WindowTable(lead, read_from, count, trail, frame)


def select_times(times, powers=None, skip_rate=None, skip_silence_thr=None, start_time=0.5, sample_duration=None,
                 num_threads=1, thread_id=0):
    """The window-time filters a reader applies to audio_pow.lst, in the reference's order (feeder.py:222-238)."""
    times = list(times)
    powers = list(powers) if powers is not None else [np.inf] * len(times)
    keep_every = 1 if skip_rate is None else skip_rate
    times, powers = times[::keep_every], powers[::keep_every]
    floor = -np.inf if skip_silence_thr is None else skip_silence_thr
    times = [t for t, p in zip(times, powers) if p > floor]
    lo = start_time if start_time > 0.5 else -np.inf                 # (the list itself starts at 0.5)
    hi = np.inf if sample_duration is None else start_time + sample_duration
    times = [t for t in times if lo <= t < hi]
    if num_threads > 1:                                              # contiguous share of this reader thread
        cut = np.linspace(0, len(times), num_threads + 1).astype(int)
        times = times[cut[thread_id]:cut[thread_id + 1]]
    return times


def read_pow_list(fname):
    """audio_pow.lst -> (times, powers)."""
    times, powers = [], []
    with open(fname) as f:
        for line in f:
            cols = line.split()
            if cols:
                times.append(float(cols[0]))
                powers.append(float(cols[1]))
    return times, powers


def rotation_matrix_z(angle):
    """First-order ambisonic (W,Y,Z,X) rotation about the vertical axis: W, Z unchanged; (Y, X) rotate as a vector
    (the augmentation of feeder.py:92-101)."""
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(4)
    m[1, 1], m[1, 3], m[3, 1], m[3, 3] = c, s, -s, c
    return m


# ------------------------------------------------------------------------------------------------
# decode caches
# ------------------------------------------------------------------------------------------------
class _Lru(object):
    def __init__(self, capacity):
        self.capacity, self.items = capacity, collections.OrderedDict()

    def fetch(self, key, make):
        if key in self.items:
            self.items.move_to_end(key)
            return self.items[key]
        value = make(key)
        self.items[key] = value
        while len(self.items) > self.capacity:
            self.items.popitem(last=False)
        return value


class WavPieces(object):
    """The 1-second wav pieces of a clip as one virtual sample axis (piece i covers samples [i*rate, (i+1)*rate))."""

    def __init__(self, folder, rate=None, ambi_order=1, cache=4):
        self.folder = str(folder)
        self.num_files = sum(1 for f in os.listdir(folder) if f.endswith('.wav'))
        if self.num_files == 0:
            raise IOError('no wav pieces in %s' % folder)
        first, file_rate = load_wav(self._path(0))
        self.rate = float(file_rate) if rate is None else rate
        self.num_channels = min(first.shape[1], (ambi_order + 1) ** 2)
        self.duration = self.num_files
        self.num_frames = int(self.duration * self.rate)
        self._cache = _Lru(cache)

    def _path(self, i):
        return os.path.join(self.folder, '%06d.wav' % i)

    def _piece(self, i):
        return self._cache.fetch(i, lambda k: load_wav(self._path(k), self.rate)[0][:, :self.num_channels])

    def read(self, read_from, count):
        """`count` samples from absolute sample `read_from` (pieces decoded once and cached)."""
        out = np.zeros((count, self.num_channels))
        per = int(self.rate)
        done = 0
        while done < count:
            i, off = divmod(read_from + done, per)
            if i >= self.num_files:
                break
            piece = self._piece(i)
            n = min(count - done, piece.shape[0] - off)
            if n <= 0:
                break
            out[done:done + n] = piece[off:off + n]
            done += n
        return out

    def window(self, t_start, size, rotation=None):
        """`size` samples from time `t_start` (seconds), zero-padded outside the clip."""
        tab = window_table([t_start], 0.0, size, self.rate, self.num_frames)
        return self.assemble(tab, 0, size, rotation)

    def assemble(self, tab, k, size, rotation=None):
        out = np.zeros((size, self.num_channels))
        lead, n = int(tab.lead[k]), int(tab.read_count[k])
        out[lead:lead + n] = self.read(int(tab.read_from[k]), n)
        if rotation is not None:
            if not -np.pi <= rotation < np.pi:
                raise ValueError('rotation must lie in [-pi, pi)')
            out = out.dot(rotation_matrix_z(rotation)[:self.num_channels, :self.num_channels].T)
        return out


class AudioReader(WavPieces):
    """Reference-named view of WavPieces: get(start_time, size, rotation) (feeder.py:50-103)."""

    def get(self, start_time, size, rotation=None):
        return self.window(start_time, size, rotation)


class JpgFrames(object):
    """%06d.jpg frames of a folder, preprocessed on decode and cached."""

    RAW_RATE = 10.

    def __init__(self, folder, rate=None, prep=None, cache=4):
        self.folder = str(folder)
        self.rate = self.RAW_RATE if rate is None else rate
        self.prep = prep
        names = sorted(f for f in os.listdir(folder) if f.endswith('.jpg'))
        if not names:
            raise IOError('no jpg frames in %s' % folder)
        self.num_frames = len(names)
        self.duration = self.num_frames / self.RAW_RATE
        self._cache = _Lru(cache)
        self.frame_shape = self.frame(int(os.path.splitext(names[0])[0])).shape

    def frame(self, index):
        def decode(i):
            img = imread(os.path.join(self.folder, '%06d.jpg' % i))
            return self.prep(img) if self.prep is not None else img
        return self._cache.fetch(index, decode)

    def frames(self, first, count, rotation=None):
        clip = np.stack([self.frame(i) for i in range(first, first + count)], 0)
        if rotation:                      # equirectangular frames: a yaw rotation is a horizontal roll
            clip = np.roll(clip, -int(rotation / (2. * np.pi) * self.frame_shape[1]), axis=2)
        return clip

    def get_by_index(self, start_time, size, rotation=None):
        return self.frames(max(int(start_time * self.rate), 0), size, rotation)


VideoReader = JpgFrames


class FlowFrames(object):
    """Optical flow frames: byte 0 = angle / 2pi * 255, byte 2 = magnitude scaled into the frame's [min, max] of
    flow_limits.npy; decoded to (m cos a, m sin a, m) float32 (feeder.py:135-161)."""

    def __init__(self, folder, limits_fn, rate=None, flow_prep=None):
        self.jpgs = JpgFrames(folder, rate=rate)
        self.limits = np.load(limits_fn)
        self.rate, self.duration = self.jpgs.rate, self.jpgs.duration
        self.flow_prep = flow_prep

    def frames(self, first, count, rotation=None):
        # the reference's op order and rounding points (feeder.py:147-160): the limits are float64, so each in-place update of the
        # float32 frames is computed in double and rounded once; the angle scale is a Python scalar (float32 arithmetic)
        out = self.jpgs.frames(first, count, rotation).astype(np.float32)
        lo = self.limits[first:first + count, 0].reshape(-1, 1, 1)
        hi = self.limits[first:first + count, 1].reshape(-1, 1, 1)
        out[..., 2] *= (hi - lo) / 255.
        out[..., 2] += lo
        out[..., 0] *= (2 * np.pi) / 255.
        out[..., 1] = out[..., 2] * np.sin(out[..., 0])
        out[..., 0] = out[..., 2] * np.cos(out[..., 0])
        return self.flow_prep(out) if self.flow_prep is not None else out

    def get_by_index(self, start_time, size, rotation=None):
        return self.frames(max(int(start_time * self.rate), 0), size, rotation)


FlowReader = FlowFrames


def video_table():
    """table[byte] of sagen_assemble_frames mode 1: frames_to_float of every byte value"""
    return frames_to_float(np.arange(256).astype(np.uint8))


def flow_table():
    """cos[256] then sin[256] of the angle a byte stands for (sagen_assemble_frames mode 2), by the expressions of FlowFrames.frames"""
    angle = np.arange(256).astype(np.float32)
    angle *= (2 * np.pi) / 255.
    return np.concatenate([np.cos(angle), np.sin(angle)])


def flow_scale_lo(limits):
    """flow_limits.npy [frames, 2] -> the operands ((hi - lo) / 255., lo) of FlowFrames.frames per frame, by its own expressions and in
    the file's dtype, then widened (exact): float64 [frames, 2]"""
    lo, hi = limits[:, 0], limits[:, 1]
    return np.stack([(hi - lo) / 255., lo], 1).astype(np.float64)


def frames_batch(frames, table, mode, pad_to=None, scale_lo=None):
    """Decoded frames uint8 [n, H, W, 3] on the device, in batch order -> float32 [pad_to or n, 1, H, W, 3] there by one launch of
    sagen_assemble_frames: mode 1 table[byte] (video_table: frames_to_float), mode 2 the flow un-coding (flow_table, scale_lo float64
    [n, 2] on the device, row i for frame i); the items behind n are 0.0.  For frames that are decoded per batch, not resident
    (evaluate --decode device); a resident clip batches through DeviceFrames.batch."""
    import torch
    from . import _lib
    from .ops import _ptr, _stream
    n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    total = n if pad_to is None else int(pad_to)
    if total < n:
        raise ValueError('pad_to=%d is less than the %d frames given' % (total, n))
    out = torch.empty((total, 1, h, w, 3), dtype=torch.float32, device=frames.device)
    if total == 0:
        return out
    args = np.zeros((2, total), np.int32)
    args[0] = -1                                                       # padding
    args[0, :n] = np.arange(n)
    dev = torch.as_tensor(args).to(frames.device)
    frames = frames.contiguous()
    _lib.check(_lib.lib().sagen_assemble_frames(_ptr(frames), n, h, w, _ptr(dev[0]), _ptr(dev[1]), total, int(mode), _ptr(table),
                                                _ptr(scale_lo) if mode == 2 else None, _ptr(out), _stream()))
    return out


class DeviceFrames(object):
    """The %06d.jpg frames of a folder RESIDENT ON THE DEVICE, and batches assembled from them there (include/sagen.h:
    sagen_assemble_frames): what JpgFrames.frames (kind='video') and FlowFrames.frames (kind='flow', with the folder's
    flow_limits.npy) return, bit for bit, without a decoded frame crossing the bus.

        ensure(first, stop)     decodes the frames [first, stop) that are not resident yet (jpeg.JpegDecoder, `block` files per call)
        batch(indices, ...)     [n, 1, H, W, 3] on the device: uint8 video as decoded, or float32 (normalised video / un-coded flow)

    The resident frames are one uint8 tensor over one contiguous range of frame numbers.  Host preprocessing callables (prep,
    flow_prep) are refused: the values are made on the device.  With SAGEN_LIB naming the CPU twin everything runs on device='cpu'."""

    RAW_RATE = JpgFrames.RAW_RATE

    def __init__(self, folder, kind='video', device=None, decoder=None, block=256, rate=None, prep=None, flow_prep=None, entropy='lane'):
        import torch
        from . import ops
        if kind not in ('video', 'flow'):
            raise ValueError("kind must be 'video' or 'flow', not %r" % (kind,))
        if prep is not None or flow_prep is not None:
            raise ValueError('DeviceFrames makes its values on the device: a prep / flow_prep callable is a host function (use JpgFrames / FlowFrames)')
        if int(block) < 1:
            raise ValueError('block must be at least 1')
        self.folder, self.kind, self.block = str(folder), kind, int(block)
        self.rate = self.RAW_RATE if rate is None else rate
        names = sorted(f for f in os.listdir(folder) if f.endswith('.jpg'))
        if not names:
            raise IOError('no jpg frames in %s' % folder)
        self.num_frames = len(names)
        self.duration = self.num_frames / self.RAW_RATE
        from PIL import Image
        with Image.open(os.path.join(self.folder, names[0])) as im:       # (the header only: nothing is decoded here)
            self.frame_shape = (im.size[1], im.size[0], 3)
        if device is None and decoder is not None:
            device = decoder.device
        self.device = ops.default_device(device)
        if decoder is None:
            from .jpeg import JpegDecoder
            decoder = JpegDecoder(self.device, entropy=entropy)                 # ('split': many lanes per restart segment; same pixels)
        elif entropy != 'lane' and getattr(decoder, 'entropy', 'lane') != entropy:
            raise ValueError('entropy=%r, but the decoder handed in was made with another' % (entropy,))
        self.decoder = decoder
        self.first = self.stop = 0                                      # the resident range
        self._frames = torch.empty((0,) + self.frame_shape, dtype=torch.uint8, device=self.device)
        self._scale_lo = None
        if kind == 'flow':
            limits = np.load(os.path.join(self.folder, 'flow_limits.npy'))
            if limits.ndim != 2 or limits.shape[1] != 2:
                raise ValueError('flow_limits.npy must be [frames, 2], not %s' % (limits.shape,))
            self.limits = limits
            self._scale_lo = torch.as_tensor(flow_scale_lo(limits)).contiguous().to(self.device)
            table = flow_table()
        else:
            table = video_table()
        self._table = torch.as_tensor(np.ascontiguousarray(table, dtype=np.float32)).to(self.device)

    def ensure(self, first, stop):
        """Make the frames [first, stop) resident.  The resident range stays one range: it grows to cover the request (and what lies
        between the two, if they do not touch); frames already resident are not decoded again."""
        import torch
        first, stop = int(first), int(stop)
        if not 0 <= first <= stop <= self.num_frames:
            raise IndexError('frames %d..%d of the %d in %s' % (first, stop - 1, self.num_frames, self.folder))
        if self.kind == 'flow' and stop > self.limits.shape[0]:
            raise IndexError('frames %d..%d: flow_limits.npy of %s has %d rows' % (first, stop - 1, self.folder, self.limits.shape[0]))
        if first == stop:
            return
        if self.first == self.stop:
            parts, self.first, self.stop = [self._decode(first, stop)], first, stop
        else:
            parts = [self._frames]
            if first < self.first:
                parts.insert(0, self._decode(first, self.first))
                self.first = first
            if stop > self.stop:
                parts.append(self._decode(self.stop, stop))
                self.stop = stop
        if len(parts) > 1 or parts[0] is not self._frames:
            parts = [p for p in parts if p.shape[0]]
            self._frames = parts[0] if len(parts) == 1 else torch.cat(parts, 0)

    def _decode(self, first, stop):
        import torch
        names = [os.path.join(self.folder, '%06d.jpg' % i) for i in range(first, stop)]
        parts = [self.decoder.decode(names[k:k + self.block]) for k in range(0, len(names), self.block)]
        for p in parts:
            if tuple(p.shape[1:]) != self.frame_shape:
                raise ValueError('%s: a frame of %dx%d, the first one is %dx%d' % ((self.folder, p.shape[2], p.shape[1]) + self.frame_shape[1::-1]))
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)

    def shift_of(self, rotation):
        """The roll of JpgFrames.frames, by its expression: a yaw rotation of an equirectangular frame is a horizontal roll."""
        return -int(rotation / (2. * np.pi) * self.frame_shape[1]) if rotation else 0

    def batch(self, indices, rotations=None, pad_to=None, as_float=False):
        """The frames `indices` (resident frame numbers, any order, repeats allowed), item i rolled by rotations[i] (a sequence, one
        number for all, or None), as [n, 1, H, W, 3] on the device.  video: uint8 as decoded, or with as_float=True the float32 of
        frames_to_float; flow: always the float32 of FlowFrames.frames.  pad_to: the float32 forms are filled up to pad_to items
        with items of 0.0 (a zero-padded partial batch; no uint8 value stands for 0.0 after normalisation, so uint8 has no padding).
        One launch; an index that is not resident raises before it."""
        import torch
        from . import _lib
        from .ops import _ptr, _stream
        idx =[int(i) for i in indices]
        n = len(idx)
        for i in idx:
            if not self.first <= i < self.stop:
                raise IndexError('frame %d of %s is not resident (resident: %d..%d; ensure() decodes)' % (i, self.folder, self.first, self.stop - 1))
        if rotations is None or isinstance(rotations, (int, float)):
            rotations = [rotations] * n
        if len(rotations) != n:
            raise ValueError('%d rotations for %d frames' % (len(rotations), n))
        as_float = bool(as_float) or self.kind == 'flow'
        total = n if pad_to is None else int(pad_to)
        if total < n:
            raise ValueError('pad_to=%d is less than the %d frames asked for' % (total, n))
        if total > n and not as_float:
            raise ValueError('uint8 frames cannot be padded (0.0 after normalisation is no uint8 value): as_float=True')
        h, w = self.frame_shape[:2]
        out = torch.empty((total, 1, h, w, 3), dtype=torch.float32 if as_float else torch.uint8, device=self.device)
        if total == 0:
            return out
        args = np.zeros((2, total), np.int32)
        args[0] = -1                                                   # padding
        args[0, :n] = np.asarray(idx, np.int64) - self.first
        args[1, :n] = [self.shift_of(r) for r in rotations]
        dev = torch.as_tensor(args).to(self.device)
        mode = 2 if self.kind == 'flow' else (1 if as_float else 0)
        _lib.check(_lib.lib().sagen_assemble_frames(_ptr(self._frames), int(self._frames.shape[0]), h, w, _ptr(dev[0]), _ptr(dev[1]), total, mode,
                                                    _ptr(self._table), _ptr(self._scale_lo[self.first:]) if mode == 2 else None, _ptr(out),
                                                    _stream()))
        return out


class DeviceAudio(object):
    """The %06d.wav pieces of an ambix folder RESIDENT ON THE DEVICE, and batches of windows assembled from them there (include/sagen.h:
    sagen_assemble_audio): what WavPieces.assemble(...).astype(float32) returns for every window, without a window crossing the bus -
    and, in the same launch, the two views the network is fed from (the mono input, the target rows of the other channels).

        batch(times, context, size, ...)     the windows at `times`, as the outputs named by `want`, on the device

    The samples are kept as the files store them when that is int16 or float32 (the op widens them as load_wav does), float64 of
    load_wav's values otherwise (other PCM widths, pieces of mixed types).  Piece i lies at row i * rate; num_frames = n_files * rate as
    WavPieces has it; a short LAST piece is zero-filled, any other piece that is not `rate` rows long raises ValueError (WavPieces would
    read zeros or the wrong rows there).  A file at another rate raises, as load_wav does by default: nothing is resampled here.
    With SAGEN_LIB naming the CPU twin everything runs on device='cpu'."""

    OUTPUTS = ('full', 'mono', 'target')

    def __init__(self, folder, rate=None, ambi_order=1, device=None):
        import torch
        from scipy.io import wavfile
        from . import ops
        self.folder = str(folder)
        self.num_files = sum(1 for f in os.listdir(folder) if f.endswith('.wav'))
        if self.num_files == 0:
            raise IOError('no wav pieces in %s' % folder)
        pieces = []
        for i in range(self.num_files):
            fname = os.path.join(self.folder, '%06d.wav' % i)
            file_rate, pcm = wavfile.read(fname)
            if i == 0:
                self.rate = float(file_rate) if rate is None else rate
                self.num_channels = min(1 if pcm.ndim == 1 else pcm.shape[1], (ambi_order + 1) ** 2)
            if int(self.rate) != int(file_rate):
                raise ValueError('%s is sampled at %d Hz, expected %d (DeviceAudio does not resample)' % (fname, file_rate, self.rate))
            pcm = pcm[:, None] if pcm.ndim == 1 else pcm
            if pcm.shape[1] < self.num_channels:
                raise ValueError('%s has %d channels, the first piece has %d' % (fname, pcm.shape[1], self.num_channels))
            pieces.append(pcm[:, :self.num_channels])
        per = int(self.rate)
        self.duration = self.num_files
        self.num_frames = int(self.duration * self.rate)
        for i, pcm in enumerate(pieces):
            if pcm.shape[0] > per or (pcm.shape[0] < per and i != self.num_files - 1):
                raise ValueError('%s holds %d samples, not the %d of one second (only the last piece may be short)'
                                 % (os.path.join(self.folder, '%06d.wav' % i), pcm.shape[0], per))
        kinds = set(p.dtype for p in pieces)
        if kinds == {np.dtype(np.int16)} or kinds == {np.dtype(np.float32)}:
            dtype = kinds.pop()
        else:                                                          # load_wav's values
            dtype = np.dtype(np.float64)
            for i, pcm in enumerate(pieces):
                offset, scale = _PCM_SCALE.get(pcm.dtype, (0.0, 1.0))
                pieces[i] = (pcm.astype(np.float64) - offset) / scale
        self.sample_type = {np.dtype(np.int16): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}[dtype]
        host = np.zeros((self.num_frames, self.num_channels), dtype)
        for i, pcm in enumerate(pieces):
            host[i * per:i * per + pcm.shape[0]] = pcm
        self.device = ops.default_device(device)
        self._samples = torch.as_tensor(host).to(self.device)

    def table(self, times, context, size):
        """The window table of `times` over this clip (see window_table)."""
        return window_table(times, context, size, self.rate, self.num_frames)

    def batch(self, times, context, size, rotations=None, pad_to=None, want=('mono',), t_off=None, t_len=None, out=None):
        """The `size`-sample windows at `times` (window_table's arithmetic with `context`), window i rotated about the vertical axis by
        rotations[i] (a sequence, one number for all, or None; each angle in [-pi, pi) as WavPieces.assemble demands; needs the 4
        first-order channels).  Returns a tuple of float32 device tensors in the order of `want`:
            'full'    [n, size, channels]
            'mono'    [n, size, 1]: channel 0, the network's input
            'target'  [n, t_len, channels - 1]: the other channels of the rows [t_off, t_off + t_len)
        pad_to: the outputs are filled up to pad_to windows with windows of zeros (read_count = 0; a zero-padded partial batch).
        out: {name: tensor} to write into (contiguous, of exactly these shapes - slices along the first axis of a larger batch, say),
        instead of new tensors.  The three columns of the table and the (cos, sin) pairs go up in one small tensor; one launch.
        When `rotations` mixes None with angles, None becomes (cos, sin) = (1, 0), which is the identity on every value but one: a
        sample of -0.0 in Y or X comes out as +0.0 (1 * -0.0 + 0 * x).  All None passes no rotation at all and keeps it."""
        import ctypes as C
        import torch
        from . import _lib
        from .ops import _ptr, _stream
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(w not in self.OUTPUTS for w in want) or len(set(want)) != len(want):
            raise ValueError('want must name one or more of %s, once each; not %r' % (self.OUTPUTS, want))
        times = [float(t) for t in times]
        n, size = len(times), int(size)
        if rotations is None or isinstance(rotations, (int, float)):
            rotations = [rotations] * n
        if len(rotations) != n:
            raise ValueError('%d rotations for %d windows' % (len(rotations), n))
        rotated = any(r is not None for r in rotations)
        for r in rotations:
            if r is not None and not -np.pi <= r < np.pi:
                raise ValueError('rotation must lie in [-pi, pi)')
        if rotated and self.num_channels != 4:
            raise ValueError('a rotation needs the 4 first-order channels (W,Y,Z,X), this clip has %d' % self.num_channels)
        total = n if pad_to is None else int(pad_to)
        if total < n:
            raise ValueError('pad_to=%d is less than the %d windows asked for' % (total, n))
        if 'target' in want:
            if t_off is None or t_len is None:
                raise ValueError("want='target' needs t_off and t_len")
            if self.num_channels < 2 or not (0 <= int(t_off) and 1 <= int(t_len) and int(t_off) + int(t_len) <= size):
                raise ValueError('target rows t_off=%s t_len=%s of %d-sample windows of %d channels' % (t_off, t_len, size, self.num_channels))
        t_off, t_len = (int(t_off), int(t_len)) if 'target' in want else (0, 0)
        shapes = {'full': (total, size, self.num_channels), 'mono': (total, size, 1), 'target': (total, t_len, self.num_channels - 1)}
        outs = {}
        for w in want:
            if out is not None and w in out:
                o = out[w]
                if tuple(o.shape) != shapes[w] or o.dtype != torch.float32 or o.device != self._samples.device or not o.is_contiguous():
                    raise ValueError('out[%r] must be a contiguous float32 %s on %s' % (w, shapes[w], self.device))
                outs[w] = o
            else:
                outs[w] = torch.empty(shapes[w], dtype=torch.float32, device=self.device)
        if total == 0:
            return tuple(outs[w] for w in want)
        # one int64 buffer: read_from [total] | (cos, sin) [total][2] as fp64 | lead [total] int32 | read_count [total] int32
        buf = np.zeros(4 * total, np.int64)
        i32 = buf[3 * total:].view(np.int32)
        if n:
            tab = window_table(times, context, size, self.rate, self.num_frames)
            buf[:n] = tab.read_from
            i32[:n] = tab.lead
            i32[total:total + n] = tab.read_count
        if rotated:
            cs = buf[total:3 * total].view(np.float64).reshape(total, 2)
            cs[:, 0] = 1.0
            cs[:n] = [(1.0, 0.0) if r is None else (np.cos(r), np.sin(r)) for r in rotations]
        dev = torch.as_tensor(buf).to(self.device)
        base = dev.data_ptr()
        _lib.check(_lib.lib().sagen_assemble_audio(
            _ptr(self._samples), self.sample_type, int(self._samples.shape[0]), self.num_channels, C.c_void_p(base + 24 * total),
            C.c_void_p(base), C.c_void_p(base + 28 * total), C.c_void_p(base + 8 * total) if rotated else None, total, size, t_off, t_len,
            _ptr(outs.get('full')), _ptr(outs.get('mono')), _ptr(outs.get('target')), _stream()))
        return tuple(outs[w] for w in want)


# ------------------------------------------------------------------------------------------------
# one clip -> 0.1 s samples
# ------------------------------------------------------------------------------------------------
class SampleReader(object):
    """Samples {'id', 'ambix' [audio_size, C], 'video' / 'flow' [n, 224, 448, 3]} of one clip folder, one per selected
    window time, with the reference reader's interface (feeder.py:164-278).  `chunks_t` may be re-assigned before
    reading (deploy.py:106-107 shifts it)."""

    def __init__(self, folder, ambi_order=1, audio_rate=48000, video_rate=10, context=1.0, duration=0.1,
                 return_video=True, img_prep=None, return_flow=False, flow_prep=None, skip_silence_thr=None,
                 shuffle=True, start_time=0.5, sample_duration=None, skip_rate=None, random_rotations=True,
                 num_threads=1, thread_id=0):
        for name, v in (('audio/video rate ratio', float(audio_rate) / video_rate), ('duration*audio_rate', duration * audio_rate),
                        ('duration*video_rate', duration * video_rate), ('context*audio_rate', context * audio_rate)):
            if float(v) != int(v):
                raise ValueError('%s must be an integer (got %r)' % (name, v))
        self.folder = folder
        self.video_id = os.path.basename(os.path.normpath(folder))
        self.duration, self.context = duration, context
        self.audio_rate, self.video_rate = audio_rate, video_rate
        self.audio_size = int(duration * audio_rate) + int(context * audio_rate) - 1
        self.video_size = int(duration * video_rate)
        self.return_video, self.return_flow, self.random_rotations = return_video, return_flow, random_rotations
        self.audio_reader = AudioReader(os.path.join(folder, 'ambix'), audio_rate, ambi_order)
        self.video_reader = JpgFrames(os.path.join(folder, 'video'), video_rate, img_prep) if return_video else None
        self.flow_reader = None
        if return_flow:
            fdir = os.path.join(folder, 'flow')
            self.flow_reader = FlowFrames(fdir, os.path.join(fdir, 'flow_limits.npy'), video_rate, flow_prep)
        times, powers = read_pow_list(os.path.join(folder, 'audio_pow.lst'))
        times = select_times(times, powers, skip_rate, skip_silence_thr, start_time, sample_duration, num_threads, thread_id)
        if shuffle:
            random.shuffle(times)
        self.chunks_t = times
        self.head = -1
        self.cur_t = None

    def table(self):
        """Window table of the current `chunks_t` (see window_table)."""
        return window_table(self.chunks_t, self.context, self.audio_size, self.audio_rate, self.audio_reader.num_frames,
                            self.video_rate)

    def sample_at(self, t, rotation=None):
        """The sample of window time `t` (any time, not only the listed ones)."""
        tab = window_table([t], self.context, self.audio_size, self.audio_rate, self.audio_reader.num_frames, self.video_rate)
        sample = {'id': '%s %s' % (self.video_id, t),
                  'ambix': self.audio_reader.assemble(tab, 0, self.audio_size, rotation)}
        if self.return_video:
            sample['video'] = self.video_reader.frames(int(tab.frame[0]), self.video_size, rotation)
        if self.return_flow:
            sample['flow'] = self.flow_reader.frames(int(tab.frame[0]), self.video_size, rotation)
        return sample

    def get(self):
        self.head += 1
        if self.head >= len(self.chunks_t):
            return None
        self.cur_t = self.chunks_t[self.head]
        return self.sample_at(self.cur_t, random.random() * 2 * np.pi - np.pi if self.random_rotations else None)

    def loop_chunks(self, n=np.inf):
        served = 0
        while served < n:
            sample = self.get()
            if sample is None:
                return
            served += 1
            yield sample


# ------------------------------------------------------------------------------------------------
# background batching (the role of the reference's feeder threads + TF queue, feeder.py:281-435)
# ------------------------------------------------------------------------------------------------
class BatchPrefetcher(object):
    """One producer thread decodes batches ahead of the GPU into a bounded queue (optionally as pinned torch tensors).
    Order is preserved.  A failure in the producer (missing / short wav or jpg, bad flow limits) is re-raised in the
    consumer at the position where it happened - it never looks like a clean end of stream."""

    _END = object()

    def __init__(self, make_batches, depth=2, pin=False):
        self.q = queue.Queue(maxsize=max(1, depth))
        self.pin = pin
        self._stop = threading.Event()
        self.thread = threading.Thread(target=self._run, args=(make_batches,))
        self.thread.daemon = True
        self.thread.start()

    def _put(self, item):
        while not self._stop.is_set():
            try:
                self.q.put(item, timeout=0.05)
                return True
            except queue.Full:
                continue
        return False

    def _run(self, make_batches):
        try:
            for batch in make_batches:
                if self.pin:
                    import torch
                    # (decoded frames stay uint8 - the device normalises them; everything else travels as float32)
                    batch = {k: (torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint8 if v.dtype == np.uint8 else np.float32)).pin_memory()
                                 if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
                if not self._put(batch):
                    return
            self._put(self._END)
        except BaseException as e:          # handed to the consumer
            self._put(e)

    def __iter__(self):
        while True:
            item = self.q.get()
            if item is self._END:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def close(self):
        """Stop the producer (it may be blocked on a full queue) and drop what is queued."""
        self._stop.set()
        try:
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass
        self.thread.join(timeout=5.0)
