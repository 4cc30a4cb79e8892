"""The op-level cases of sagen_assemble_frames (include/sagen.h), shared by tests/test_cpu_twin_feed.py (the CPU twin, through ctypes on
numpy arrays) and tests/test_gpu_feed.py (the device library, through torch): the inputs, and the expected output made by the numpy
of the host feed itself - np.roll as JpgFrames.frames rolls, feeder.frames_to_float, and FlowFrames.frames run on a stand-in for its
decoder.  Everything is compared as bit patterns: there is no tolerance anywhere in these cases.

A `call` is   call(frames uint8 [n_frames, h, w, 3], index int32 [n_out], shift int32 [n_out], mode, table float32 or None,
                   scale_lo float64 [n_frames, 2] or None) -> numpy [n_out, h, w, 3] (uint8 in mode 0, float32 otherwise)."""
import numpy as np

from spatialaudiogen_amd import feeder as F
from util import rng

SHAPES = [(1, 1), (2, 5), (3, 64), (3, 65), (16, 16)]
INDEX = [2, 0, -1, 2, 7, 1]                     # a repeat, a padding item, an out-of-range item (zeros too), more outputs than frames
N_FRAMES = 3


def shifts(w):
    return [0, 1, w - 1, -1, w + 3, 0]


def frames_of(h, w, seed=0):
    """[3, h, w, 3] uint8; at 16 x 16 every frame holds all 256 byte values in channel 0 and a permutation of them in channel 2"""
    r = rng(100 * h + w + seed)
    fr = r.integers(0, 256, size=(N_FRAMES, h, w, 3)).astype(np.uint8)
    if h * w == 256:
        for f in range(N_FRAMES):
            fr[f, :, :, 0] = np.roll(np.arange(256), 37 * f).reshape(h, w)
            fr[f, :, :, 2] = r.permutation(256).reshape(h, w)
    return fr


def limits_of(dtype):
    """rows of flow_limits.npy: lo = 0, lo == hi, lo > 0"""
    return np.array([[0., 3.7], [1.25, 1.25], [0.3, 9.1]]).astype(dtype)


def video_table():
    return F.frames_to_float(np.arange(256).astype(np.uint8))


def flow_table():
    """cos[256] then sin[256] of the angle a byte stands for, by the expressions of FlowFrames.frames: a float32 array scaled in
    place by the Python scalar, then np.cos / np.sin of it"""
    a = np.arange(256).astype(np.float32)
    a *= (2 * np.pi) / 255.
    return np.concatenate([np.cos(a), np.sin(a)])


def scale_lo_of(limits):
    """((hi - lo) / 255., lo) per frame as FlowFrames.frames computes them, in the file's dtype, then widened"""
    lo, hi = limits[:, 0], limits[:, 1]
    return np.ascontiguousarray(np.stack([(hi - lo) / 255., lo], 1).astype(np.float64))


class _Decoded(object):
    """stands where FlowFrames keeps its JpgFrames: serves frames that are decoded (and rolled) already"""

    def __init__(self, clip):
        self.clip = clip

    def frames(self, first, count, rotation=None):
        return self.clip[first:first + count]


def expected(frames, index, shift, mode, limits=None):
    n_frames, h, w = frames.shape[:3]
    out = np.zeros((len(index), h, w, 3), np.uint8 if mode == 0 else np.float32)
    for i, (f, s) in enumerate(zip(index, shift)):
        if not 0 <= f < n_frames:
            continue                                                  # padding: zeros
        rolled = np.roll(frames, int(s), axis=2)                      # JpgFrames.frames: np.roll(clip, shift, axis=2)
        if mode == 0:
            out[i] = rolled[f]
        elif mode == 1:
            out[i] = F.frames_to_float(rolled[f:f + 1])[0]
        else:
            ff = object.__new__(F.FlowFrames)
            ff.jpgs, ff.limits, ff.flow_prep = _Decoded(rolled), limits, None
            out[i] = ff.frames(f, 1)[0]
    return out


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, '%d of %d elements differ, the first at %d' % (bad.size, got.size, bad[0])


def check_shape(call, h, w):
    """modes 0 and 1, and mode 2 for a float32 and a float64 limits file, at one frame size"""
    fr = frames_of(h, w)
    index, shift = np.array(INDEX, np.int32), np.array(shifts(w), np.int32)
    same_bits(call(fr, index, shift, 0, None, None), expected(fr, index, shift, 0))
    same_bits(call(fr, index, shift, 1, video_table(), None), expected(fr, index, shift, 1))
    for dtype in (np.float32, np.float64):
        lim = limits_of(dtype)
        got = call(fr, index, shift, 2, flow_table(), scale_lo_of(lim))
        same_bits(got, expected(fr, index, shift, 2, lim))
        if h * w == 256:                                              # not vacuous: every angle byte met a magnitude that is not zero
            assert np.count_nonzero(got[0, ..., 2]) >= 250 and len(set(fr[2, :, :, 0].reshape(-1))) == 256


def check_no_frames(call, h=3, w=65):
    """n_frames == 0: everything is padding, in every mode, whatever the index says"""
    fr = np.zeros((0, h, w, 3), np.uint8)
    index, shift = np.array([0, -1, 5], np.int32), np.array([1, 2, 3], np.int32)
    for mode, table in ((0, None), (1, video_table()), (2, flow_table())):
        got = call(fr, index, shift, mode, table, None)
        same_bits(got, np.zeros((3, h, w, 3), np.uint8 if mode == 0 else np.float32))


def check_any_int32_shift(call, h=3, w=65):
    """the modulo is the mathematical one over all of int32"""
    fr = frames_of(h, w, seed=1)
    shift = np.array([2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1, 65 * 1000, -65 * 1000 - 1, 2 ** 30], np.int32)
    index = np.array([0, 1, 2, 0, 1, 2], np.int32)
    want = np.stack([np.roll(fr[f], int(s) % w, axis=1) for f, s in zip(index, shift)], 0)
    same_bits(call(fr, index, shift, 0, None, None), want)
    lim = limits_of(np.float64)
    same_bits(call(fr, index, shift, 2, flow_table(), scale_lo_of(lim)), expected(fr, index, shift, 2, lim))
