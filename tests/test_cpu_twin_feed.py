"""sagen_assemble_frames of the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: plain loops over csrc/feed_core.h) against the numpy
of the host feed - JpgFrames.frames' roll, frames_to_float, FlowFrames.frames - as bit patterns, in a container without a GPU.  The
cases are tests/feed_cases.py; tests/test_gpu_feed.py runs the same ones through the device library."""
import ctypes as C

import numpy as np
import pytest

import feed_cases as FC


@pytest.fixture(scope='module')
def call():
    from spatialaudiogen_amd import build, _lib
    l = C.CDLL(build.build_cpu_twin())
    l.sagen_assemble_frames.restype, l.sagen_assemble_frames.argtypes = _lib.SIGNATURES['sagen_assemble_frames']
    l.sagen_last_error.restype = C.c_char_p

    def run(frames, index, shift, mode, table, scale_lo):
        frames, index, shift = np.ascontiguousarray(frames), np.ascontiguousarray(index, np.int32), np.ascontiguousarray(shift, np.int32)
        n_frames, h, w = frames.shape[:3]
        out = np.full((len(index), h, w, 3), 0xAB, np.uint8) if mode == 0 else np.full((len(index), h, w, 3), np.nan, np.float32)
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        table = None if table is None else np.ascontiguousarray(table, np.float32)
        rc = l.sagen_assemble_frames(ptr(frames), n_frames, h, w, ptr(index), ptr(shift), len(index), mode, ptr(table), ptr(scale_lo),
                                     ptr(out), None)
        assert rc == 0, l.sagen_last_error()
        return out
    return run


@pytest.mark.parametrize('h,w', FC.SHAPES)
def test_every_mode_equals_the_host_feed_bit_for_bit(call, h, w):
    FC.check_shape(call, h, w)


def test_no_frames_is_all_padding(call):
    FC.check_no_frames(call)


def test_any_int32_is_a_shift(call):
    FC.check_any_int32_shift(call)


def test_the_tables_equal_numpy_at_every_position_of_a_strided_view():
    """What the table form rests on: np.sin / np.cos of the strided [..., 0] view of a float32 frame array, as FlowFrames.frames
    calls them, give at every position the value of the 256-entry table (one value per byte, wherever it stands)."""
    r = FC.rng(3)
    b = r.integers(0, 256, size=(2, 32, 48, 3)).astype(np.uint8)
    out = b.astype(np.float32)
    out[..., 0] *= (2 * np.pi) / 255.
    t = FC.flow_table()
    FC.same_bits(np.cos(out[..., 0]), t[:256][b[..., 0]])
    FC.same_bits(np.sin(out[..., 0]), t[256:][b[..., 0]])
