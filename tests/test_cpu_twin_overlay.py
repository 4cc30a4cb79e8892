"""The op-level cases of tests/test_gpu_overlay.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp:
sagen_power_map_windows and sagen_overlay_blend in plain C++) - in a container without a GPU, in the manner of
tests/test_cpu_twin_render.py.  The twin is held to the same bars as the kernels (the maps' tolerance, the blend's pixel rule), not
to their bits; overlay.Overlay's stream logic runs on it unchanged."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_overlay_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_overlay import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_overlay.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the driver-level cases need the device and stay out


def test_the_twin_exports_the_overlay_entries(twin):
    import ctypes as C
    l = C.CDLL(twin)
    P, I, I64, SZ = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    l.sagen_power_map_windows.argtypes = [P, I64, I, I, I64, P, I, P, P, SZ, P]
    l.sagen_overlay_blend.argtypes = [P, I, I64, I, I, P, P, I, I64, I, I, I, P, P, SZ, P]
    l.sagen_power_map_windows_scratch_bytes.restype = l.sagen_overlay_blend_scratch_bytes.restype = SZ
    # two windows of two samples at stride 2 from a W-only stream, two nodes: rms = |W| sh[p][0]
    x = (C.c_float * 32)(*([3., 0, 0, 0, 9, 9, 9, 9] * 2 + [4., 0, 0, 0, 9, 9, 9, 9] * 2))
    sh = (C.c_float * 8)(1., 0, 0, 0, 0.5, 0, 0, 0)
    rms = (C.c_float * 4)()
    # the twin checks the scratch as the device library does (the entry points are shared: csrc/op_entries.h) and does not use it
    assert l.sagen_power_map_windows_scratch_bytes(2, 4) == 2 * 10 * 8
    scratch = (C.c_double * 20)()
    assert l.sagen_power_map_windows(x, 8, 4, 2, 2, sh, 2, rms, scratch, 160, None) == 0
    assert list(rms) == [3., 1.5, 4., 2.]
    assert l.sagen_power_map_windows(x, 8, 4, 2, 2, sh, 2, rms, scratch, 159, None) == -5
    assert l.sagen_power_map_windows(None, 8, 4, 2, 2, sh, 2, rms, scratch, 160, None) == -1
    assert l.sagen_power_map_windows(x, 8, 5, 2, 2, sh, 2, rms, scratch, 160, None) == -3
    assert l.sagen_power_map_windows(x, 8, 4, 0, 2, sh, 2, rms, scratch, 160, None) == -2
    assert l.sagen_power_map_windows(None, 2, 4, 2, 2, None, 2, None, None, 0, None) == 0          # no map fits: nothing is looked at
    # two flat maps: v = 0, alpha = 0 - the frames come back; a frame without its `cur` map is refused
    maps = (C.c_float * 4)(1., 1., 2., 2.)
    lut = (C.c_double * 768)(*([0.5] * 768))
    frames = (C.c_uint8 * 18)(*range(10, 28))
    out = (C.c_uint8 * 18)()
    # the device library's number (csrc/host_sizes.h): the grid of per-node (r, g, b, v) doubles rounded up to 256 bytes, then 4 doubles of clip bounds per frame
    need = (3 * 1 * 2 * 4 * 8 + 255) // 256 * 256 + 3 * 4 * 8
    assert l.sagen_overlay_blend_scratch_bytes(2, 1, 2, 3) == need
    blend_scratch = (C.c_double * (need // 8 + 2))()
    sp = (C.addressof(blend_scratch) + 15) // 16 * 16
    assert l.sagen_overlay_blend(maps, 2, 0, 1, 2, lut, frames, 3, 0, 1, 2, 5, out, sp, need, None) == 0
    assert list(out) == list(frames)
    assert l.sagen_overlay_blend(maps, 2, 0, 1, 2, lut, frames, 3, 0, 1, 2, 5, out, sp, need - 1, None) == -5
    assert l.sagen_overlay_blend(maps, 2, 0, 1, 2, lut, frames, 3, 3, 1, 2, 5, out, sp, need, None) == -2
    assert l.sagen_overlay_blend(maps, 2, 0, 1, 2, None, frames, 3, 0, 1, 2, 5, out, sp, need, None) == -1
    assert l.sagen_overlay_blend(maps, 2, 0, 1, 2, lut, frames, 0, 99, 1, 2, 5, out, None, 0, None) == 0
