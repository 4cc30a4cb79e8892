"""The op-level cases of tests/test_gpu_project.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: sagen_reproject
in plain loops over csrc/project_core.h) - in a container without a GPU, in the manner of tests/test_cpu_twin_overlay.py.  The
twin is held to the same pixel rule as the kernel; project.Projector runs on it unchanged."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_project_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_project import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_project.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the command-line case needs the device and stays out


def test_the_twin_exports_the_project_entries(twin):
    import ctypes as C
    from spatialaudiogen_amd._lib import SagenProjection
    l = C.CDLL(twin)
    P, I, SZ = C.c_void_p, C.c_int, C.c_size_t
    l.sagen_reproject.argtypes = [P, I, I, I, P, P, I, I, P, P, I, I, P, SZ, P]
    l.sagen_reproject_scratch_bytes.restype = SZ
    l.sagen_reproject_scratch_bytes.argtypes = [I] * 4
    assert l.sagen_reproject_scratch_bytes(2, 4, 8, 2) == 0
    er = SagenProjection()                               # kind 0, rectangle 0: the whole frame, equirectangular
    # a 2 x 4 frame onto itself: the input; turned by half a turn about z: columns move by two
    src = (C.c_uint8 * 24)(*range(10, 34))
    dst = (C.c_uint8 * 24)()
    assert l.sagen_reproject(src, 1, 2, 4, C.byref(er), dst, 2, 4, C.byref(er), None, 0, 1, None, 0, None) == 0
    assert list(dst) == list(src)
    rot = (C.c_double * 9)(-1., 0., 0., 0., -1., 0., 0., 0., 1.)
    assert l.sagen_reproject(src, 1, 2, 4, C.byref(er), dst, 2, 4, C.byref(er), rot, 1, 1, None, 0, None) == 0
    assert list(dst) == list(src[6:12]) + list(src[0:6]) + list(src[18:24]) + list(src[12:18])
    assert l.sagen_reproject(None, 1, 2, 4, C.byref(er), dst, 2, 4, C.byref(er), None, 0, 1, None, 0, None) == -1
    assert l.sagen_reproject(src, 1, 2, 4, C.byref(er), dst, 2, 4, C.byref(er), rot, 2, 1, None, 0, None) == -2
    assert l.sagen_reproject(src, 1, 2, 4, C.byref(er), dst, 2, 4, C.byref(er), None, 0, 9, None, 0, None) == -3
    view = SagenProjection()
    view.kind = 3
    assert l.sagen_reproject(src, 1, 2, 4, C.byref(view), dst, 2, 4, C.byref(er), None, 0, 1, None, 0, None) == -3
    assert l.sagen_reproject(None, 0, 2, 4, None, None, 2, 4, None, None, 0, 1, None, 0, None) == 0
