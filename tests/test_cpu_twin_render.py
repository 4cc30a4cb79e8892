"""The op-level cases of tests/test_gpu_render.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: sagen_render_fir in
plain C++) - in a container without a GPU, in the manner of tests/test_cpu_twin_ops.py.  The twin is held to the same tolerance
as the kernel, not to the kernel's bits; together with tests/test_render_host.py this shows the feature's arithmetic where no
kernel can run."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_render_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_render import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_render.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the driver-level cases need the device and stay out


def test_the_twin_exports_the_render_entry(twin):
    import ctypes as C
    l = C.CDLL(twin)
    buf = (C.c_float * 16)()
    l.sagen_render_fir.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                   C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    assert l.sagen_render_fir(None, 0, 4, 4, buf, 1, 1, None, 0, 0, 0, 0, buf, None) == -1
    assert l.sagen_render_fir(buf, 0, 4, 5, buf, 1, 1, None, 0, 0, 0, 0, buf, None) == -3
    x = (C.c_float * 16)(*[float(i) for i in range(16)])
    taps = (C.c_float * 8)(1, 0, 0, 1, 0, 0, 0, 0)     # [1 output][4 channels][2 taps]: y[t] = x[t, 0] + x[t - 1, 1]
    y = (C.c_float * 4)()
    assert l.sagen_render_fir(x, 0, 4, 4, taps, 1, 2, None, 0, 0, 0, 0, y, None) == 0
    assert list(y) == [0., 4. + 1., 8. + 5., 12. + 9.]
