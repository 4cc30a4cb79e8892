"""The op-level cases of tests/test_gpu_resample.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: sagen_resample_fir and
sagen_window_rms in plain loops over csrc/resample_core.h) - in a container without a GPU, in the manner of tests/test_cpu_twin_flow.py.
The twin is held to the same comparison rule as the kernels; resample.Resampler and HrirSet.resampled run on it unchanged."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_resample_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_resample import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_resample.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the command-line cases stay with the device


def test_the_twin_exports_the_resample_entries(twin):
    import ctypes as C
    l = C.CDLL(twin)
    P, I, I64 = C.c_void_p, C.c_int, C.c_int64
    l.sagen_resample_fir.argtypes = [P, I64, I64, I, P, I, I, I, I, P, I, I64, I64, P, P]
    l.sagen_window_rms.argtypes = [P, I64, I, I, I64, I64, I64, I64, P, P]
    # 1 -> 2 with the prototype h = [0.5, 1, 0.5] (H = 1, L = 2, T = 2): phase 0 = [h[0], 0], phase 1 = [h[1], h[-1]]: linear interpolation
    taps = (C.c_double * 4)(1., 0., .5, .5)
    x = (C.c_float * 3)(1., 3., 7.)
    y = (C.c_float * 6)(*([9.] * 6))
    assert l.sagen_resample_fir(x, 0, 3, 1, taps, 2, 1, 1, 2, None, 1, 0, 6, y, None) == 0
    assert list(y) == [1., 2., 3., 5., 7., 3.5]
    mix = (C.c_double * 1)(2.)
    # the same two floats standing for the stream's rows 1 and 2 (row 0 is not in the buffer: zero), doubled by a 1 x 1 mix
    assert l.sagen_resample_fir(x, 1, 2, 1, taps, 2, 1, 1, 2, mix, 1, 1, 3, y, None) == 0
    assert list(y) == [1., 2., 4., 5., 7., 3.5]                   # outputs 1 .. 3 = (0 + 2) / 2, 2, (2 + 6) / 2; the rest untouched
    assert l.sagen_resample_fir(None, 0, 3, 1, taps, 2, 1, 1, 2, None, 1, 0, 6, y, None) == -1
    assert l.sagen_resample_fir(x, 0, 3, 1, taps, 2, 1, 1, 3, None, 1, 0, 6, y, None) == -2
    assert l.sagen_resample_fir(x, 0, 3, 65, taps, 2, 1, 1, 2, None, 65, 0, 6, y, None) == -3
    assert l.sagen_resample_fir(None, 0, 3, 1, None, 0, 0, 0, 0, None, 1, 0, 0, None, None) == 0
    rms = (C.c_double * 2)(9., 9.)
    assert l.sagen_window_rms(x, 3, 1, 0, 0, 1, 2, 2, rms, None) == 0
    assert list(rms) == [5. ** .5, 29. ** .5]
    assert l.sagen_window_rms(x, 3, 1, 0, 0, 2, 2, 2, rms, None) == -2
    assert l.sagen_window_rms(None, 3, 1, 0, 0, 1, 2, 2, rms, None) == -1
    assert l.sagen_window_rms(None, 3, 1, 0, 0, 1, 2, 0, None, None) == 0
