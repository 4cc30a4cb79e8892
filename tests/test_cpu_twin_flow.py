"""The op-level cases of tests/test_gpu_flow.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: sagen_optical_flow and
sagen_flow_encode in plain loops over csrc/flow_core.h) - in a container without a GPU, in the manner of
tests/test_cpu_twin_project.py.  The twin is held to the same tolerance and truncation rule as the kernels; flow.FlowEstimator runs
on it unchanged."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_flow_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_flow import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_flow.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the command-line case needs the device and stays out


def test_the_twin_exports_the_flow_entries(twin):
    import ctypes as C
    from spatialaudiogen_amd._lib import SagenFlowParams
    l = C.CDLL(twin)
    P, I, SZ = C.c_void_p, C.c_int, C.c_size_t
    l.sagen_optical_flow.argtypes = [P, I, I, I, P, P, P, SZ, P]
    l.sagen_optical_flow_scratch_bytes.restype = SZ
    l.sagen_optical_flow_scratch_bytes.argtypes = [I] * 4
    l.sagen_flow_encode.argtypes = [P, I, I, I, P, P, P, SZ, P]
    l.sagen_flow_encode_scratch_bytes.restype = SZ
    l.sagen_flow_encode_scratch_bytes.argtypes = [I] * 3
    n, h, w, levels = 2, 8, 16, 2
    # doubles: the pyramid (8 x 16 + 4 x 8) and one smoothed level per frame, three coefficient planes and three (u, v) fields per pair
    nbytes = l.sagen_optical_flow_scratch_bytes(n, h, w, levels)
    assert nbytes == 8 * (n * (h * w + h * w // 4 + h * w) + (n - 1) * h * w * 9)
    assert l.sagen_optical_flow_scratch_bytes(n, h, w, 3) == 0          # 2 x 4 pixels on the coarsest level: the call would refuse
    assert l.sagen_optical_flow_scratch_bytes(1, h, w, levels) == 0 and l.sagen_optical_flow_scratch_bytes(n, 9, w, levels) == 0
    assert l.sagen_flow_encode_scratch_bytes(3, h, w) == 3 * 64 * 2 * 4 and l.sagen_flow_encode_scratch_bytes(0, h, w) == 0
    prm = SagenFlowParams(levels, 2, 5, 1, 0, 8.)
    frame = bytes((7 * i * i + 3 * i) % 256 for i in range(h * w * 3))
    frames = (C.c_uint8 * (n * h * w * 3))(*(frame + frame))            # twice the same frame: a flow of exactly zero
    flow = (C.c_float * ((n - 1) * h * w * 2))(*([5.] * ((n - 1) * h * w * 2)))
    scratch = (C.c_double * (nbytes // 8))()
    assert l.sagen_optical_flow(frames, n, h, w, C.byref(prm), flow, scratch, nbytes, None) == 0
    assert not any(flow)
    assert l.sagen_optical_flow(None, n, h, w, C.byref(prm), flow, scratch, nbytes, None) == -1
    assert l.sagen_optical_flow(frames, n, h, w, C.byref(prm), flow, scratch, nbytes - 8, None) == -2
    assert l.sagen_optical_flow(frames, n, 9, w, C.byref(prm), flow, scratch, nbytes, None) == -2
    bad = SagenFlowParams(levels, 2, 5, 1, 9, 8.)
    assert l.sagen_optical_flow(frames, n, h, w, C.byref(bad), flow, scratch, nbytes, None) == -3
    assert l.sagen_optical_flow(None, 1, h, w, None, None, None, 0, None) == 0
    # the coding of that zero flow: limits (0, 1), every byte 0
    rgb = (C.c_uint8 * (h * w * 3))(*([9] * (h * w * 3)))
    lim = (C.c_float * 2)(-1., -1.)
    eb = l.sagen_flow_encode_scratch_bytes(1, h, w)
    es = (C.c_float * (eb // 4))()
    assert l.sagen_flow_encode(flow, 1, h, w, rgb, lim, es, eb, None) == 0
    assert list(lim) == [0., 1.] and not any(rgb)
    assert l.sagen_flow_encode(flow, 1, h, w, None, lim, es, eb, None) == -1
    assert l.sagen_flow_encode(flow, 1, 0, w, rgb, lim, es, eb, None) == -2
    assert l.sagen_flow_encode(flow, 1, 4097, w, rgb, lim, es, eb, None) == -3
    assert l.sagen_flow_encode(None, 0, h, w, None, None, None, 0, None) == 0
    assert l.sagen_flow_encode(None, 0, 0, w, None, None, None, 0, None) == 0
    assert l.sagen_flow_encode(None, -1, h, w, None, None, None, 0, None) == -2
