"""The op-level cases of tests/test_gpu_jpeg_rst.py - the transcode checks and the `jpeg restart` command line among them - against
the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: sagen_jpeg_encode_rst and sagen_jpeg_transcode as plain loops over
csrc/jpeg_enc_core.h) - in a container without a GPU, in the manner of tests/test_cpu_twin_jpeg_enc.py - the twin
against the fixture through the bare C ABI, the command lines of project and flow with --restart_rows through the twin, and a sanitizer
build of the same host loop as a stand-alone program (tools/jpeg_rst_check.cpp)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_enc_oracle as JE
from test_jpeg_enc_host import FACTORS
from test_jpeg_rst_host import fixture, scan_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_jpeg_rst_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_jpeg_rst import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_jpeg_rst.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]


def test_the_twin_equals_the_fixture_through_the_bare_abi(twin):
    """sizes, bytes and status of every case, in a row of exactly the stride with poison behind it."""
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling, interval = fixture()
    l = C.CDLL(twin)
    P, I = C.c_void_p, C.c_int
    l.sagen_jpeg_encode_rst.argtypes = [P, I, I, I, I, I, I, I, P, P, C.c_int64, P, P, P, C.c_size_t, P]
    l.sagen_jpeg_encode_rst_scratch_bytes.restype = C.c_size_t
    l.sagen_jpeg_encode_rst_scratch_bytes.argtypes = [I] * 7 + [C.c_int64]
    for n in names:
        img, want = np.ascontiguousarray(image[n]), scan_of(data[n])
        h, w = img.shape[:2]
        comps = 1 if img.ndim == 2 else 3
        hs, vs = FACTORS[sampling[n]]
        q = np.ascontiguousarray(jpeg.quality_tables(quality[n])[:, JE.zigzag()])
        stride = (len(want) + 3) // 4 * 4
        out, sizes, status = np.full(stride + 64, 9, np.uint8), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
        need = l.sagen_jpeg_encode_rst_scratch_bytes(1, w, h, comps, hs, vs, interval[n], stride)
        assert need > 0 and need % 16 == 0
        scratch = np.zeros(need // 8 + 2, np.float64)
        sc = (scratch.ctypes.data + 15) // 16 * 16
        assert l.sagen_jpeg_encode_rst(img.ctypes.data, 1, w, h, comps, hs, vs, interval[n], q.ctypes.data, out.ctypes.data, stride, sizes.ctypes.data,
                                       status.ctypes.data, sc, need, None) == 0, n
        assert status[0] == 0 and sizes[0] == len(want) and out[:len(want)].tobytes() == want and (out[len(want):] == 9).all(), n
        out[:] = 9
        assert l.sagen_jpeg_encode_rst(img.ctypes.data, 1, w, h, comps, hs, vs, interval[n], q.ctypes.data, out.ctypes.data, 4, sizes.ctypes.data,
                                       status.ctypes.data, sc, need, None) == 0, n
        assert status[0] == (1 if len(want) > 4 else 0) and sizes[0] == len(want) and (out[4:] == 9).all(), n


def _folder(path, n, h, w, seed):
    from PIL import Image
    os.makedirs(path)
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    for k in range(n):
        a = np.stack([127 + 100 * np.sin((x + 3 * k) / 9.), 127 + 100 * np.cos(y / 7.), (3 * x + 2 * y + 9 * k) % 256], -1) + rs.randint(-8, 9, (h, w, 3))
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(os.path.join(path, '%06d.jpg' % k), quality=95)


CLI = """
import os, sys
from spatialaudiogen_amd import flow, jpeg, project
src, dst = sys.argv[1], sys.argv[2]
for mode in ('host', 'device'):
    project.main([src, os.path.join(dst, 'p_' + mode), '--from', 'er', '--to', 'er', '--size', '24', '48', '--decode', mode, '--encode', mode,
                  '--block', '4', '--restart_rows', '1'])
    flow.main([src, os.path.join(dst, 'f_' + mode), '--levels', '2', '--iters', '4', '--decode', mode, '--encode', mode, '--block', '4',
               '--restart_rows', '1'])
project.main([src, os.path.join(dst, 'p_plain'), '--from', 'er', '--to', 'er', '--size', '24', '48', '--block', '4'])
for kind, count in (('p', 6), ('f', 6)):
    a, b = os.path.join(dst, kind + '_host'), os.path.join(dst, kind + '_device')
    names = sorted(f for f in os.listdir(a) if f.endswith('.jpg'))
    assert names == sorted(f for f in os.listdir(b) if f.endswith('.jpg')) and len(names) == count
    for f in names:
        data = open(os.path.join(a, f), 'rb').read()
        assert data == open(os.path.join(b, f), 'rb').read(), f
        info = jpeg.parse(data)
        assert (info.width, info.height, info.restart_interval, info.segments.size) == (48, 24, 3, 2) if kind == 'p' else info.segments.size > 1, f
assert jpeg.parse(open(os.path.join(dst, 'p_plain', '000000.jpg'), 'rb').read()).restart_interval == 0
for tool in (project, flow):
    try:
        tool.main([src, os.path.join(dst, 'png'), '--format', 'png', '--restart_rows', '1'] + (['--from', 'er', '--to', 'er', '--size', '24', '48'] if tool is project else []))
    except SystemExit as e:
        assert '--restart_rows' in str(e.code), e.code
    else:
        raise AssertionError('png with --restart_rows was not refused')
assert not os.path.exists(os.path.join(dst, 'png'))
print('restart command lines ok')
"""


def test_project_and_flow_write_the_same_segmented_folders_either_way(twin, tmp_path):
    """--restart_rows 1 with --encode host (PIL's restart_marker_rows) and, through the twin, with --encode device."""
    src = str(tmp_path / 'in')
    _folder(src, 6, 32, 64, 5)
    os.makedirs(str(tmp_path / 'out'))
    env = dict(os.environ, SAGEN_LIB=twin, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-c', CLI, src, str(tmp_path / 'out')], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'restart command lines ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_sanitizer_build_of_the_host_loop_runs_the_fixture_clean(tmp_path):
    """tools/jpeg_rst_check.cpp with -fsanitize=address,undefined: a plain executable on the CPU, every array in a heap block of its
    exact size, strides of 4, 64, exactly sizes[f] and the bound; the segment geometry over every small interval."""
    from spatialaudiogen_amd import jpeg
    cxx = os.environ.get('CXX', 'g++')
    exe = str(tmp_path / 'jpeg_rst_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'tools', 'jpeg_rst_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and ('cannot find' in r.stderr or 'asan' in r.stderr.lower()):
        pytest.skip('this compiler has no sanitizer runtime to link: %s' % r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    names, image, data, quality, sampling, interval = fixture()
    with open(str(tmp_path / 'cases.bin'), 'wb') as f:
        f.write(np.int32(len(names)).tobytes())
        for n in names:
            img, want = np.ascontiguousarray(image[n]), scan_of(data[n])
            hs, vs = FACTORS[sampling[n]]
            f.write(np.array([img.shape[1], img.shape[0], 1 if img.ndim == 2 else 3, hs, vs, interval[n], len(want)], np.int32).tobytes())
            f.write(np.ascontiguousarray(jpeg.quality_tables(quality[n])[:, JE.zigzag()]).astype(np.uint16).tobytes())
            f.write(img.tobytes())
            f.write(want)
    r = subprocess.run([exe, str(tmp_path / 'cases.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    assert 'jpeg_rst_check: %d cases, %d runs, %d transcodes' % (len(names), 4 * len(names), 2 * len(names)) in r.stdout and 'ERROR' not in r.stderr and 'runtime error' not in r.stderr
