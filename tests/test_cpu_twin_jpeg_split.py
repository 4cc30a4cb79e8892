"""The op-level cases of tests/test_gpu_jpeg_split.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: sagen_jpeg_decode_split
as plain loops over csrc/jpeg_split_core.h, the same stages, rounds and path as the kernels) - in a container without a GPU, in the
manner of tests/test_cpu_twin_jpeg_rst.py - all 290 damaged streams of tests/test_cpu_twin_jpeg.py through the twin, and a sanitizer
build of the same host loop as a stand-alone program (tools/jpeg_split_mutate.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_cpu_twin_jpeg import mutation_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_jpeg_split_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_jpeg_split import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_jpeg_split.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert '1 deselected' in r.stdout                   # the comparison of the device with the twin needs the device and stays out


def test_all_damaged_streams_equal_the_one_lane_path(twin):
    """Every mutation at chunks of 16 bytes with 8 rounds and of 64 bytes with 1: status equal for every frame, healthy neighbours
    exact, path non-zero exactly where status is (a frame the descriptor check refused apart: nobody decodes it) or the frame was
    unsettled."""
    from spatialaudiogen_amd import jpeg
    from test_gpu_jpeg import _twin_decode
    from test_gpu_jpeg_split import check_damaged, twin_split
    cases = mutation_cases()
    assert len(cases) == 290
    paths = {}
    for what, datas, infos, flags, expected in cases:
        ref, ref_status = _twin_decode(datas, infos)
        packed = jpeg.pack(datas, infos)
        for chunk_bytes, rounds in ((16, 8), (64, 1)):
            out, status, path = twin_split(packed, chunk_bytes, rounds, jpeg.split_chunks(packed, chunk_bytes))
            assert np.array_equal(status, ref_status), (what, chunk_bytes, status, ref_status)
            seen = (status & 16) == 0
            assert np.array_equal(out[seen], ref[seen]), (what, chunk_bytes, path)
            check_damaged(what, datas, infos, flags, expected, out, status, path)
            for v in path.tolist():
                paths[v] = paths.get(v, 0) + 1
    print('path values over the damaged calls:', sorted(paths.items()))
    assert paths.get(0, 0) > 0 and paths.get(2, 0) > 0                # split frames next to anomalous ones


def test_sanitizer_build_of_the_host_loop_runs_the_mutations_clean(tmp_path):
    """tools/jpeg_split_mutate.cpp with -fsanitize=address,undefined: a plain executable on the CPU, every array in a heap block of its
    exact size, chunk_bytes 16 and 64, rounds 1 and 8."""
    from spatialaudiogen_amd import jpeg
    cxx = os.environ.get('CXX', 'g++')
    exe = str(tmp_path / 'jpeg_split_mutate')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'tools', 'jpeg_split_mutate.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and ('cannot find' in r.stderr or 'asan' in r.stderr.lower()):
        pytest.skip('this compiler has no sanitizer runtime to link: %s' % r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    cases = mutation_cases()
    with open(str(tmp_path / 'cases.bin'), 'wb') as f:
        f.write(np.int32(len(cases)).tobytes())
        for what, datas, infos, flags, expected in cases:
            p = jpeg.pack(datas, infos)
            w, h, comps, hs, vs = p.geometry
            f.write(np.array([p.n, p.n_segments, p.n_qtabs, p.n_hufftabs, w, h, comps, hs, vs, p.total_bytes], np.int32).tobytes())
            for at, size in ((p.frames_at, 64 * p.n), (p.segments_at, 8 * p.n_segments), (p.qtabs_at, 128 * p.n_qtabs), (p.hufftabs_at, 272 * p.n_hufftabs),
                             (p.bytes_at, p.total_bytes)):
                f.write(p.buffer[at:at + size].tobytes())
            f.write(flags.tobytes())
            f.write(np.ascontiguousarray(expected).tobytes())
    r = subprocess.run([exe, str(tmp_path / 'cases.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    assert 'jpeg_split_mutate: %d cases, %d runs' % (len(cases), 4 * len(cases)) in r.stdout and 'ERROR' not in r.stderr and 'runtime error' not in r.stderr
