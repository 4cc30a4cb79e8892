"""The op-level cases of tests/test_gpu_jpeg.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: sagen_jpeg_decode as
plain loops over csrc/jpeg_core.h) - in a container without a GPU, in the manner of tests/test_cpu_twin_project.py - and the
DAMAGED streams, which go to the twin and to a sanitizer build of the same host loop only, never to a device.

Mutations (deterministic, of fixture streams): the file cut at every eighth byte of its scan, the end-of-block symbol of a frame's
AC table replaced by the run-of-16 symbol, a restart marker moved one byte forward.  For each: the call returns, every damaged frame
has a status, the intact frames of the same call have status 0 and exactly the fixture's pixels."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_jpeg_host import fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_jpeg_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_jpeg import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_jpeg.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the flagship-sized call and the command lines need the device and stay out


def test_the_twin_returns_the_documented_codes(twin):
    import ctypes as C
    from spatialaudiogen_amd import jpeg
    names, data, rgb, _ = fixture()
    l = C.CDLL(twin)
    P, I = C.c_void_p, C.c_int
    l.sagen_jpeg_decode.argtypes = [P, C.c_int64, P, I, P, I, P, I, P, I, I, I, I, I, I, P, P, P, C.c_size_t, P]
    l.sagen_jpeg_decode_scratch_bytes.restype = C.c_size_t
    l.sagen_jpeg_decode_scratch_bytes.argtypes = [I] * 7
    d = data['grey_8x8_q75']
    p = jpeg.pack([d], [jpeg.parse(d)])
    buf = np.zeros(p.buffer.size // 8 + 1, np.float64)
    buf.view(np.uint8)[:p.buffer.size] = p.buffer
    base = buf.ctypes.data
    out, status = np.full((1, 8, 8, 3), 9, np.uint8), np.full(1, -1, np.int32)
    need = l.sagen_jpeg_decode_scratch_bytes(1, 8, 8, 1, 1, 1, p.n_hufftabs)
    assert need == 912 * p.n_hufftabs + 128 + 64                     # derived tables, one block of coefficients, one 8 x 8 plane
    scratch = np.zeros(need // 8 + 2, np.float64)
    sc = (scratch.ctypes.data + 15) // 16 * 16

    def call(n=1, w=8, comps=1, hs=1, total=p.total_bytes, o=out.ctypes.data, sc_bytes=need, b=base + p.bytes_at):
        return l.sagen_jpeg_decode(b, total, base + p.frames_at, n, base + p.segments_at, p.n_segments, base + p.qtabs_at, p.n_qtabs,
                                   base + p.hufftabs_at, p.n_hufftabs, w, 8, comps, hs, 1, o, status.ctypes.data, sc, sc_bytes, None)

    assert call(o=None) == -1 and call(b=None) == -1
    assert call(n=-1) == -2 and call(w=0) == -2 and call(total=p.total_bytes + 2) == -2 and call(n=2) == -2        # (n_segments < n)
    assert call(comps=2) == -3 and call(hs=2) == -3 and call(w=16385) == -3 and call(n=65536) == -3
    assert call(sc_bytes=need - 1) == -5
    assert (out == 9).all() and status[0] == -1
    assert call(n=0) == 0 and (out == 9).all()
    assert call() == 0 and status[0] == 0 and np.array_equal(out[0], rgb['grey_8x8_q75'])


# ---- damaged streams ----------------------------------------------------------------------------------------------------------------
GROUPS = (['420_17x23_q75', '420_17x23_q1', '420_17x23_q100_opt', '420_17x23_q30_rows'], ['420_48x64_q75_blocks', '420_48x64_q95_opt'],
          ['422_40x56_q75_rows'], ['grey_9x31_q100'])


def _eob_to_zrl(spec):
    t = bytearray(spec)
    total = sum(t[:16])
    at = t.index(0, 16, 16 + total) if 0 in t[16:16 + total] else 16
    t[at] = 0xF0
    return bytes(t)


def mutation_cases():
    """[(what, datas, infos, damaged flags, expected pixels)]: one damaged frame per case, among the intact others of its group."""
    from spatialaudiogen_amd import jpeg
    names, data, rgb, _ = fixture()
    cases = []
    for group in GROUPS:
        datas, infos = [data[n] for n in group], [jpeg.parse(data[n]) for n in group]
        expected = np.stack([rgb[n] for n in group], 0)

        def add(what, f, d, i):
            flags = np.zeros(len(group), np.int32)
            flags[f] = 1
            cases.append(('%s of %s' % (what, group[f]), datas[:f] + [d] + datas[f + 1:], infos[:f] + [i] + infos[f + 1:], flags, expected))

        for f, (d, i) in enumerate(zip(datas, infos)):
            if i.scan_bytes <= 600:                                  # (the 3108-byte stream would add 388 cases that show nothing new)
                for cut in range(8, i.scan_bytes, 8):
                    add('cut at byte %d' % cut, f, d[:i.scan_offset + cut], i._replace(scan_bytes=cut, segments=i.segments[i.segments <= cut]))
            add('EOB -> ZRL', f, d, i._replace(actabs=[_eob_to_zrl(t) for t in i.actabs]))
            for k in range(1, i.segments.size):
                at = i.scan_offset + int(i.segments[k])
                moved = d[:at - 3] + d[at - 2:at] + d[at - 3:at - 2] + d[at:]
                seg = i.segments.copy()
                seg[k] -= 1
                add('restart marker %d moved' % k, f, moved, i._replace(segments=seg))
    return cases


def test_mutations_cover_the_three_kinds():
    cases = mutation_cases()
    for word, least in (('cut at', 150), ('EOB -> ZRL', 8), ('moved', 12)):
        assert sum(word in c[0] for c in cases) >= least, word


def test_damaged_streams_are_flagged_and_leave_their_neighbours_exact(twin):
    from test_gpu_jpeg import _twin_decode
    kinds = {}
    for what, datas, infos, flags, expected in mutation_cases():
        got, status = _twin_decode(datas, infos)                     # (returns: the call came back with SAGEN_OK)
        for k in range(len(datas)):
            if flags[k]:
                assert status[k] != 0, what
                kinds[int(status[k])] = kinds.get(int(status[k]), 0) + 1
            else:
                assert status[k] == 0 and np.array_equal(got[k], expected[k]), (what, k)
    print('status words seen on damaged frames:', sorted(kinds.items()))
    assert len(kinds) >= 3                                           # truncation, a bad run and a misplaced marker do not all look alike


def test_sanitizer_build_of_the_host_loop_runs_the_mutations_clean(tmp_path):
    """tools/jpeg_mutate.cpp with -fsanitize=address,undefined: a plain executable on the CPU, every array in a heap block of its
    exact size."""
    from spatialaudiogen_amd import jpeg
    cxx = os.environ.get('CXX', 'g++')
    exe = str(tmp_path / 'jpeg_mutate')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'tools', 'jpeg_mutate.cpp'), '-o', exe], capture_output=True, text=True)
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
    assert 'jpeg_mutate: %d cases' % len(cases) in r.stdout and 'ERROR' not in r.stderr and 'runtime error' not in r.stderr
