"""PNG encode without a GPU: the op-level cases of tests/test_gpu_png.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp:
sagen_png_filter and sagen_deflate as plain loops over csrc/png_core.h), in the manner of tests/test_cpu_twin_jpeg_enc.py; what the two
entry points refuse, with which code and which message, pinned for BOTH libraries by tests/golden/op_refusals_png_v1.txt (the entry
points are written once, csrc/op_entries_png.h; the fixture holds what libsagen_hip.so answered; every call of the table returns before
any launch); and a sanitizer build of the same host loops as a stand-alone program (tools/png_encode_check.cpp).

    python tests/test_png_host.py        prints the lines of the device library of the tree the file lies in
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import png_oracle as PO
from test_op_refusals_host import P, OFF2, OFF1, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'op_refusals_png_v1.txt')
OFF8 = P + 8
CALLS = {
    'sagen_png_filter': (('frames', 'n', 'w', 'h', 'components', 'rows', 'stream'),
                         dict(frames=P, n=2, w=4, h=5, components=3, rows=P, stream=None)),
    'sagen_deflate': (('data', 'n', 'length', 'out', 'stride', 'sizes', 'status', 'scratch', 'scratch_bytes', 'stream'),
                      dict(data=P, n=2, length=300, out=P, stride=512, sizes=P, status=P, scratch=P, scratch_bytes=1 << 20, stream=None)),
}                                                                                       # would launch: never made
UNSUPPORTED = ('components_2', 'components_0', 'w_16385', 'h_16385', 'filter_n_65536', 'n_65536', 'length_above_2_28', 'stride_above_2_28')
ROWS = [
    ('sagen_png_filter', 'filter_empty', dict(n=0, frames=None, rows=None, w=0, h=0, components=7)),
    ('sagen_png_filter', 'filter_n_-1', dict(n=-1)), ('sagen_png_filter', 'w_0', dict(w=0)), ('sagen_png_filter', 'h_0', dict(h=0)),
    ('sagen_png_filter', 'components_2', dict(components=2)), ('sagen_png_filter', 'components_0', dict(components=0)),
    ('sagen_png_filter', 'w_16385', dict(w=16385)), ('sagen_png_filter', 'h_16385', dict(h=16385)), ('sagen_png_filter', 'filter_n_65536', dict(n=65536)),
    ('sagen_png_filter', 'null_frames', dict(frames=None)), ('sagen_png_filter', 'null_rows', dict(rows=None)),
    ('sagen_deflate', 'empty', dict(n=0, data=None, out=None, sizes=None, status=None, scratch=None, length=-1, stride=3)),
    ('sagen_deflate', 'n_-1', dict(n=-1)), ('sagen_deflate', 'length_-1', dict(length=-1)),
    ('sagen_deflate', 'stride_0', dict(stride=0)), ('sagen_deflate', 'stride_-4', dict(stride=-4)), ('sagen_deflate', 'stride_510', dict(stride=510)),
    ('sagen_deflate', 'n_65536', dict(n=65536)), ('sagen_deflate', 'length_above_2_28', dict(length=(1 << 28) + 1)),
    ('sagen_deflate', 'stride_above_2_28', dict(stride=(1 << 28) + 4)),
    ('sagen_deflate', 'null_data', dict(data=None)), ('sagen_deflate', 'null_out', dict(out=None)), ('sagen_deflate', 'null_sizes', dict(sizes=None)),
    ('sagen_deflate', 'null_status', dict(status=None)), ('sagen_deflate', 'null_scratch', dict(scratch=None)),
    ('sagen_deflate', 'out_off_2', dict(out=OFF2)), ('sagen_deflate', 'sizes_off_1', dict(sizes=OFF1)), ('sagen_deflate', 'status_off_2', dict(status=OFF2)),
    ('sagen_deflate', 'scratch_off_8', dict(scratch=OFF8)),
    ('sagen_deflate', 'scratch_too_small', dict(scratch_bytes=1000)), ('sagen_deflate', 'scratch_0', dict(scratch_bytes=0)),
]


def refusal_lines(lib):
    """'<function> <case> <rc> <message>' per row: what the golden file holds."""
    lines = []
    for fn, case, over in ROWS:
        names, valid = CALLS[fn]
        args = dict(valid, **over)
        rc = getattr(lib, fn)(*[args[k] for k in names])
        assert (rc == 0) == ('empty' in case), (case, rc, lib.sagen_last_error())
        lines.append(('%s %s %d %s' % (fn, case, rc, lib.sagen_last_error().decode() if rc else '')).rstrip())
    return lines


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def golden():
    text = open(GOLDEN).read().split('\n')
    assert text[0].startswith('# ')
    return [l for l in text[1:] if l]


def test_png_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_png import OP_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_png.py'), '-m', 'gpu', '-q', '-x', '-k', OP_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the flagship-sized call and the command lines need the device and stay out


def test_the_twin_refuses_as_the_device_library_did(twin):
    assert refusal_lines(_bind(C.CDLL(twin))) == golden()


def test_the_device_library_refuses_as_recorded():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    assert refusal_lines(_lib.lib()) == golden()


def test_every_refusal_of_the_entry_points_is_reached():
    """Each fail(...) statement of csrc/op_entries_png.h is the message of at least one line of the fixture, with every reason
    csrc/png_core.h can give it."""
    text = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'op_entries_png.h')).read()
    formats = re.findall(r'\bfail\([A-Za-z_]+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text)
    assert len(formats) == 2
    messages = [l.split(' ', 3)[3] for l in golden() if len(l.split(' ', 3)) == 4]
    for f in formats:
        fmt = ''.join(re.findall(r'"((?:[^"\\]|\\.)*)"', f))
        pattern = '.*'.join(re.escape(part) for part in re.split(r'%(?:ld|zu|d|g|s)', fmt))
        assert any(re.fullmatch(pattern, m) for m in messages), 'no row of the table reaches: ' + fmt
    core = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'png_core.h')).read()
    reasons = re.findall(r'\*why = "([^"]+)"', core)
    assert len(reasons) == 11
    for reason in reasons:
        assert any(reason in m for m in messages), 'no row of the table gives the reason: ' + reason


def test_the_codes_are_the_documented_ones():
    code = {l.split(' ')[1]: int(l.split(' ')[2]) for l in golden()}
    assert len(code) == len(ROWS)
    assert code['empty'] == 0 and code['filter_empty'] == 0
    assert {code[k] for k in UNSUPPORTED} == {-3}
    assert {code[k] for k in code if k.startswith('null_')} == {-1}
    assert {code[k] for k in code if k.startswith('scratch_') and not k.startswith('scratch_off')} == {-5}
    assert {code[k] for k in code if not k.startswith(('null_', 'scratch_too', 'scratch_0')) and 'empty' not in k and k not in UNSUPPORTED} == {-2}


def test_sanitizer_build_of_the_host_loops_runs_the_fixture_clean(tmp_path):
    """tools/png_encode_check.cpp with -fsanitize=address,undefined: a plain executable on the CPU, every array in a heap block of its
    exact size, strides of 4, exactly sizes[f] and the bound; the length symbols and the token rule swept."""
    cxx = os.environ.get('CXX', 'g++')
    exe = str(tmp_path / 'png_encode_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(ROOT, 'tools', 'png_encode_check.cpp'), '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and ('cannot find' in r.stderr or 'asan' in r.stderr.lower()):
        pytest.skip('this compiler has no sanitizer runtime to link: %s' % r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'png_v1.npz'))
    names, filters = [str(n) for n in z['names']], [str(n) for n in z['filter_names']]
    frames = PO.filter_cases()
    runs = 0
    with open(str(tmp_path / 'cases.bin'), 'wb') as f:
        f.write(np.int32(len(names)).tobytes())
        for n in names:
            strings, out, sizes = np.ascontiguousarray(z['in_' + n]), z['out_' + n], z['sizes_' + n]
            f.write(np.array(strings.shape, np.int32).tobytes() + strings.tobytes())
            for k in range(strings.shape[0]):
                f.write(np.int32(sizes[k]).tobytes() + out[k, :sizes[k]].tobytes())
            runs += 2 + strings.shape[0]
        f.write(np.int32(len(filters)).tobytes())
        for n in filters:
            fr = np.ascontiguousarray(frames[n])
            f.write(np.array([fr.shape[0], fr.shape[2], fr.shape[1], 3 if fr.ndim == 4 else 1], np.int32).tobytes() + fr.tobytes() + z['rows_' + n].tobytes())
    r = subprocess.run([exe, str(tmp_path / 'cases.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    assert 'png_encode_check: %d deflate cases, %d runs, %d filter cases' % (len(names), runs, len(filters)) in r.stdout
    assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from spatialaudiogen_amd import _lib
    print('\n'.join(refusal_lines(_lib.lib())))
