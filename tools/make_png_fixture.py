"""Write tests/golden/png_v1.npz: the small deflate and filter cases of tests/png_oracle.py with what the CPU twin (libsagen_cpu.so) makes
of them.  The twin and the device library must both reproduce these bytes (tests/test_gpu_png.py, tests/test_png_host.py).

    python tools/make_png_fixture.py [OUT.npz]

Every stream is checked with zlib's inflate and every filtered frame against the oracle before anything is written."""
import ctypes as C
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import png_oracle as PO  # noqa: E402

FILTER_RECORDED = ('grey_17x9', 'rgb_17x9', 'rgb_1x1', 'gradient_sub_wins', 'repeated_rows_up_wins', 'tie')


def twin():
    from spatialaudiogen_amd import build
    l = C.CDLL(build.build_cpu_twin())
    P, I, I64 = C.c_void_p, C.c_int, C.c_int64
    l.sagen_png_filter.argtypes = [P, I, I, I, I, P, P]
    l.sagen_deflate.argtypes = [P, I, I64, P, I64, P, P, P, C.c_size_t, P]
    l.sagen_deflate_scratch_bytes.restype = C.c_size_t
    l.sagen_deflate_scratch_bytes.argtypes = [I, I64, I64]
    l.sagen_deflate_max_bytes.restype = I64
    l.sagen_deflate_max_bytes.argtypes = [I64]
    return l


def twin_deflate(l, strings):
    strings = np.ascontiguousarray(strings)
    n, length = strings.shape
    stride = (int(l.sagen_deflate_max_bytes(length)) + 3) // 4 * 4
    out, sizes, status = np.zeros((n, stride), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    need = l.sagen_deflate_scratch_bytes(n, length, stride)
    scratch = np.zeros(need // 8 + 2, np.float64)
    sc = (scratch.ctypes.data + 15) // 16 * 16
    rc = l.sagen_deflate(strings.ctypes.data if length else None, n, length, out.ctypes.data, stride, sizes.ctypes.data, status.ctypes.data, sc, need, None)
    assert rc == 0 and not status.any()
    return out, sizes


def main(path):
    l = twin()
    cases, frames = PO.deflate_cases(), PO.filter_cases()
    arrays = {'names': np.array(PO.RECORDED), 'filter_names': np.array(FILTER_RECORDED)}
    for name in PO.RECORDED:
        out, sizes = twin_deflate(l, cases[name])
        for f in range(out.shape[0]):
            assert zlib.decompress(out[f, :sizes[f]].tobytes()) == cases[name][f].tobytes(), name
        arrays['in_' + name], arrays['out_' + name], arrays['sizes_' + name] = cases[name], out[:, :sizes.max()], sizes
    for name in FILTER_RECORDED:
        fr = np.ascontiguousarray(frames[name])
        comps = 3 if fr.ndim == 4 else 1
        rows = np.zeros(fr.shape[:2] + (1 + fr.shape[2] * comps,), np.uint8)
        assert l.sagen_png_filter(fr.ctypes.data, fr.shape[0], fr.shape[2], fr.shape[1], comps, rows.ctypes.data, None) == 0
        assert np.array_equal(rows, PO.filter_rows(fr)), name
        arrays['rows_' + name] = rows
    np.savez_compressed(path, **arrays)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'png_v1.npz'))
