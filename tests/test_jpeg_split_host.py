"""The split JPEG decode, the host side (no GPU): what sagen_jpeg_decode_split refuses, with which code and message, pinned for BOTH
libraries by tests/golden/op_refusals_jpeg_split_v1.txt (the entry points are csrc/op_entries_jpeg_split.h, written once);
jpeg.split_chunks against a count by hand; what --entropy and its Python counterparts refuse, before any file is touched.

    python tests/test_jpeg_split_host.py        prints the refusal lines of the device library of the tree the file lies in"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from test_jpeg_host import fixture
from test_jpeg_rst_host import fixture as rst_fixture
from test_op_refusals_host import P, OFF2, OFF1, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'op_refusals_jpeg_split_v1.txt')

OFF8 = P + 8
NAMES = ('bytes', 'total_bytes', 'frames', 'n', 'segments', 'n_segments', 'qtabs', 'n_qtabs', 'hufftabs', 'n_hufftabs', 'w', 'h', 'components', 'hs', 'vs',
         'out', 'status', 'scratch', 'scratch_bytes', 'stream', 'chunk_bytes', 'rounds', 'max_chunks', 'path')
VALID = dict(bytes=P, total_bytes=4096, frames=P, n=2, segments=P, n_segments=2, qtabs=P, n_qtabs=2, hufftabs=P, n_hufftabs=4, w=17, h=23, components=3,
             hs=2, vs=2, out=P, status=P, scratch=P, scratch_bytes=1 << 20, stream=None, chunk_bytes=512, rounds=6, max_chunks=64, path=P)   # would run: never made
UNSUPPORTED = ('components_2', 'sampling_1x2', 'w_16385', 'h_16385', 'n_65536', 'total_bytes_2_31', 'n_hufftabs_65537', 'n_qtabs_65537', 'blocks_2_31')
ROWS = [
    ('empty', dict(n=0, bytes=None, frames=None, segments=None, qtabs=None, hufftabs=None, out=None, status=None, scratch=None, w=0, chunk_bytes=0, rounds=0,
                   max_chunks=-1, path=OFF1)),
    ('n_-1', dict(n=-1)), ('w_0', dict(w=0)), ('h_0', dict(h=0)), ('total_bytes_-4', dict(total_bytes=-4)), ('total_bytes_4094', dict(total_bytes=4094)),
    ('n_segments_1', dict(n_segments=1)), ('n_qtabs_0', dict(n_qtabs=0)), ('n_hufftabs_0', dict(n_hufftabs=0)),
    ('components_2', dict(components=2)), ('sampling_1x2', dict(hs=1, vs=2)), ('w_16385', dict(w=16385)), ('h_16385', dict(h=16385)),
    ('n_65536', dict(n=65536, n_segments=65536, max_chunks=65536)), ('total_bytes_2_31', dict(total_bytes=1 << 31)),
    ('n_hufftabs_65537', dict(n_hufftabs=65537)), ('n_qtabs_65537', dict(n_qtabs=65537)),
    ('blocks_2_31', dict(n=65535, n_segments=65535, max_chunks=65535, w=16384, h=16384)),
    ('null_bytes', dict(bytes=None)), ('null_frames', dict(frames=None)), ('null_segments', dict(segments=None)), ('null_qtabs', dict(qtabs=None)),
    ('null_hufftabs', dict(hufftabs=None)), ('null_out', dict(out=None)), ('null_status', dict(status=None)), ('null_scratch', dict(scratch=None)),
    ('bytes_off_2', dict(bytes=OFF2)), ('frames_off_4', dict(frames=P + 4)), ('segments_off_2', dict(segments=OFF2)), ('qtabs_off_1', dict(qtabs=OFF1)),
    ('status_off_1', dict(status=OFF1)), ('scratch_off_8', dict(scratch=OFF8)),
    ('chunk_bytes_12', dict(chunk_bytes=12)), ('chunk_bytes_18', dict(chunk_bytes=18)), ('chunk_bytes_0', dict(chunk_bytes=0)),
    ('chunk_bytes_65540', dict(chunk_bytes=65540)), ('rounds_0', dict(rounds=0)), ('rounds_65', dict(rounds=65)),
    ('max_chunks_1', dict(max_chunks=1)), ('max_chunks_2_31', dict(max_chunks=1 << 31)), ('path_off_2', dict(path=OFF2)), ('path_off_1', dict(path=OFF1)),
    ('scratch_too_small', dict(scratch_bytes=1000)), ('scratch_0', dict(scratch_bytes=0)), ('scratch_of_the_one_lane_call', dict(scratch_bytes='lane')),
    ('scratch_one_short', dict(scratch_bytes='short')),
]
QUERIES = [('sagen_jpeg_decode_split_scratch_bytes', a) for a in ((2, 17, 23, 3, 2, 2, 4, 2, 64), (2, 17, 23, 3, 2, 2, 4, 2, 2), (2, 17, 23, 3, 2, 2, 4, 2, 1),
                                                                  (2, 17, 23, 3, 2, 2, 4, 1, 64), (2, 17, 23, 3, 2, 2, 4, 2, 1 << 31), (0, 17, 23, 3, 2, 2, 4, 2, 64),
                                                                  (2, 17, 23, 3, 1, 2, 4, 2, 64), (2, 17, 23, 3, 2, 2, 0, 2, 64), (2, 17, 23, 1, 1, 1, 2, 300, 300))]


def refusal_lines(lib):
    """'<function> <case> <rc> <message>' per row, '<query> <arguments> <value>' per size query: what the golden file holds."""
    lines = []
    lane = int(lib.sagen_jpeg_decode_scratch_bytes(2, 17, 23, 3, 2, 2, 4))
    need = int(lib.sagen_jpeg_decode_split_scratch_bytes(2, 17, 23, 3, 2, 2, 4, 2, 64))
    for case, over in ROWS:
        args = dict(VALID, **over)
        args['scratch_bytes'] = {'lane': lane, 'short': need - 1}.get(args['scratch_bytes'], args['scratch_bytes'])
        rc = lib.sagen_jpeg_decode_split(*[args[k] for k in NAMES])
        assert (rc == 0) == (case == 'empty'), (case, rc, lib.sagen_last_error())
        lines.append(('sagen_jpeg_decode_split %s %d %s' % (case, rc, lib.sagen_last_error().decode() if rc else '')).rstrip())
    for fn, a in QUERIES:
        lines.append('%s %s %d' % (fn, ','.join(str(v) for v in a), getattr(lib, fn)(*a)))
    return lines


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def golden():
    text = open(GOLDEN).read().split('\n')
    assert text[0].startswith('# ')
    return [l for l in text[1:] if l]


def test_the_twin_refuses_as_recorded(twin):
    assert refusal_lines(_bind(C.CDLL(twin))) == golden()


def test_the_device_library_refuses_as_recorded():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    assert refusal_lines(_lib.lib()) == golden()


def test_every_refusal_of_the_entry_point_is_reached():
    text = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'op_entries_jpeg_split.h')).read()
    formats = re.findall(r'\bfail\([A-Za-z_]+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text)
    assert len(formats) == 1
    mine = [l.split(' ', 3)[3] for l in golden() if l.startswith('sagen_jpeg_decode_split ') and len(l.split(' ', 3)) == 4]
    fmt = ''.join(re.findall(r'"((?:[^"\\]|\\.)*)"', formats[0]))
    pattern = '.*'.join(re.escape(part) for part in re.split(r'%(?:ld|zu|d|g|s)', fmt))
    assert mine and all(re.fullmatch(pattern, m) for m in mine)
    core = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'jpeg_split_core.h')).read()
    reasons = re.findall(r'\*why = "([^"]+)"', core)
    assert len(reasons) == 5
    plain = re.findall(r'\*why = "([^"]+)"', open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'jpeg_core.h')).read())
    for reason in reasons + [r for r in plain if r != 'scratch too small']:     # (the one-lane size check is passed an unbounded size: the split's own decides)
        assert any(reason in m for m in mine), 'no row of the table gives the reason: ' + reason


def test_the_codes_and_sizes_are_the_documented_ones():
    lines = golden()
    code = {l.split(' ')[1]: int(l.split(' ')[2]) for l in lines if l.startswith('sagen_jpeg_decode_split ')}
    assert len(code) == len(ROWS) and code['empty'] == 0
    assert {code[k] for k in UNSUPPORTED} == {-3}
    assert {code[k] for k in code if k.startswith('null_')} == {-1}
    assert {code[k] for k in code if k.startswith('scratch_') and not k.startswith('scratch_off')} == {-5}
    assert {code[k] for k in code if not k.startswith(('null_', 'scratch_too', 'scratch_0', 'scratch_of', 'scratch_one')) and k != 'empty' and k not in UNSUPPORTED} == {-2}
    value = {l.split(' ')[1]: int(l.split(' ')[2]) for l in lines if l.startswith('sagen_jpeg_decode_split_scratch_bytes ')}
    assert len(value) == len(QUERIES)
    sc = lambda *a: value[','.join(str(v) for v in a)]
    lane = 4 * 912 + 2 * 24 * 128 + (2 * (32 * 32 + 2 * 16 * 16) + 15) // 16 * 16    # tables, 2 x 2 MCUs of 6 blocks, the padded planes
    assert sc(2, 17, 23, 3, 2, 2, 4, 2, 64) > sc(2, 17, 23, 3, 2, 2, 4, 2, 2) > lane and sc(2, 17, 23, 3, 2, 2, 4, 2, 64) % 16 == 0
    a16 = lambda x: (x + 15) // 16 * 16
    tables = lambda m: 3 * a16(4 * m) + 3 * a16(8 * m)                # per chunk: its row, blocks, prefix (int32); entry and two exits (64 bits)
    assert sc(2, 17, 23, 3, 2, 2, 4, 2, 64) - sc(2, 17, 23, 3, 2, 2, 4, 2, 2) == tables(64) - tables(2) == 64 * 36 - 96
    assert sc(2, 17, 23, 3, 2, 2, 4, 2, 1) == sc(2, 17, 23, 3, 2, 2, 4, 1, 64) == sc(2, 17, 23, 3, 2, 2, 4, 2, 1 << 31) == 0
    assert sc(0, 17, 23, 3, 2, 2, 4, 2, 64) == sc(2, 17, 23, 3, 1, 2, 4, 2, 64) == sc(2, 17, 23, 3, 2, 2, 0, 2, 64) == 0
    assert sc(2, 17, 23, 1, 1, 1, 2, 300, 300) > 0


def test_split_chunks_against_a_count_by_hand():
    from spatialaudiogen_amd import jpeg
    names, data, _, _ = fixture()
    rnames, _, rdata = rst_fixture()[:3]
    d = data['420_17x23_q75']
    i = jpeg.parse(d)
    assert i.segments.size == 1
    p = jpeg.pack([d], [i])
    for cb in (16, 20, 64, 65536):
        assert jpeg.split_chunks(p, cb) == -(-i.scan_bytes // cb)
    assert jpeg.split_chunks(p, i.scan_bytes) == 1 and jpeg.split_chunks(p, (i.scan_bytes + 3) // 4 * 4 - 4) == 2
    # a segmented file: every segment by itself, the two marker bytes between them left out; one of a single byte still has a chunk
    n = '444_40x72_q100_noise_rrow'
    d = rdata[n]
    i = jpeg.parse(d)
    starts = [int(s) for s in i.segments]
    lengths = [e - s for s, e in zip(starts, [s - 2 for s in starts[1:]] + [i.scan_bytes])]
    assert len(lengths) > 2 and sum(lengths) + 2 * (len(lengths) - 1) == i.scan_bytes
    for cb in (16, 64, 1024):
        assert jpeg.split_chunks(jpeg.pack([d], [i]), cb) == sum(max(1, -(-l // cb)) for l in lengths)
        assert jpeg.split_chunks(jpeg.pack([d, d, d], [i, i, i]), cb) == 3 * sum(max(1, -(-l // cb)) for l in lengths)
    assert jpeg.split_chunks(jpeg.pack([d], [i]), 65536) == len(lengths)
    empty = i._replace(scan_bytes=0, segments=i.segments[:1], restart_interval=0)
    assert jpeg.split_chunks(jpeg.pack([d], [empty]), 16) == 1


def test_entropy_is_refused_where_it_means_nothing(tmp_path):
    """--entropy split with --decode host, by every command line that has the flag, before a file is read or a folder made; and the
    classes behind them."""
    from spatialaudiogen_amd import deploy, evaluate, flow, frames, jpeg, overlay, project
    missing, out = str(tmp_path / 'missing'), str(tmp_path / 'out')
    for tool, argv in ((project, [missing, out, '--from', 'er', '--to', 'er', '--size', '24', '48']), (flow, [missing, out]),
                       (overlay, [__file__, missing, out]), (deploy, [missing, missing]), (evaluate, [missing, missing])):
        for extra in (['--entropy', 'split'], ['--decode', 'host', '--entropy', 'split']):
            with pytest.raises(SystemExit) as e:
                tool.main(argv + extra)
            assert '--entropy split belongs to --decode device' in str(e.value.code), (tool.__name__, e.value.code)
        with pytest.raises(SystemExit) as e:
            tool.main(argv + ['--decode', 'device', '--entropy', 'both'])
        assert e.value.code == 2                                      # argparse: not one of the choices
    assert not os.path.exists(out)
    for make in (lambda: frames.FrameReader('cpu', 'host', 'split'), lambda: frames.FrameReader('cpu', 'device', 'both'),
                 lambda: deploy.W2XYZ(decode='host', entropy='split'), lambda: jpeg.JpegDecoder('cpu', entropy='both'),
                 lambda: jpeg.JpegDecoder('cpu', chunk_bytes=512), lambda: jpeg.JpegDecoder('cpu', entropy='split', chunk_bytes=18),
                 lambda: jpeg.JpegDecoder('cpu', entropy='split', rounds=0), lambda: evaluate.evaluate(missing, missing, decode='host', entropy='split')):
        with pytest.raises(ValueError, match='entropy|chunk_bytes|rounds'):
            make()
    assert frames.FrameReader('cpu', 'host').decoder is None and frames.FrameReader('cpu', 'host', 'lane').decoder is None


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from spatialaudiogen_amd import _lib
    print('\n'.join(refusal_lines(_lib.lib())))
