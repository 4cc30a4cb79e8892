"""sagen_jpeg_decode_split (csrc/jpeg_split.hip through jpeg.decode_packed(entropy='split') / jpeg.JpegDecoder(entropy='split')) against
sagen_jpeg_decode on the same packed call: EQUALITY of every output byte and every status word, and against the pixels PIL decoded
where the fixture holds them.  `path` says who decoded a frame; where a case proves the split path itself it must be all 0, so that
nothing hides behind the one-lane redo.  On the device every call is also made on the CPU twin, and `path` must agree.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_jpeg_split.py)."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from test_jpeg_host import fixture, turbo
from test_jpeg_rst_host import fixture as rst_fixture
from util import ensure_lib

pytestmark = pytest.mark.gpu

OP_CASES = ('test_every_fixture_case_alone or test_cases_of_one_geometry_in_one_call or test_forced_unsettled or test_forced_capacity or '
            'test_stuffing_across_a_chunk_boundary or test_corner_inputs or test_dc_scan_across_tiles or test_chunk_scans_across_workgroups or '
            'test_damaged_streams or test_decoder_with_split_entropy or test_project_command_line_with_split_entropy')
UNSETTLED, ANOMALY, CAPACITY = 1, 2, 4
_TWIN = {}


def _dev():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    if _lib.IS_CPU_TWIN:
        return 'cpu'
    import torch
    assert torch.cuda.is_available()
    return 'cuda'


def all_cases():
    """[(name, file bytes, PIL's pixels or None)]: the 30 of jpeg_v1.npz and the 30 files of jpeg_rst_v1.npz"""
    names, data, rgb, _ = fixture()
    rnames, _, rdata = rst_fixture()[:3]
    return [(n, data[n], rgb[n]) for n in names] + [('rst:' + n, rdata[n], None) for n in rnames]


def segment_chunks(info, chunk_bytes):
    """chunks of each restart segment of a parsed file, by hand: max(1, ceil(bytes / chunk_bytes))"""
    starts = [int(s) for s in info.segments]
    ends = [s - 2 for s in starts[1:]] + [info.scan_bytes]
    return [max(1, -(-(e - s) // chunk_bytes)) for s, e in zip(starts, ends)]


def chunk_size_for(infos, chunk_bytes):
    """chunk_bytes, raised until no segment of the call has more than 64 chunks (rounds = 64 then settles whatever the stream)"""
    while max(max(segment_chunks(i, chunk_bytes)) for i in infos) > 64:
        chunk_bytes *= 2
    return chunk_bytes


def twin_split(packed, chunk_bytes, rounds, max_chunks):
    """The same call on the CPU twin through the bare C ABI, on numpy buffers -> (out, status, path)."""
    from spatialaudiogen_amd import build
    if 'l' not in _TWIN:
        l = C.CDLL(build.build_cpu_twin())
        P, I, I64 = C.c_void_p, C.c_int, C.c_int64
        l.sagen_jpeg_decode_split_scratch_bytes.restype = C.c_size_t
        l.sagen_jpeg_decode_split_scratch_bytes.argtypes = [I] * 8 + [I64]
        l.sagen_jpeg_decode_split.argtypes = [P, I64, P, I, P, I, P, I, P, I, I, I, I, I, I, P, P, P, C.c_size_t, P, I, I, I64, P]
        _TWIN['l'] = l
    l, p = _TWIN['l'], packed
    w, h, comps, hs, vs = p.geometry
    out, status, path = np.zeros((p.n, h, w, 3), np.uint8), np.full(p.n, -1, np.int32), np.full(p.n, -1, np.int32)
    need = l.sagen_jpeg_decode_split_scratch_bytes(p.n, w, h, comps, hs, vs, p.n_hufftabs, p.n_segments, max_chunks)
    assert need > 0 and need % 16 == 0
    scratch = np.zeros(need // 8 + 2, np.float64)
    buf = np.zeros(p.buffer.size // 8 + 2, np.float64)
    buf.view(np.uint8)[:p.buffer.size] = p.buffer
    base, sc = buf.ctypes.data, (scratch.ctypes.data + 15) // 16 * 16
    assert l.sagen_jpeg_decode_split(base + p.bytes_at, p.total_bytes, base + p.frames_at, p.n, base + p.segments_at, p.n_segments, base + p.qtabs_at,
                                     p.n_qtabs, base + p.hufftabs_at, p.n_hufftabs, w, h, comps, hs, vs, out.ctypes.data, status.ctypes.data, sc, need,
                                     None, chunk_bytes, rounds, max_chunks, path.ctypes.data) == 0
    return out, status, path


def both(datas, chunk_bytes, rounds, infos=None, max_chunks=None):
    """One packed call through sagen_jpeg_decode and through sagen_jpeg_decode_split: out and status must be equal, and on the device
    out, status and path must be the twin's.  Returns (out, status, path, packed) as numpy."""
    import torch
    from spatialaudiogen_amd import jpeg
    dev = _dev()
    infos = infos if infos is not None else [jpeg.parse(d) for d in datas]
    packed = jpeg.pack(datas, infos)
    staged = torch.as_tensor(packed.buffer).to(dev)
    ref, ref_status = jpeg.decode_packed(packed, staged)
    max_chunks = jpeg.split_chunks(packed, chunk_bytes) if max_chunks is None else max_chunks
    out, status, path = jpeg.decode_packed(packed, staged, entropy='split', chunk_bytes=chunk_bytes, rounds=rounds, want_path=True, max_chunks=max_chunks)
    ref, ref_status, out, status, path = (t.cpu().numpy() for t in (ref, ref_status, out, status, path))
    assert np.array_equal(status, ref_status), (status, ref_status, path)
    # (a frame the descriptor check refused - SAGEN_JPEG_ST_DESC, 16 - is decoded by neither call: both convert whatever their scratch
    # held, so there is nothing to compare)
    seen = (status & 16) == 0
    assert np.array_equal(out[seen], ref[seen]), path
    if dev == 'cuda':
        t_out, t_status, t_path = twin_split(packed, chunk_bytes, rounds, max_chunks)
        assert np.array_equal(path, t_path), (path, t_path)
        assert np.array_equal(status, t_status) and np.array_equal(out[seen], t_out[seen])
    return out, status, path, packed


# ---- 1: every fixture case, the split path itself --------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(60))
def test_every_fixture_case_alone(k):
    from spatialaudiogen_amd import jpeg
    name, data, want = all_cases()[k]
    info = jpeg.parse(data)
    for chunk_bytes in (16, 32, 64):
        cb = chunk_size_for([info], chunk_bytes)
        assert max(segment_chunks(info, cb)) <= 64
        out, status, path, packed = both([data], cb, 64)
        assert jpeg.split_chunks(packed, cb) == sum(segment_chunks(info, cb))
        assert path.tolist() == [0] and status.tolist() == [0], (name, cb, path, status)
        if want is not None:
            assert np.array_equal(out[0], want), (name, cb)


def _geometries():
    from spatialaudiogen_amd import jpeg
    groups = {}
    for name, data, want in all_cases():
        groups.setdefault(tuple(jpeg.parse(data)[:5]), []).append((name, data, want))
    return groups


def test_cases_of_one_geometry_in_one_call():
    from spatialaudiogen_amd import jpeg
    groups = _geometries()
    assert sum(len(v) > 1 for v in groups.values()) >= 6
    for geom, members in sorted(groups.items()):
        infos = [jpeg.parse(d) for _, d, _ in members]
        for chunk_bytes in (16, 32, 64):
            cb = chunk_size_for(infos, chunk_bytes)
            out, status, path, _ = both([d for _, d, _ in members], cb, 64, infos)
            assert not path.any() and not status.any(), (geom, cb, path, status)
            for j, (name, _, want) in enumerate(members):
                if want is not None:
                    assert np.array_equal(out[j], want), (geom, name, cb)


# ---- 2, 3: the redo ------------------------------------------------------------------------------------------------------------------------
def test_forced_unsettled():
    """One round only: the test first shows on the twin that the call needs more, then the frames come out UNSETTLED and still equal."""
    from spatialaudiogen_amd import jpeg
    members = _geometries()[(17, 23, 3, 2, 2)]
    datas = [d for _, d, _ in members]
    packed = jpeg.pack(datas, [jpeg.parse(d) for d in datas])
    t_path = twin_split(packed, 16, 1, jpeg.split_chunks(packed, 16))[2]
    assert t_path.any() and set(t_path.tolist()) <= {0, UNSETTLED}, t_path
    out, status, path, _ = both(datas, 16, 1)
    assert np.array_equal(path, t_path) and not status.any()
    for j, (name, _, want) in enumerate(members):
        if want is not None:
            assert np.array_equal(out[j], want), name
    assert not both(datas, 16, 64)[2].any()                           # the same call with rounds enough


def test_forced_capacity():
    """max_chunks = n_segments, the smallest legal value: the rows are placed in their order, and a frame owning a row that ends behind the
    capacity is decoded by one lane per segment."""
    from spatialaudiogen_amd import jpeg
    members = _geometries()[(17, 23, 3, 2, 2)]
    datas = [d for _, d, _ in members]
    infos = [jpeg.parse(d) for d in datas]
    n_segments = sum(i.segments.size for i in infos)
    want_path, placed = [], 0
    for i in infos:
        hit = 0
        for c in segment_chunks(i, 64):
            placed += c
            hit |= CAPACITY if placed > n_segments else 0
        want_path.append(hit)
    assert 0 in want_path and CAPACITY in want_path
    out, status, path, packed = both(datas, 64, 64, infos, max_chunks=n_segments)
    assert packed.n_segments == n_segments and path.tolist() == want_path and not status.any()
    for j, (name, _, want) in enumerate(members):
        if want is not None:
            assert np.array_equal(out[j], want), name


# ---- 4: inputs that reach the corners ----------------------------------------------------------------------------------------------------
def _save(a, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, 'JPEG', **kw)
    return b.getvalue()


def _noise(h, w, seed, grey=False):
    return np.random.RandomState(seed).randint(0, 256, (h, w) if grey else (h, w, 3)).astype(np.uint8)


def _smooth(h, w, seed, grey=False):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([127 + 100 * np.sin(x / 9. + seed), 127 + 100 * np.cos(y / 7.), (3 * x + 2 * y + 9 * seed) % 256], -1)
    a = np.clip(a + np.random.RandomState(seed).randint(-8, 9, (h, w, 3)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(a[..., 1]) if grey else a


def _pil_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def _exact(datas, chunk_bytes, rounds=64, settles=True):
    out, status, path, _ = both(datas, chunk_bytes, rounds)
    assert not status.any(), status
    if settles:
        assert not path.any(), path
    if turbo():
        for j, d in enumerate(datas):
            assert np.array_equal(out[j], _pil_pixels(d)), j
    return path


def test_stuffing_across_a_chunk_boundary():
    """A scan in which an FF 00 pair straddles a chunk boundary at the chunk size used, for grey and every sampling."""
    from spatialaudiogen_amd import jpeg
    for kw, grey in ((dict(), True), (dict(subsampling=0), False), (dict(subsampling=1), False), (dict(subsampling=2), False)):
        found = None
        for seed in range(200):
            data = _save(_noise(24, 40, seed, grey), quality=95, **kw)
            info = jpeg.parse(data)
            scan = data[info.scan_offset:info.scan_offset + info.scan_bytes]
            cb = chunk_size_for([info], 32)
            if any(scan[i] == 0xFF and scan[i + 1] == 0 for i in range(cb - 1, len(scan) - 1, cb)):
                found = (data, cb)
                break
        assert found is not None, kw
        _exact([found[0]], found[1])


def test_corner_inputs():
    from spatialaudiogen_amd import jpeg
    # a flat frame: more than 64 blocks inside one chunk
    data = _save(np.full((128, 128), 77, np.uint8), quality=75)
    info = jpeg.parse(data)
    assert 16 * 16 > 64 * sum(segment_chunks(info, 128))              # (more blocks than 64 per chunk: some chunk holds more)
    _exact([data], 128)
    # noise at quality 100: a block is longer than two chunks of 16 bytes
    data = _save(_noise(16, 16, 3, True), quality=100)
    info = jpeg.parse(data)
    assert info.scan_bytes > 4 * 48 and max(segment_chunks(info, 16)) <= 64
    _exact([data], 16)
    # tables of the file's own
    data = _save(_smooth(40, 56, 4), quality=85, optimize=True)
    info = jpeg.parse(data)
    assert info.actabs[0][:16 + 162] != jpeg._STD_HUFF[1]
    for cb in (16, 32, 64):
        _exact([data], chunk_size_for([info], cb))
    # segments shorter than one chunk, next to longer ones
    data = _save(_smooth(32, 48, 5), quality=60, subsampling=2, restart_marker_blocks=1)
    info = jpeg.parse(data)
    assert info.segments.size == 6 and min(np.diff(info.segments)) - 2 < 64 and 1 in segment_chunks(info, 64)
    for cb in (16, 64):
        _exact([data], cb)
    # grey, 4:4:4, 4:2:2, 4:2:0 on partial MCUs
    for kw, grey in ((dict(), True), (dict(subsampling=0), False), (dict(subsampling=1), False), (dict(subsampling=2), False)):
        data = _save(_smooth(23, 37, 6, grey), quality=90, **kw)
        _exact([data], chunk_size_for([jpeg.parse(data)], 16))


def test_dc_scan_across_tiles():
    """128 x 256: 512 blocks of one component, two tiles of the DC scan; grey and 4:4:4."""
    from spatialaudiogen_amd import jpeg
    for grey in (True, False):
        data = _save(_smooth(128, 256, 7, grey), quality=75, subsampling=0) if not grey else _save(_smooth(128, 256, 7, True), quality=75)
        info = jpeg.parse(data)
        assert (info.width, info.height) == (256, 128) and 16 * 32 > 256
        _exact([data], chunk_size_for([info], 64))


def test_chunk_scans_across_workgroups():
    """Three frames of 64 x 128 noise at quality 95 in chunks of 16 bytes: more than 256 chunks a frame, scans of different lengths.  64
    rounds need not settle 256 chunks, so path is whatever it is - the same on the device and on the twin - and the output is equal."""
    from spatialaudiogen_amd import jpeg
    datas = [_save(_noise(64, 128, 20 + k) // (k + 1), quality=95, subsampling=2) for k in range(3)]
    infos = [jpeg.parse(d) for d in datas]
    assert all(sum(segment_chunks(i, 16)) > 256 for i in infos) and len({i.scan_bytes for i in infos}) == 3
    path = _exact(datas, 16, 64, settles=False)
    print('path of the three frames at 16 bytes, 64 rounds:', path.tolist())
    cb = chunk_size_for(infos, 16)                                     # ... and settled: each frame four times, more than 256 chunks in the call
    assert 4 * sum(sum(segment_chunks(i, cb)) for i in infos) > 256
    _exact(datas * 4, cb, 64)


# ---- 5: damaged streams --------------------------------------------------------------------------------------------------------------------
def check_damaged(what, datas, infos, flags, expected, out, status, path):
    """status is the one-lane path's (both() has compared); healthy neighbours exact; path non-zero exactly where status is, or where
    the frame was unsettled; a frame the descriptor check refused is decoded by nobody and carries 0."""
    for k in range(len(datas)):
        if flags[k]:
            assert status[k] != 0, what
            assert (path[k] == 0) == bool(status[k] & (16 | 32)), (what, k, status[k], path[k])
        else:
            assert status[k] == 0 and path[k] in (0, UNSETTLED) and np.array_equal(out[k], expected[k]), (what, k, path[k])


def device_mutations():
    """the truncated and the moved-marker families, a handful of calls: every 24th cut, every moved marker of two groups"""
    from test_cpu_twin_jpeg import mutation_cases
    cases = mutation_cases()
    cuts = [c for c in cases if 'cut at' in c[0]][::24]
    moved = [c for c in cases if 'moved' in c[0]][::3]
    assert 5 <= len(cuts) <= 12 and 4 <= len(moved) <= 8
    return cuts + moved


def test_damaged_streams():
    for what, datas, infos, flags, expected in device_mutations():
        for chunk_bytes, rounds in ((16, 8), (64, 1)):
            out, status, path, _ = both(datas, chunk_bytes, rounds, infos)
            check_damaged(what, datas, infos, flags, expected, out, status, path)


# ---- 6: device against twin ------------------------------------------------------------------------------------------------------------------
def test_device_path_equals_twin_path():
    """(both() compares path, status and out with the twin's in every test of this file when it runs on the device; here: that it did)"""
    import torch
    assert _dev() == 'cuda' and torch.cuda.is_available()
    members = _geometries()[(17, 23, 3, 2, 2)]
    datas = [d for _, d, _ in members]
    seen = set()
    for rounds in (1, 2, 64):
        seen |= set(both(datas, 16, rounds)[2].tolist())
    assert seen == {0, UNSETTLED}


# ---- 7: through the surface ------------------------------------------------------------------------------------------------------------------
def test_decoder_with_split_entropy(tmp_path):
    import torch
    from spatialaudiogen_amd import jpeg
    names, data, rgb, _ = fixture()
    order = ['420_17x23_q75', '444_17x23_q75', '420_17x23_q30_rows', 'grey_17x23_q30_opt', '422_17x23_q75', '420_17x23_q1', '444_17x23_q75']
    items = [data[n] for n in order]
    path = str(tmp_path / 'frame.jpg')
    with open(path, 'wb') as f:
        f.write(items[2])
    items[2] = path
    lane, split = jpeg.JpegDecoder(_dev()), jpeg.JpegDecoder(_dev(), entropy='split')
    assert (split.chunk_bytes, split.rounds) == (jpeg.SPLIT_CHUNK_BYTES, jpeg.SPLIT_ROUNDS) and lane.last_paths == {}
    want = lane.decode(items)
    got = split.decode(items)
    assert torch.equal(got, want) and split.last_paths == {0: 7} and lane.last_paths == {}
    for j, n in enumerate(order):
        assert np.array_equal(got[j].cpu().numpy(), rgb[n]), n
    small = jpeg.JpegDecoder(_dev(), entropy='split', chunk_bytes=16, rounds=1)
    assert torch.equal(small.decode(items), want) and sum(small.last_paths.values()) == 7 and set(small.last_paths) <= {0, UNSETTLED}
    with pytest.raises(IOError, match='damaged'):
        split.decode([data['420_17x23_q75'][:-40] + b'\xff\xd9'])
    for kw in (dict(entropy='both'), dict(chunk_bytes=512), dict(entropy='split', chunk_bytes=18), dict(entropy='split', rounds=65)):
        with pytest.raises(ValueError):
            jpeg.JpegDecoder(_dev(), **kw)


def _folder(path, n, h, w, seed):
    from PIL import Image
    os.makedirs(path)
    for k in range(n):
        Image.fromarray(_smooth(h, w, seed + k)).save(os.path.join(path, '%06d.jpg' % k), quality=95)


def test_project_command_line_with_split_entropy(tmp_path):
    _dev()
    from spatialaudiogen_amd import project
    src = str(tmp_path / 'in')
    _folder(src, 6, 32, 64, 1)
    for entropy in ('lane', 'split'):
        project.main([src, str(tmp_path / entropy), '--from', 'er', '--to', 'er', '--size', '24', '48', '--decode', 'device', '--entropy', entropy,
                      '--block', '4'])
    a, b = str(tmp_path / 'lane'), str(tmp_path / 'split')
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == 6
    for f in os.listdir(a):
        assert open(os.path.join(a, f), 'rb').read() == open(os.path.join(b, f), 'rb').read(), f
