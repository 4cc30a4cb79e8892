"""The host side of the device JPEG decode, without a GPU: the numpy restatement (tests/jpeg_oracle.py) against the fixture's pixels
(tests/golden/jpeg_v1.npz, decoded by PIL on libjpeg-turbo when the fixture was made) and against live PIL, the marker walk
jpeg.parse, and the packing of descriptors and tables for include/sagen.h: sagen_jpeg_decode."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import jpeg_oracle as JO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIXTURE = {}


def fixture():
    """(names, {name: bytes}, {name: rgb}, [(reject name, bytes, word)]) - loaded once, never changed."""
    if not _FIXTURE:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_v1.npz'))
        names = [str(n) for n in z['names']]
        _FIXTURE['v'] = (names, {n: z['bytes_%d' % k].tobytes() for k, n in enumerate(names)}, {n: z['rgb_%d' % k] for k, n in enumerate(names)},
                         [(str(n), z['reject_%d' % k].tobytes(), str(z['reject_reasons'][k])) for k, n in enumerate(z['reject_names'])])
    return _FIXTURE['v']


def turbo():
    from PIL import features
    return bool(features.check_feature('libjpeg_turbo'))


def test_the_fixture_covers_what_the_issue_lists():
    names, data, rgb, rejects = fixture()
    assert 25 <= len(names) <= 40 and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg_v1.npz')) < 300 * 1024
    for word in ('444_', '422_', '420_', 'grey_', '_17x23_', '_9x31_', '_33x18_', '_q1', '_q30', '_q75', '_q100', '_opt', '_rows', '_blocks',
                 'saturated', '48x64', '8x8'):
        assert any(word in n for n in names), word
    assert {r[0] for r in rejects} >= {'progressive', 'cmyk', '411', '440'}
    assert max(v.size for v in rgb.values()) <= 48 * 64 * 3


@pytest.mark.parametrize('k', range(30))
def test_restatement_equals_the_fixture(k):
    names, data, rgb, _ = fixture()
    assert len(names) == 30
    assert np.array_equal(JO.decode(data[names[k]]), rgb[names[k]]), names[k]


def test_restatement_equals_live_pil():
    if not turbo():
        pytest.skip('this PIL is not linked against libjpeg-turbo: another decoder need not agree to the byte')
    from PIL import Image
    rs = np.random.RandomState(5)
    for w, h, sub, q, opt, kw in ((17, 23, 2, 20, False, {}), (33, 18, 1, 90, True, {}), (9, 31, 0, 5, False, {}), (24, 40, 2, 95, True, dict(restart_marker_blocks=3)),
                                  (16, 16, 2, 75, False, dict(restart_marker_rows=1)), (8, 9, 2, 50, False, {})):
        y, x = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([x * 7, y * 9, 128 + 100 * np.sin(x / 3.)], -1) + rs.randint(-30, 30, (h, w, 3)), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(a).save(b, 'JPEG', quality=q, subsampling=sub, optimize=opt, **kw)
        ref = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert('RGB'))
        assert np.array_equal(JO.decode(b.getvalue()), ref), (w, h, sub, q)


# ---- parse ---------------------------------------------------------------------------------------------------------------------------
def test_parse_fields_of_known_streams():
    from spatialaudiogen_amd import jpeg
    names, data, rgb, _ = fixture()
    want = {'444_8x8_q75': (8, 8, 3, 1, 1), '422_16x8_q75': (16, 8, 3, 2, 1), '420_16x16_q75': (16, 16, 3, 2, 2), 'grey_17x23_q30_opt': (17, 23, 1, 1, 1),
            '420_48x64_q75_blocks': (48, 64, 3, 2, 2)}
    for n in names:
        i = jpeg.parse(data[n])
        assert (i.height, i.width) == rgb[n].shape[:2]
        if n in want:
            assert tuple(i[:5]) == want[n]
        d = data[n]
        assert d[i.scan_offset + i.scan_bytes:i.scan_offset + i.scan_bytes + 2] == b'\xff\xd9'
        assert len(i.qtabs) == len(i.dctabs) == len(i.actabs) == i.components
        assert all(q.dtype == np.uint16 and q.shape == (64,) and q.min() >= 1 for q in i.qtabs)
        assert all(len(t) == jpeg.HUFF_SPEC and sum(t[:16]) <= 256 for t in i.dctabs + i.actabs)
    # the standard tables (optimize off) are shared between streams, the optimised ones are the file's own
    a, b, c = jpeg.parse(data['420_17x23_q75']), jpeg.parse(data['444_17x23_q75']), jpeg.parse(data['420_17x23_q100_opt'])
    assert a.dctabs == b.dctabs and a.actabs == b.actabs and c.actabs != a.actabs
    assert a.dctabs[0][:16] == bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0])          # Annex K, luminance DC
    q1, q100 = jpeg.parse(data['420_17x23_q1']), jpeg.parse(data['422_9x31_q100'])
    assert q1.qtabs[0].max() == 255 and q100.qtabs[0].max() == 1


def test_parse_restart_offsets():
    from spatialaudiogen_amd import jpeg
    names, data, _, _ = fixture()
    seen = 0
    for n in names:
        i, d = jpeg.parse(data[n]), data[n]
        assert i.segments[0] == 0 and i.segments.dtype == np.int32
        mcus = -(-i.width // (8 * i.hs)) * -(-i.height // (8 * i.vs))
        assert i.segments.size == (-(-mcus // i.restart_interval) if i.restart_interval else 1)
        # found the slow way: every FF Dn inside the scan
        scan = d[i.scan_offset:i.scan_offset + i.scan_bytes]
        slow = [0] + [m.start() + 2 for m in re.finditer(b'\xff[\xd0-\xd7]', scan)]
        assert list(i.segments) == slow
        for k in range(1, i.segments.size):
            assert scan[i.segments[k] - 2:i.segments[k]] == bytes([0xFF, 0xD0 + (k - 1) % 8])
        seen += i.segments.size > 1
    assert seen >= 6
    assert jpeg.parse(data['420_48x64_q75_blocks']).restart_interval == 3 and jpeg.parse(data['420_48x64_q75_blocks']).segments.size == 4
    assert jpeg.parse(data['444_24x40_q75_rows']).restart_interval == 3 and jpeg.parse(data['444_24x40_q75_rows']).segments.size == 5


def test_parse_rejects_with_reasons_and_garbage_with_value_error():
    from spatialaudiogen_amd import jpeg
    names, data, _, rejects = fixture()
    for name, d, word in rejects:
        with pytest.raises(jpeg.JpegUnsupported) as e:
            jpeg.parse(d)
        assert word in e.value.reason, (name, e.value.reason)
    good = data['420_17x23_q75']
    # component ids R, G, B and an Adobe marker with transform 0, by editing headers
    sof = good.find(b'\xff\xc0')
    rgb_ids = bytearray(good)
    sos = good.find(b'\xff\xda')
    for k, c in enumerate(b'RGB'):
        rgb_ids[sof + 10 + 3 * k] = c
        rgb_ids[sos + 5 + 2 * k] = c
    with pytest.raises(jpeg.JpegUnsupported, match='R, G, B'):
        jpeg.parse(bytes(rgb_ids))
    adobe = good[:2] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00' + good[2:]
    with pytest.raises(jpeg.JpegUnsupported, match='transform 0'):
        jpeg.parse(adobe)
    assert jpeg.parse(good[:2] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01' + good[2:]).width == 17
    sixteen = bytearray(good)
    sixteen[good.find(b'\xff\xdb') + 4] |= 0x10
    with pytest.raises(jpeg.JpegUnsupported, match='16-bit'):
        jpeg.parse(bytes(sixteen))
    for junk in (b'', b'\xff', b'PNG\r\n', bytes(100), b'\xff\xd8', b'\xff\xd8\xff\xd9', good[:40], good[:-2], good[:sos + 20], b'\x00' + good):
        with pytest.raises(ValueError):
            jpeg.parse(junk)
    moved = bytearray(data['420_48x64_q75_blocks'])                        # one restart marker fewer than the interval asks for
    at = bytes(moved).find(b'\xff\xd1')
    moved[at:at + 2] = b'\x12\x34'
    with pytest.raises(ValueError, match='restart'):
        jpeg.parse(bytes(moved))


# ---- packing -------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_as_the_header_documents():
    from spatialaudiogen_amd import _lib, jpeg
    header = open(os.path.join(ROOT, 'include', 'sagen.h')).read()
    assert '} sagen_jpeg_frame;             /* 64 bytes */' in header and '[n] sagen_jpeg_frame DEVICE (64 bytes each)' in header
    assert C.sizeof(_lib.SagenJpegFrame) == 64 == jpeg.FRAME_DTYPE.itemsize
    for name, _ in _lib.SagenJpegFrame._fields_:
        assert getattr(_lib.SagenJpegFrame, name).offset == jpeg.FRAME_DTYPE.fields[name][1], name
    assert '[n_hufftabs][272] uint8' in header and jpeg.HUFF_SPEC == 272
    for bit, name in _lib.SAGEN_JPEG_STATUS.items():
        assert re.search(r'SAGEN_JPEG_ST_[A-Z]+ = %d\b' % bit, header), name


def test_pack_deduplicates_tables_and_pads():
    from spatialaudiogen_amd import jpeg
    names, data, _, _ = fixture()
    group = ['420_17x23_q75', '420_17x23_q1', '420_17x23_q100_opt', '420_17x23_q30_rows', '420_17x23_q75']
    datas = [data[n] for n in group]
    infos = [jpeg.parse(d) for d in datas]
    p = jpeg.pack(datas, infos)
    assert p.geometry == (17, 23, 3, 2, 2) and p.n == 5 and p.n_segments == 1 + 1 + 1 + 2 + 1
    # three streams carry the standard Huffman tables (4 of them), the optimised one its own 4; quality 75 (twice) and 30 have a luma
    # and a chroma table each, at quality 1 both are all 255 and at 100 both all 1
    assert p.n_hufftabs == 8 and p.n_qtabs == 2 + 1 + 1 + 2
    for off in (p.frames_at, p.segments_at, p.qtabs_at, p.hufftabs_at, p.bytes_at):
        assert off % 16 == 0
    assert p.total_bytes % 4 == 0 and 0 <= p.total_bytes - sum(len(d) for d in datas) < 4 and p.buffer.size == p.bytes_at + p.total_bytes
    frames = np.frombuffer(p.buffer, jpeg.FRAME_DTYPE, 5, p.frames_at)
    segs = np.frombuffer(p.buffer, np.int32, 2 * p.n_segments, p.segments_at).reshape(-1, 2)
    qt = np.frombuffer(p.buffer, np.uint16, 64 * p.n_qtabs, p.qtabs_at).reshape(-1, 64)
    ht = np.frombuffer(p.buffer, np.uint8, 272 * p.n_hufftabs, p.hufftabs_at).reshape(-1, 272)
    start = 0
    for f, (d, i) in enumerate(zip(datas, infos)):
        fr = frames[f]
        assert fr['scan_offset'] == start + i.scan_offset and fr['scan_bytes'] == i.scan_bytes and fr['restart_interval'] == i.restart_interval
        assert bytes(p.buffer[p.bytes_at + start:p.bytes_at + start + len(d)]) == d
        rows = segs[fr['first_segment']:fr['first_segment'] + fr['n_segments']]
        assert (rows[:, 0] == f).all() and list(rows[:, 1]) == list(i.segments)
        for c in range(3):
            assert np.array_equal(qt[fr['qtab'][c]], i.qtabs[c]) and bytes(ht[fr['dctab'][c]]) == i.dctabs[c] and bytes(ht[fr['actab'][c]]) == i.actabs[c]
        start += len(d)
    assert list(frames[0]['qtab']) == list(frames[4]['qtab']) and list(frames[0]['actab']) == list(frames[4]['actab'])
    assert frames[0]['reserved'] == 0
    with pytest.raises(ValueError):
        jpeg.pack([data['420_17x23_q75'], data['444_17x23_q75']], [infos[0], jpeg.parse(data['444_17x23_q75'])])
