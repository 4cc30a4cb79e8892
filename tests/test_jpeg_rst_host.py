"""JPEG restart intervals, the host side (no GPU): tests/golden/jpeg_rst_v1.npz (tools/make_jpeg_rst_fixture.py: images and the complete
files PIL wrote for them on libjpeg-turbo with restart_marker_blocks=R) against the numpy restatement tests/jpeg_rst_oracle.py; the
header and interval pieces of spatialaudiogen_amd/jpeg.py against live PIL; what sagen_jpeg_encode_rst and sagen_jpeg_transcode refuse, with which code and
message, pinned for BOTH libraries by tests/golden/op_refusals_jpeg_rst_v1.txt (the entry points are csrc/op_entries_jpeg_rst.h, written
once).  Every comparison is equality of bytes.

    python tests/test_jpeg_rst_host.py        prints the refusal lines of the device library of the tree the file lies in"""
import ctypes as C
import io
import os
import re
import sys

import numpy as np
import pytest

import jpeg_enc_oracle as JE
import jpeg_rst_oracle as JR
from test_jpeg_enc_host import FACTORS, PIL_SUB, SUBSAMPLING, turbo
from test_op_refusals_host import P, OFF2, OFF1, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'op_refusals_jpeg_rst_v1.txt')
N_CASES = 30
_FIXTURE = {}


def fixture():
    """(names, {name: image}, {name: file bytes}, {name: quality}, {name: '444' | '422' | '420' | 'grey'}, {name: interval in MCUs}) -
    loaded once, never changed."""
    if not _FIXTURE:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_rst_v1.npz'))
        names = [str(n) for n in z['names']]
        _FIXTURE['v'] = (names, {n: z['image_%d' % k] for k, n in enumerate(names)}, {n: z['file_%d' % k].tobytes() for k, n in enumerate(names)},
                         {n: int(z['quality'][k]) for k, n in enumerate(names)}, {n: str(z['sampling'][k]) for k, n in enumerate(names)},
                         {n: int(z['interval'][k]) for k, n in enumerate(names)})
    return _FIXTURE['v']


def scan_of(data):
    """the entropy-coded bytes, restart markers included: between the SOS header and FF D9"""
    at = data.index(b'\xff\xda')
    assert data[-2:] == b'\xff\xd9'
    return data[at + 2 + ((data[at + 2] << 8) | data[at + 3]):-2]


def mcus_of(img, sampling):
    fh, fv = FACTORS[sampling]
    return -(-img.shape[1] // (8 * fh)), -(-img.shape[0] // (8 * fv))


def pil_file(img, quality, sampling, **restart):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', quality=quality, **dict({} if img.ndim == 2 else dict(subsampling=PIL_SUB[sampling]), **restart))
    return b.getvalue()


def markers_of(scan):
    """the restart markers of a scan in their order (a stuffed FF is followed by 00, never by D0..D7)"""
    return [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]


def test_the_fixture_covers_what_the_issue_lists():
    names, image, data, quality, sampling, interval = fixture()
    assert len(names) == N_CASES and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg_rst_v1.npz')) < 300 * 1024
    assert all(v.size <= 48 * 64 * 3 or v.shape[:2] == (72, 40) for v in image.values()) and any(v.shape[:2] == (72, 40) for v in image.values())
    for word in ('_1x1_', '_8x8_', '_16x16_', '_17x23_', '_9x33_', '_33x18_', '_40x35_', '_24x40_', '_48x64_', '_40x72_', '444_', '422_', '420_', 'grey_',
                 '_q1_', '_q75_', '_q95_', '_q100_', 'noise', 'smooth', 'saturated', '_r1', '_r2', '_rrow', '_rover'):
        assert any(word in n for n in names), word
    segments = {n: JR.segment_bits(image[n], JE.tables(quality[n]), *FACTORS[sampling[n]], interval[n]) for n in names}
    for n in names:
        mx, my = mcus_of(image[n], sampling[n])
        assert len(segments[n]) == (-(-mx * my // interval[n]) if interval[n] < mx * my else 1), n
        assert markers_of(scan_of(data[n])) == [0xD0 + (k & 7) for k in range(len(segments[n]) - 1)], n
        at = data[n].index(b'\xff\xda')                                 # DRI directly in front of SOS
        assert data[n][at - 6:at] == b'\xff\xdd\x00\x04' + interval[n].to_bytes(2, 'big'), n
        if n.endswith('_rrow'):
            assert interval[n] == mx and len(segments[n]) == my
    assert any(interval[n] > 1 and len(segments[n]) == 1 for n in names)            # DRI, no marker
    assert any(len(segments[n]) >= 10 for n in names)                               # ... FF D7, then FF D0 again
    assert any(len(segments[n]) > 1 and len(segments[n]) * interval[n] > np.prod(mcus_of(image[n], sampling[n])) for n in names)   # a short last segment
    # a segment that ends exactly on a byte: no fill; and one whose fill completes a byte of ones, which is stuffed in front of the marker
    n = '444_16x16_q100_nofill_r1'
    assert any(len(s) % 8 == 0 for s in segments[n][:-1])
    # ... and from the file's bytes: the bytes of the scan between two markers, unstuffed, are the segment's bits with ones behind
    # them; where the segment ends on a byte, the byte in front of the marker is its last 8 bits, where not, bits + fill
    for n in ('444_16x16_q100_nofill_r1', '444_16x16_q100_ffill_r1'):
        scan, parts, start = scan_of(data[n]), [], 0
        for i in range(len(scan) - 1):
            if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
                parts.append(scan[start:i])
                start = i + 2
        parts.append(scan[start:])
        assert len(parts) == len(segments[n])
        for part, bits in zip(parts, segments[n]):
            raw = part.replace(b'\xff\x00', b'\xff')
            assert ''.join(format(v, '08b') for v in raw) == bits + '1' * (-len(bits) % 8), n
            if len(bits) % 8 == 0:
                assert format(raw[-1], '08b') == bits[-8:] and len(raw) * 8 == len(bits)
    n = '444_16x16_q100_ffill_r1'
    hits = [k for k, s in enumerate(segments[n][:-1]) if len(s) % 8 and set(s[len(s) // 8 * 8:]) == {'1'}]
    assert hits and all(b'\xff\x00\xff' + bytes([0xD0 + (k & 7)]) in scan_of(data[n]) for k in hits)
    # dummies inside segments: luma blocks of an MCU wholly outside the image
    assert any(n.startswith('420_9x33_') for n in names) and any(n.startswith('420_33x18_') for n in names)
    groups = {}
    for n in names:
        groups.setdefault((sampling[n], image[n].shape, quality[n], interval[n]), []).append(n)
    assert sum(len(v) > 1 for v in groups.values()) >= 2


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_equals_the_fixture(k):
    names, image, data, quality, sampling, interval = fixture()
    n = names[k]
    assert JR.encode(image[n], quality[n], SUBSAMPLING[sampling[n]], interval[n]) == data[n], n


def test_restatement_without_an_interval_is_the_plain_one():
    names, image, data, quality, sampling, interval = fixture()
    for n in names[:12]:
        assert JR.encode(image[n], quality[n], SUBSAMPLING[sampling[n]], 0) == JE.encode(image[n], quality[n], SUBSAMPLING[sampling[n]]), n


def test_restatement_equals_live_pil():
    if not turbo():
        pytest.skip('this PIL is not linked against libjpeg-turbo: another encoder need not agree to the byte')
    rs = np.random.RandomState(17)
    for w, h, sampling, q, R in ((19, 21, '420', 20, 1), (33, 18, '422', 90, 2), (9, 31, '444', 5, 3), (26, 40, '420', 97, 2), (16, 14, 'grey', 60, 1),
                                 (7, 9, '420', 50, 5), (64, 40, '420', 95, 4)):
        y, x = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([x * 7, y * 9, 128 + 100 * np.sin(x / 3.)], -1) + rs.randint(-40, 40, (h, w, 3)), 0, 255).astype(np.uint8)
        a = np.ascontiguousarray(a[..., 0]) if sampling == 'grey' else a
        assert JR.encode(a, q, SUBSAMPLING[sampling], R) == pil_file(a, q, sampling, restart_marker_blocks=R), (w, h, sampling, q, R)


def test_header_and_interval_follow_live_pil():
    """DRI directly in front of SOS; rows win over blocks and mean rows x MCUs per row; an interval DRI cannot name is refused."""
    from spatialaudiogen_amd import jpeg
    rs = np.random.RandomState(18)
    t = jpeg.quality_tables(75)
    for sampling in ('444', '422', '420', 'grey'):
        img = rs.randint(0, 256, (23, 41) if sampling == 'grey' else (23, 41, 3)).astype(np.uint8)
        hs, vs = FACTORS[sampling]
        comps = 1 if sampling == 'grey' else 3
        mx = mcus_of(img, sampling)[0]
        for rows, blocks, interval in ((0, 1, 1), (0, 300, 300), (1, 0, mx), (2, 1, 2 * mx), (0, 0, 0)):
            assert jpeg.restart_interval_of(41, 23, comps, hs, vs, rows, blocks) == interval
            want = pil_file(img, 75, sampling, restart_marker_rows=rows, restart_marker_blocks=blocks)
            head = jpeg.encode_header(41, 23, comps, hs, vs, t, interval)
            assert want[:len(head)] == head and len(head) == len(want) - len(scan_of(want)) - 2, (sampling, rows, blocks)
            assert jpeg.parse(want).restart_interval == interval
        assert jpeg.encode_header(41, 23, comps, hs, vs, t, 0) == jpeg.encode_header(41, 23, comps, hs, vs, t)
    assert jpeg.restart_interval_of(16384, 16, 1, 1, 1, 31, 0) == 31 * 2048
    for kw in (dict(restart_rows=32), dict(restart_blocks=65536)):
        with pytest.raises(ValueError, match='65535'):
            jpeg.restart_interval_of(16384, 16, 1, 1, 1, **kw)
    with pytest.raises(ValueError):
        jpeg.restart_interval_of(16, 16, 1, 1, 1, -1, 0)
    for bad in (-1, 65536):
        with pytest.raises(ValueError, match='65535'):
            jpeg.encode_header(8, 8, 3, 1, 1, t, bad)


def test_parse_of_a_fixture_file_returns_its_segments():
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling, interval = fixture()
    for n in names:
        i = jpeg.parse(data[n])
        mx, my = mcus_of(image[n], sampling[n])
        assert i.restart_interval == interval[n] and i.segments.size == -(-mx * my // interval[n]), n
        assert data[n][i.scan_offset:i.scan_offset + i.scan_bytes] == scan_of(data[n])


# ---- what the entry points refuse -----------------------------------------------------------------------------------------------------
OFF8 = P + 8
NAMES = ('frames', 'n', 'w', 'h', 'components', 'hs', 'vs', 'restart_interval', 'qtabs', 'out', 'stride', 'sizes', 'status', 'scratch', 'scratch_bytes',
         'stream')
VALID = dict(frames=P, n=2, w=17, h=23, components=3, hs=2, vs=2, restart_interval=1, qtabs=P, out=P, stride=4096, sizes=P, status=P, scratch=P,
             scratch_bytes=1 << 20, stream=None)                                        # would launch: never made
UNSUPPORTED = ('components_2', 'components_4', 'sampling_1x2', 'grey_2x2', 'w_16385', 'h_16385', 'n_65536', 'stride_above_2_28', 'interval_-1',
               'interval_65536')
ROWS = [
    ('empty', dict(n=0, frames=None, qtabs=None, out=None, sizes=None, status=None, scratch=None, w=0, restart_interval=-5)),
    ('n_-1', dict(n=-1)), ('w_0', dict(w=0)), ('h_0', dict(h=0)), ('stride_0', dict(stride=0)), ('stride_-4', dict(stride=-4)),
    ('stride_4094', dict(stride=4094)),
    ('components_2', dict(components=2)), ('components_4', dict(components=4)), ('sampling_1x2', dict(hs=1, vs=2)),
    ('grey_2x2', dict(components=1)), ('w_16385', dict(w=16385)), ('h_16385', dict(h=16385)), ('n_65536', dict(n=65536)),
    ('stride_above_2_28', dict(stride=(1 << 28) + 4)), ('interval_-1', dict(restart_interval=-1)), ('interval_65536', dict(restart_interval=65536)),
    ('null_frames', dict(frames=None)), ('null_qtabs', dict(qtabs=None)), ('null_out', dict(out=None)), ('null_sizes', dict(sizes=None)),
    ('null_status', dict(status=None)), ('null_scratch', dict(scratch=None)),
    ('out_off_2', dict(out=OFF2)), ('sizes_off_2', dict(sizes=OFF2)), ('status_off_1', dict(status=OFF1)), ('qtabs_off_1', dict(qtabs=OFF1)),
    ('scratch_off_8', dict(scratch=OFF8)),
    ('scratch_too_small', dict(scratch_bytes=1000)), ('scratch_0', dict(scratch_bytes=0)),
    ('scratch_of_the_plain_call', dict(scratch_bytes='plain')),
]
QUERIES = [('sagen_jpeg_encode_rst_scratch_bytes', a) for a in ((2, 17, 23, 3, 2, 2, 0, 4096), (2, 17, 23, 3, 2, 2, 1, 4096), (2, 17, 23, 3, 2, 2, 4, 4096),
                                                                (2, 17, 23, 3, 2, 2, 65535, 4096), (2, 17, 23, 3, 2, 2, 65536, 4096),
                                                                (2, 17, 23, 3, 2, 2, -1, 4096), (0, 17, 23, 3, 2, 2, 1, 4096), (2, 17, 23, 3, 1, 2, 1, 4096),
                                                                (2, 17, 23, 3, 2, 2, 1, 4095))]
QUERIES += [('sagen_jpeg_encode_rst_max_bytes', a) for a in ((17, 23, 3, 2, 2, 0), (17, 23, 3, 2, 2, 1), (17, 23, 3, 2, 2, 2), (17, 23, 3, 2, 2, 3),
                                                            (17, 23, 3, 2, 2, 4), (17, 23, 1, 1, 1, 1), (17, 23, 3, 2, 2, 65536), (17, 23, 3, 2, 2, -1),
                                                            (17, 23, 3, 1, 2, 1))]


T_NAMES = ('bytes', 'total_bytes', 'frames', 'n', 'segments', 'n_segments', 'hufftabs', 'n_hufftabs', 'w', 'h', 'components', 'hs', 'vs',
           'restart_interval', 'out', 'stride', 'sizes', 'status', 'scratch', 'scratch_bytes', 'stream')
T_VALID = dict(bytes=P, total_bytes=4096, frames=P, n=2, segments=P, n_segments=2, hufftabs=P, n_hufftabs=4, w=17, h=23, components=3, hs=2, vs=2,
               restart_interval=1, out=P, stride=4096, sizes=P, status=P, scratch=P, scratch_bytes=1 << 20, stream=None)     # would run: never made
T_UNSUPPORTED = ('components_2', 'w_16385', 'n_65536', 'stride_above_2_28', 'interval_65536', 'total_bytes_2_31', 'n_hufftabs_65537')
T_ROWS = [
    ('empty', dict(n=0, bytes=None, frames=None, segments=None, hufftabs=None, out=None, sizes=None, status=None, scratch=None, w=0)),
    ('n_-1', dict(n=-1)), ('h_0', dict(h=0)), ('stride_4094', dict(stride=4094)), ('total_bytes_-4', dict(total_bytes=-4)),
    ('total_bytes_4094', dict(total_bytes=4094)), ('n_segments_1', dict(n_segments=1)), ('n_hufftabs_0', dict(n_hufftabs=0)),
    ('components_2', dict(components=2)), ('w_16385', dict(w=16385)), ('n_65536', dict(n=65536, n_segments=65536)),
    ('stride_above_2_28', dict(stride=(1 << 28) + 4)), ('interval_65536', dict(restart_interval=65536)), ('total_bytes_2_31', dict(total_bytes=1 << 31)),
    ('n_hufftabs_65537', dict(n_hufftabs=65537)),
    ('null_bytes', dict(bytes=None)), ('null_frames', dict(frames=None)), ('null_segments', dict(segments=None)), ('null_hufftabs', dict(hufftabs=None)),
    ('null_out', dict(out=None)), ('null_sizes', dict(sizes=None)), ('null_status', dict(status=None)), ('null_scratch', dict(scratch=None)),
    ('bytes_off_2', dict(bytes=OFF2)), ('frames_off_4', dict(frames=P + 4)), ('segments_off_2', dict(segments=OFF2)), ('out_off_2', dict(out=OFF2)),
    ('sizes_off_2', dict(sizes=OFF2)), ('status_off_1', dict(status=OFF1)), ('scratch_off_8', dict(scratch=OFF8)),
    ('scratch_too_small', dict(scratch_bytes=1000)), ('scratch_0', dict(scratch_bytes=0)),
]
QUERIES += [('sagen_jpeg_transcode_scratch_bytes', a) for a in ((2, 17, 23, 3, 2, 2, 4, 0, 4096), (2, 17, 23, 3, 2, 2, 4, 1, 4096), (2, 17, 23, 3, 2, 2, 0, 1, 4096),
                                                                (2, 17, 23, 3, 2, 2, 4, 65536, 4096), (0, 17, 23, 3, 2, 2, 4, 1, 4096), (2, 17, 23, 3, 2, 2, 4, 1, 4095))]
QUERIES += [('sagen_jpeg_transcode_max_bytes', a) for a in ((17, 23, 3, 2, 2, 0), (17, 23, 3, 2, 2, 1), (17, 23, 1, 1, 1, 3), (17, 23, 3, 2, 2, 65536),
                                                            (17, 23, 3, 1, 2, 1))]


def refusal_lines(lib):
    """'<function> <case> <rc> <message>' per row, '<query> <arguments> <value>' per size query: what the golden file holds."""
    lines = []
    plain = int(lib.sagen_jpeg_encode_scratch_bytes(2, 17, 23, 3, 2, 2, 4096))
    for case, over in ROWS:
        args = dict(VALID, **over)
        if args['scratch_bytes'] == 'plain':                           # what sagen_jpeg_encode asks for is too little once there are segments
            args['scratch_bytes'] = plain
        rc = lib.sagen_jpeg_encode_rst(*[args[k] for k in NAMES])
        assert (rc == 0) == (case == 'empty'), (case, rc, lib.sagen_last_error())
        lines.append(('sagen_jpeg_encode_rst %s %d %s' % (case, rc, lib.sagen_last_error().decode() if rc else '')).rstrip())
    for case, over in T_ROWS:
        args = dict(T_VALID, **over)
        rc = lib.sagen_jpeg_transcode(*[args[k] for k in T_NAMES])
        assert (rc == 0) == (case == 'empty'), (case, rc, lib.sagen_last_error())
        lines.append(('sagen_jpeg_transcode %s %d %s' % (case, rc, lib.sagen_last_error().decode() if rc else '')).rstrip())
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
    text = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'op_entries_jpeg_rst.h')).read()
    formats = re.findall(r'\bfail\([A-Za-z_]+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text)
    assert len(formats) == 2
    messages = []
    for f, fn in zip(formats, ('sagen_jpeg_encode_rst ', 'sagen_jpeg_transcode ')):
        mine = [l.split(' ', 3)[3] for l in golden() if l.startswith(fn) and len(l.split(' ', 3)) == 4]
        fmt = ''.join(re.findall(r'"((?:[^"\\]|\\.)*)"', f))
        pattern = '.*'.join(re.escape(part) for part in re.split(r'%(?:ld|zu|d|g|s)', fmt))
        assert all(re.fullmatch(pattern, m) for m in mine) and mine
        messages += mine
    core = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'jpeg_enc_core.h')).read()
    reasons = re.findall(r'\*why = "([^"]+)"', core)
    assert len(reasons) == 14                                          # six of the encoder, eight of the transcode
    for reason in reasons:
        assert any(reason in m for m in messages), 'no row of the table gives the reason: ' + reason


def test_the_codes_and_sizes_are_the_documented_ones():
    lines = golden()
    code = {l.split(' ')[1]: int(l.split(' ')[2]) for l in lines if l.startswith('sagen_jpeg_encode_rst ')}
    assert len(code) == len(ROWS) and code['empty'] == 0
    assert {code[k] for k in UNSUPPORTED} == {-3}
    assert {code[k] for k in code if k.startswith('null_')} == {-1}
    assert {code[k] for k in code if k.startswith('scratch_') and not k.startswith('scratch_off')} == {-5}
    assert {code[k] for k in code if not k.startswith(('null_', 'scratch_too', 'scratch_0', 'scratch_of')) and k != 'empty' and k not in UNSUPPORTED} == {-2}
    tcode = {l.split(' ')[1]: int(l.split(' ')[2]) for l in lines if l.startswith('sagen_jpeg_transcode ')}
    assert len(tcode) == len(T_ROWS) and tcode['empty'] == 0
    assert {tcode[k] for k in T_UNSUPPORTED} == {-3}
    assert {tcode[k] for k in tcode if k.startswith('null_')} == {-1}
    assert {tcode[k] for k in ('scratch_too_small', 'scratch_0')} == {-5}
    assert {tcode[k] for k in tcode if not k.startswith(('null_', 'scratch_too', 'scratch_0')) and k != 'empty' and k not in T_UNSUPPORTED} == {-2}
    value = {tuple(l.split(' ')[:2]): int(l.split(' ')[2]) for l in lines if not l.startswith(('sagen_jpeg_encode_rst ', 'sagen_jpeg_transcode '))}
    assert len(value) == len(QUERIES)
    plain = 2 * ((24 * 1658 + 7) // 8) + 2                             # 17 x 23 at 4:2:0: 2 x 2 MCUs of 6 blocks
    mx = lambda *a: value[('sagen_jpeg_encode_rst_max_bytes', ','.join(str(v) for v in a))]
    assert [mx(17, 23, 3, 2, 2, r) for r in (0, 1, 2, 3, 4)] == [plain, plain + 12, plain + 4, plain + 4, plain]
    assert mx(17, 23, 1, 1, 1, 1) == 2 * ((9 * 1658 + 7) // 8) + 2 + 4 * 8
    assert mx(17, 23, 3, 2, 2, 65536) == mx(17, 23, 3, 2, 2, -1) == mx(17, 23, 3, 1, 2, 1) == 0
    sc = lambda *a: value[('sagen_jpeg_encode_rst_scratch_bytes', ','.join(str(v) for v in a))]
    assert sc(2, 17, 23, 3, 2, 2, 0, 4096) == sc(2, 17, 23, 3, 2, 2, 4, 4096) == sc(2, 17, 23, 3, 2, 2, 65535, 4096) > 0
    assert sc(2, 17, 23, 3, 2, 2, 1, 4096) > sc(2, 17, 23, 3, 2, 2, 0, 4096) and sc(2, 17, 23, 3, 2, 2, 1, 4096) % 16 == 0
    assert sc(2, 17, 23, 3, 2, 2, 65536, 4096) == sc(2, 17, 23, 3, 2, 2, -1, 4096) == sc(0, 17, 23, 3, 2, 2, 1, 4096) == 0
    assert sc(2, 17, 23, 3, 1, 2, 1, 4096) == sc(2, 17, 23, 3, 2, 2, 1, 4095) == 0
    tmx = lambda *a: value[('sagen_jpeg_transcode_max_bytes', ','.join(str(v) for v in a))]
    assert tmx(17, 23, 3, 2, 2, 0) == 2 * ((24 * 1660 + 7) // 8) + 2 and tmx(17, 23, 3, 2, 2, 1) == tmx(17, 23, 3, 2, 2, 0) + 12
    assert tmx(17, 23, 1, 1, 1, 3) == 2 * ((9 * 1660 + 7) // 8) + 2 + 8 and tmx(17, 23, 3, 2, 2, 65536) == tmx(17, 23, 3, 1, 2, 1) == 0
    tsc = lambda *a: value[('sagen_jpeg_transcode_scratch_bytes', ','.join(str(v) for v in a))]
    assert tsc(2, 17, 23, 3, 2, 2, 4, 1, 4096) > tsc(2, 17, 23, 3, 2, 2, 4, 0, 4096) > sc(2, 17, 23, 3, 2, 2, 0, 4096) + 2 * 24 * 128 + 4 * 912
    assert tsc(2, 17, 23, 3, 2, 2, 0, 1, 4096) == tsc(2, 17, 23, 3, 2, 2, 4, 65536, 4096) == tsc(0, 17, 23, 3, 2, 2, 4, 1, 4096) == 0
    assert tsc(2, 17, 23, 3, 2, 2, 4, 1, 4095) == 0


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from spatialaudiogen_amd import _lib
    print('\n'.join(refusal_lines(_lib.lib())))
