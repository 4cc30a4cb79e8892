"""Baseline JPEG encode, the host side (no GPU): tests/golden/jpeg_enc_v1.npz (tools/make_jpeg_enc_fixture.py: images and the complete
files PIL wrote for them on libjpeg-turbo) against the numpy restatement tests/jpeg_enc_oracle.py, and the header pieces of
spatialaudiogen_amd/jpeg.py (quality_tables, encode_header) against live PIL.  Every comparison is equality of bytes."""
import io
import os

import numpy as np
import pytest

import jpeg_enc_oracle as JE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSAMPLING = {'444': '4:4:4', '422': '4:2:2', '420': '4:2:0', 'grey': '4:2:0'}      # (a grey image has no subsampling; any name will do)
PIL_SUB = {'444': 0, '422': 1, '420': 2}
FACTORS = {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'grey': (1, 1)}
_FIXTURE = {}


def fixture():
    """(names, {name: image}, {name: file bytes}, {name: quality}, {name: '444' | '422' | '420' | 'grey'}) - loaded once, never changed."""
    if not _FIXTURE:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_enc_v1.npz'))
        names = [str(n) for n in z['names']]
        _FIXTURE['v'] = (names, {n: z['image_%d' % k] for k, n in enumerate(names)}, {n: z['file_%d' % k].tobytes() for k, n in enumerate(names)},
                         {n: int(z['quality'][k]) for k, n in enumerate(names)}, {n: str(z['sampling'][k]) for k, n in enumerate(names)})
    return _FIXTURE['v']


def turbo():
    from PIL import features
    return bool(features.check_feature('libjpeg_turbo'))


def scan_of(data):
    """the entropy-coded bytes of a file without restart markers: between the SOS header and FF D9"""
    at = data.index(b'\xff\xda')
    return data[at + 2 + ((data[at + 2] << 8) | data[at + 3]):-2]


def pil_file(img, quality, sampling):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', quality=quality, **({} if img.ndim == 2 else dict(subsampling=PIL_SUB[sampling])))
    return b.getvalue()


def test_the_fixture_covers_what_the_issue_lists():
    names, image, data, quality, sampling = fixture()
    assert len(names) <= 30 and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg_enc_v1.npz')) < 300 * 1024
    assert max(v.size for v in image.values()) <= 48 * 64 * 3
    for word in ('_1x1_', '_8x8_', '_16x16_', '_17x23_', '_9x33_', '_33x18_', '_40x35_', '_24x40_', '_48x64_', '444_', '422_', '420_', 'grey_',
                 '_q1_', '_q30_', '_q75_', '_q95_', '_q100_', 'noise', 'smooth', 'saturated'):
        assert any(word in n for n in names), word
    assert any(n.startswith('420_') and image[n].shape[0] % 2 == 0 and image[n].shape[0] % 16 for n in names)     # even height, padded chroma rows
    assert any(n.startswith('420_') and image[n].shape[0] % 2 == 1 for n in names)
    assert set(np.unique(image['420_17x23_q30_saturated'])) == {0, 255}
    assert max(scan_of(d).count(b'\xff\x00') for d in data.values()) >= 20
    n = '420_16x16_q100_fill'
    bits = JE.scan_bits(image[n], JE.tables(quality[n]), 2, 2)
    assert len(bits) % 8 != 0 and bits[len(bits) // 8 * 8:] == '1' * (len(bits) % 8) and scan_of(data[n])[-2:] == b'\xff\x00'


@pytest.mark.parametrize('k', range(30))
def test_restatement_equals_the_fixture(k):
    names, image, data, quality, sampling = fixture()
    assert len(names) == 30
    n = names[k]
    assert JE.encode(image[n], quality[n], SUBSAMPLING[sampling[n]]) == data[n], n


def test_restatement_equals_live_pil():
    if not turbo():
        pytest.skip('this PIL is not linked against libjpeg-turbo: another encoder need not agree to the byte')
    rs = np.random.RandomState(7)
    for w, h, sampling, q in ((19, 21, '420', 20), (33, 18, '422', 90), (9, 31, '444', 5), (26, 40, '420', 97), (16, 14, 'grey', 60), (7, 9, '420', 50)):
        y, x = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([x * 7, y * 9, 128 + 100 * np.sin(x / 3.)], -1) + rs.randint(-40, 40, (h, w, 3)), 0, 255).astype(np.uint8)
        a = np.ascontiguousarray(a[..., 0]) if sampling == 'grey' else a
        assert JE.encode(a, q, SUBSAMPLING[sampling]) == pil_file(a, q, sampling), (w, h, sampling, q)


def test_tables_and_header_equal_the_head_of_a_live_pil_file():
    from spatialaudiogen_amd import jpeg
    rs = np.random.RandomState(8)
    for q in (1, 50, 95, 100):
        t = jpeg.quality_tables(q)
        assert t.dtype == np.uint16 and t.shape == (2, 64) and t.min() >= 1 and t.max() <= 255
        assert np.array_equal(t, np.stack(JE.tables(q)))
        for sampling in ('444', '422', '420', 'grey'):
            img = rs.randint(0, 256, (23, 17) if sampling == 'grey' else (23, 17, 3)).astype(np.uint8)
            want = pil_file(img, q, sampling)
            hs, vs = FACTORS[sampling]
            head = jpeg.encode_header(17, 23, 1 if sampling == 'grey' else 3, hs, vs, t)
            assert want[:len(head)] == head and len(head) == len(want) - len(scan_of(want)) - 2, (q, sampling)
    assert np.array_equal(jpeg.quality_tables(0), jpeg.quality_tables(1)) and np.array_equal(jpeg.quality_tables(101), jpeg.quality_tables(100))
    with pytest.raises(ValueError):
        jpeg.encode_header(8, 8, 3, 1, 2, jpeg.quality_tables(75))
    with pytest.raises(ValueError):
        jpeg.encode_header(8, 8, 1, 2, 2, jpeg.quality_tables(75))


def test_parse_of_a_fixture_file_returns_the_geometry_asked_for():
    from spatialaudiogen_amd import jpeg
    names, image, data, quality, sampling = fixture()
    for n in names:
        i = jpeg.parse(data[n])
        h, w = image[n].shape[:2]
        assert (i.width, i.height, i.components, i.hs, i.vs) == (w, h, 1 if sampling[n] == 'grey' else 3) + FACTORS[sampling[n]], n
        assert i.restart_interval == 0 and data[n][i.scan_offset:i.scan_offset + i.scan_bytes] == scan_of(data[n])
        rows = min(i.components, 2)                                     # (the file holds its tables in zigzag order)
        assert np.array_equal(np.stack(i.qtabs[:rows]), jpeg.quality_tables(quality[n])[:rows][:, JE.zigzag()]), n
