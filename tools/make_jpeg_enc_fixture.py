"""Writes tests/golden/jpeg_enc_v1.npz: small uint8 images and the complete files PIL on libjpeg-turbo wrote for them (standard Huffman
tables, no restart interval: PIL's defaults), the expectation of tests/test_jpeg_enc_host.py, tests/test_gpu_jpeg_enc.py and
tests/test_cpu_twin_jpeg_enc.py.

    python tools/make_jpeg_enc_fixture.py

Refuses to run on a PIL that is not linked against libjpeg-turbo: the files must be the ones the contract names.  Deterministic;
the two cases that need a property of the STREAM (>= 20 stuffed FFs; a last byte that is a filled FF) search seeds until it holds.  (The
filled FF needs a frame of whole MCUs: a padded last block is smooth and ends in an end-of-block code, whose bits are zeros.)"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = {'444': 0, '422': 1, '420': 2}

# (sampling, width, height, quality, content)
CASES = [('420', 1, 1, 75, 'smooth'), ('444', 1, 1, 95, 'noise'), ('grey', 1, 1, 75, 'noise'),
         ('420', 8, 8, 75, 'noise'), ('444', 8, 8, 30, 'smooth'), ('422', 8, 8, 95, 'saturated'),
         ('420', 16, 16, 95, 'noise'), ('grey', 16, 16, 100, 'noise'),
         ('420', 17, 23, 75, 'noise'), ('420', 17, 23, 1, 'noise'), ('420', 17, 23, 100, 'noise'), ('420', 17, 23, 95, 'noise'),
         ('420', 17, 23, 95, 'smooth'), ('420', 16, 16, 100, 'fill'), ('420', 17, 23, 30, 'saturated'),
         ('422', 17, 23, 75, 'smooth'), ('444', 17, 23, 95, 'saturated'), ('grey', 17, 23, 30, 'smooth'),
         ('420', 9, 33, 95, 'smooth'), ('444', 9, 33, 75, 'noise'), ('420', 33, 18, 30, 'noise'), ('422', 33, 18, 100, 'saturated'),
         ('420', 40, 35, 95, 'noise'), ('grey', 40, 35, 75, 'saturated'), ('420', 24, 40, 95, 'smooth'), ('422', 24, 40, 30, 'noise'),
         ('444', 24, 40, 1, 'smooth'), ('420', 48, 64, 95, 'smooth'), ('420', 48, 64, 95, 'stuffed'), ('grey', 48, 64, 95, 'smooth')]


def image(kind, w, h, grey, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == 'smooth':
        a = np.stack([127 + 100 * np.sin(x / 5. + seed), 127 + 100 * np.cos(y / 7.), (5 * x + 3 * y) % 256], -1) + rs.randint(-3, 4, (h, w, 3))
    elif kind == 'saturated':
        a = 255 * rs.randint(0, 2, (h, w, 3))
    else:
        a = rs.randint(0, 256, (h, w, 3))
    a = np.clip(a, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(a[..., 1]) if grey else a


def pil_file(img, quality, sub):
    from PIL import Image
    b = io.BytesIO()
    if img.ndim == 2:
        Image.fromarray(img).save(b, 'JPEG', quality=quality)
    else:
        Image.fromarray(img).save(b, 'JPEG', quality=quality, subsampling=SUB[sub])
    return b.getvalue()


def scan_of(data):
    """the entropy-coded bytes: between the SOS header and FF D9 (there are no restart markers)"""
    at = data.index(b'\xff\xda')
    start = at + 2 + ((data[at + 2] << 8) | data[at + 3])
    assert data[-2:] == b'\xff\xd9'
    return data[start:-2]


def filled(img, quality, sub):
    """whether the stream's bits end inside a byte (tests/jpeg_enc_oracle.py knows the bit count; the file does not show it)"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import jpeg_enc_oracle as JE
    hs, vs = JE.SAMPLING[SUB[sub]]
    return len(JE.scan_bits(img, JE.tables(quality), hs, vs)) % 8 != 0


def main():
    from PIL import features
    if not features.check_feature('libjpeg_turbo'):
        sys.exit('make_jpeg_enc_fixture: this PIL is not linked against libjpeg-turbo; the fixture must hold that library\'s files')
    out = {'names': [], 'quality': [], 'sampling': []}
    assert len(CASES) <= 30
    for k, (sub, w, h, q, kind) in enumerate(CASES):
        want = {'fill': lambda s, i: s[-2:] == b'\xff\x00' and filled(i, q, sub),
                'stuffed': lambda s, i: s.count(b'\xff\x00') >= 20}.get(kind, lambda s, i: True)
        for seed in range(1000 * k, 1000 * k + 1000):
            img = image('noise' if kind in ('fill', 'stuffed') else kind, w, h, sub == 'grey', seed)
            data = pil_file(img, q, sub)
            if want(scan_of(data), img):
                break
        else:
            sys.exit('no seed gives a %s stream for %s' % (kind, (sub, w, h, q)))
        assert img.size <= 48 * 64 * 3
        out['names'].append('%s_%dx%d_q%d_%s' % (sub, w, h, q, kind))
        out['quality'].append(q)
        out['sampling'].append(sub)
        out['image_%d' % k] = img
        out['file_%d' % k] = np.frombuffer(data, np.uint8)
    path = os.path.join(ROOT, 'tests', 'golden', 'jpeg_enc_v1.npz')
    np.savez_compressed(path, **{k: np.array(v) if isinstance(v, list) else v for k, v in out.items()})
    assert os.path.getsize(path) < 300 * 1024
    print('%s: %d cases, %d bytes' % (path, len(CASES), os.path.getsize(path)))


if __name__ == '__main__':
    main()
