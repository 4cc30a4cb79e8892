"""Writes tests/golden/jpeg_rst_v1.npz: small uint8 images and the complete files PIL on libjpeg-turbo wrote for them WITH a restart
interval (standard Huffman tables, restart_marker_blocks=R), the expectation of tests/test_jpeg_rst_host.py,
tests/test_cpu_twin_jpeg_rst.py and tests/test_gpu_jpeg_rst.py, in the manner of tools/make_jpeg_enc_fixture.py.

    python tools/make_jpeg_rst_fixture.py

Refuses to run on a PIL that is not linked against libjpeg-turbo.  Deterministic; two cases need a property of the STREAM and search
seeds until it holds, and the tool asserts that each is present:
    nofill   a segment that is not the last ends exactly on a byte: no fill bit in front of its marker
    ffill    a segment that is not the last ends inside a byte whose bits are all ones: the fill makes FF, which is stuffed, FF 00 FF Dx
The interval 'row' is one row of MCUs, 'over' more than the frame holds (DRI, no marker)."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SUB = {'444': 0, '422': 1, '420': 2}
FACTORS = {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'grey': (1, 1)}

# (sampling, width, height, quality, content, interval)
CASES = [('420', 1, 1, 75, 'smooth', 1), ('grey', 1, 1, 75, 'noise', 1), ('444', 8, 8, 95, 'noise', 'over'), ('422', 8, 8, 1, 'saturated', 2),
         ('420', 17, 23, 75, 'noise', 1), ('420', 17, 23, 75, 'smooth', 1), ('420', 17, 23, 75, 'saturated', 1),
         ('420', 17, 23, 1, 'noise', 2), ('420', 17, 23, 100, 'noise', 'row'), ('422', 17, 23, 75, 'smooth', 2),
         ('444', 17, 23, 95, 'saturated', 'row'), ('grey', 17, 23, 100, 'smooth', 1),
         ('444', 16, 16, 100, 'nofill', 1), ('444', 16, 16, 100, 'ffill', 1), ('444', 16, 16, 100, 'noise', 1),
         ('420', 9, 33, 95, 'smooth', 1), ('420', 33, 18, 30, 'noise', 2), ('422', 33, 18, 100, 'saturated', 1),
         ('420', 40, 35, 95, 'noise', 1), ('444', 24, 40, 1, 'smooth', 1), ('grey', 40, 35, 75, 'saturated', 'row'),
         ('420', 48, 64, 95, 'smooth', 'row'), ('420', 48, 64, 95, 'noise', 1), ('grey', 48, 64, 95, 'smooth', 'row'), ('grey', 48, 64, 75, 'noise', 1),
         ('420', 48, 64, 75, 'noise', 'over'),
         ('420', 40, 72, 95, 'noise', 'row'), ('422', 40, 72, 75, 'saturated', 2), ('444', 40, 72, 100, 'noise', 'row'), ('grey', 40, 72, 1, 'smooth', 2)]


def mcus(sub, w, h):
    fh, fv = FACTORS[sub]
    return -(-w // (8 * fh)), -(-h // (8 * fv))


def interval_of(sub, w, h, interval):
    mx, my = mcus(sub, w, h)
    return {'row': mx, 'over': mx * my + 85}.get(interval, interval)


def pil_file(img, quality, sub, interval):
    from PIL import Image
    b = io.BytesIO()
    if img.ndim == 2:
        Image.fromarray(img).save(b, 'JPEG', quality=quality, restart_marker_blocks=interval)
    else:
        Image.fromarray(img).save(b, 'JPEG', quality=quality, subsampling=SUB[sub], restart_marker_blocks=interval)
    return b.getvalue()


def segments_of(img, quality, sub, interval):
    import jpeg_enc_oracle as JE
    import jpeg_rst_oracle as JR
    hs, vs = FACTORS[sub]
    return JR.segment_bits(img, JE.tables(quality), hs, vs, interval)


def has_nofill(segs):
    return any(len(s) % 8 == 0 for s in segs[:-1])


def has_ffill(segs):
    return any(len(s) % 8 and set(s[len(s) // 8 * 8:]) == {'1'} for s in segs[:-1])


def main():
    from PIL import features
    from make_jpeg_enc_fixture import image
    if not features.check_feature('libjpeg_turbo'):
        sys.exit('make_jpeg_rst_fixture: this PIL is not linked against libjpeg-turbo; the fixture must hold that library\'s files')
    out = {'names': [], 'quality': [], 'sampling': [], 'interval': []}
    seen = {'nofill': False, 'ffill': False, 'wrap': False, 'over': False}
    for k, (sub, w, h, q, kind, interval) in enumerate(CASES):
        R = interval_of(sub, w, h, interval)
        want = {'nofill': has_nofill, 'ffill': has_ffill}.get(kind)
        for seed in range(1000 * k, 1000 * k + 1000):
            img = image('noise' if want else kind, w, h, sub == 'grey', seed)
            if want is None or want(segments_of(img, q, sub, R)):
                break
        else:
            sys.exit('no seed gives a %s stream for %s' % (kind, (sub, w, h, q)))
        data = pil_file(img, q, sub, R)
        segs = segments_of(img, q, sub, R)
        assert data[data.index(b'\xff\xda') - 6:data.index(b'\xff\xda')] == b'\xff\xdd\x00\x04' + R.to_bytes(2, 'big')
        if kind == 'nofill':
            assert has_nofill(segs)
            seen['nofill'] = True
        if kind == 'ffill':
            assert has_ffill(segs) and any(b'\xff\x00\xff' + bytes([0xD0 + j]) in data for j in range(8))
            seen['ffill'] = True
        seen['wrap'] = seen['wrap'] or (len(segs) >= 10 and b'\xff\xd7' in data)
        seen['over'] = seen['over'] or (len(segs) == 1 and R > 1)
        assert img.size <= 48 * 64 * 3 or img.shape[:2] == (72, 40)
        out['names'].append('%s_%dx%d_q%d_%s_r%s' % (sub, w, h, q, kind, interval))
        out['quality'].append(q)
        out['sampling'].append(sub)
        out['interval'].append(R)
        out['image_%d' % k] = img
        out['file_%d' % k] = np.frombuffer(data, np.uint8)
    assert all(seen.values()), seen
    assert len(set(out['names'])) == len(CASES)
    path = os.path.join(ROOT, 'tests', 'golden', 'jpeg_rst_v1.npz')
    np.savez_compressed(path, **{k: np.array(v) if isinstance(v, list) else v for k, v in out.items()})
    assert os.path.getsize(path) < 300 * 1024
    print('%s: %d cases, %d bytes' % (path, len(CASES), os.path.getsize(path)))


if __name__ == '__main__':
    main()
