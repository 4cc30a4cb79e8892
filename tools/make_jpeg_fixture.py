"""Write tests/golden/jpeg_v1.npz: tiny baseline JPEG streams as byte strings, the RGB that PIL (libjpeg-turbo) decodes from each
on the machine that runs this, and a handful of streams the parser must refuse.  Everything is made here from seeds; nothing
outside the repository is read.

    python tools/make_jpeg_fixture.py [--out tests/golden/jpeg_v1.npz]

The file holds, per stream k of `names`: bytes_<k> (uint8), rgb_<k> (uint8 [h, w, 3]); per reject k of `reject_names`:
reject_<k> (uint8) and reject_reasons[k], a word the reason must contain.  It refuses to run where PIL is not linked against
libjpeg-turbo: the expected pixels are that library's.
"""
import argparse
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def picture(w, h, kind, seed):
    r = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == 'noise':
        a = r.randint(0, 256, (h, w, 3))
    elif kind == 'smooth':
        a = np.stack([127 + 120 * np.sin(x / 5. + seed), 127 + 120 * np.cos(y / 7.), (x * 3 + y * 5) % 256], -1) + r.randint(-6, 7, (h, w, 3))
    else:                                           # saturated checkerboard: clamps of the transform and of the colour step
        a = np.where(((x // 3 + y // 2) % 2)[..., None] > 0, [255, 0, 255], [0, 255, 0])
    return np.clip(a, 0, 255).astype(np.uint8)


# name -> (w, h, content, subsampling (PIL's 0 / 1 / 2, or 'grey'), quality, optimize, restart keyword or None)
STREAMS = [
    ('444_8x8_q75', 8, 8, 'smooth', 0, 75, False, None),
    ('422_16x8_q75', 16, 8, 'smooth', 1, 75, False, None),
    ('420_16x16_q75', 16, 16, 'smooth', 2, 75, False, None),
    ('grey_8x8_q75', 8, 8, 'smooth', 'grey', 75, False, None),
    ('420_8x8_q75_one_chroma_column', 8, 8, 'noise', 2, 75, False, None),
    ('420_8x9_q30', 8, 9, 'noise', 2, 30, False, None),
    ('444_17x23_q75', 17, 23, 'noise', 0, 75, False, None),
    ('422_17x23_q75', 17, 23, 'noise', 1, 75, True, None),
    ('420_17x23_q75', 17, 23, 'noise', 2, 75, False, None),
    ('420_17x23_q1', 17, 23, 'noise', 2, 1, False, None),
    ('420_17x23_q100_opt', 17, 23, 'smooth', 2, 100, True, None),
    ('420_17x23_q30_rows', 17, 23, 'smooth', 2, 30, False, 'rows'),
    ('grey_17x23_q30_opt', 17, 23, 'noise', 'grey', 30, True, None),
    ('444_9x31_q30', 9, 31, 'smooth', 0, 30, True, None),
    ('422_9x31_q100', 9, 31, 'noise', 1, 100, False, None),
    ('420_9x31_q75_blocks', 9, 31, 'noise', 2, 75, False, 'blocks'),
    ('grey_9x31_q100', 9, 31, 'smooth', 'grey', 100, False, 'blocks'),
    ('444_33x18_q1', 33, 18, 'smooth', 0, 1, False, None),
    ('422_33x18_q30_blocks', 33, 18, 'noise', 1, 30, True, 'blocks'),
    ('420_33x18_q75_opt', 33, 18, 'smooth', 2, 75, True, None),
    ('420_33x18_q100', 33, 18, 'noise', 2, 100, False, 'rows'),
    ('444_24x40_q75_rows', 24, 40, 'noise', 0, 75, False, 'rows'),
    ('422_24x40_q30', 24, 40, 'smooth', 1, 30, False, None),
    ('420_24x40_saturated_q95', 24, 40, 'saturated', 2, 95, False, None),
    ('444_16x16_saturated_q1', 16, 16, 'saturated', 0, 1, False, None),
    ('420_40x56_q75', 40, 56, 'smooth', 2, 75, False, None),
    ('420_40x56_q30_opt_blocks', 40, 56, 'noise', 2, 30, True, 'blocks'),
    ('422_40x56_q75_rows', 40, 56, 'smooth', 1, 75, True, 'rows'),
    ('420_48x64_q75_blocks', 48, 64, 'smooth', 2, 75, False, 'blocks'),
    ('420_48x64_q95_opt', 48, 64, 'noise', 2, 95, True, None),
]


def encode(w, h, kind, sub, quality, optimize, restart, seed, **extra):
    from PIL import Image
    im = Image.fromarray(picture(w, h, kind, seed))
    kw = dict(quality=quality, optimize=optimize, **extra)
    if sub == 'grey':
        im = im.convert('L')
    elif sub is not None:
        kw['subsampling'] = sub
    if restart == 'blocks':
        kw['restart_marker_blocks'] = 3
    elif restart == 'rows':
        kw['restart_marker_rows'] = 1
    b = io.BytesIO()
    im.save(b, 'JPEG', **kw)
    return b.getvalue()


def rejects():
    """(name, bytes, word of the reason)"""
    from PIL import Image
    out = [('progressive', encode(24, 24, 'smooth', 2, 75, False, None, 1, progressive=True), 'progressive')]
    b = io.BytesIO()
    Image.fromarray(picture(16, 16, 'smooth', 2)).convert('CMYK').save(b, 'JPEG', quality=75)
    out.append(('cmyk', b.getvalue(), 'four components'))
    # 4:1:1 and 4:4:0 by editing the luma sampling byte of a 4:2:2 header (h2 v1 -> h4 v1, h1 v2): the parser reads headers only
    for name, hv in (('411', 0x41), ('440', 0x12)):
        d = bytearray(encode(32, 16, 'smooth', 1, 75, False, None, 3))
        sof = d.find(b'\xff\xc0')
        assert sof > 0 and d[sof + 11] == 0x21
        d[sof + 11] = hv
        out.append((name, bytes(d), 'sampling'))
    # 12-bit samples by editing the precision byte
    d = bytearray(encode(8, 8, 'smooth', 0, 75, False, None, 5))
    sof = d.find(b'\xff\xc0')
    d[sof + 4] = 12
    out.append(('12bit', bytes(d), '12-bit'))
    return out


def main():
    from PIL import Image, features
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'jpeg_v1.npz'))
    args = ap.parse_args()
    if not features.check_feature('libjpeg_turbo'):
        raise SystemExit('make_jpeg_fixture: this PIL is not linked against libjpeg-turbo; the fixture records that library\'s pixels')
    arrays = {'names': np.array([s[0] for s in STREAMS])}
    for k, (name, w, h, kind, sub, q, opt, rst) in enumerate(STREAMS):
        data = encode(w, h, kind, sub, q, opt, rst, 100 + k)
        arrays['bytes_%d' % k] = np.frombuffer(data, np.uint8)
        arrays['rgb_%d' % k] = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    rej = rejects()
    arrays['reject_names'] = np.array([r[0] for r in rej])
    arrays['reject_reasons'] = np.array([r[2] for r in rej])
    for k, r in enumerate(rej):
        arrays['reject_%d' % k] = np.frombuffer(r[1], np.uint8)
    np.savez_compressed(args.out, **arrays)
    print('wrote %s: %d streams, %d rejects, %d bytes' % (args.out, len(STREAMS), len(rej), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
