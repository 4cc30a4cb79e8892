"""A numpy / plain-Python restatement of baseline JPEG ENCODING as libjpeg does it with its defaults (the "islow" forward DCT, the
standard Huffman tables, h2v1 / h2v2 box downsampling with the alternating bias): encode(image, quality, subsampling) -> the complete
file PIL's Image.save(..., 'JPEG', quality=, subsampling=) writes.  It shares nothing with spatialaudiogen_amd/jpeg.py or
csrc/jpeg_enc_core.h: whole planes in numpy, the entropy-coded data as a string of '0' / '1' characters.

Test infrastructure (tests/test_jpeg_enc_host.py checks it against files PIL wrote on libjpeg-turbo)."""
import numpy as np

# Annex K.1 / K.2 (natural order) and K.3 - K.6 (counts per code length, then the symbols)
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
            0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
            0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
            0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
            0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
            0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
            0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
            0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
              0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
              0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
              0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
              0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
              0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
              0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
              0xfa])
SAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2), 0: (1, 1), 1: (2, 1), 2: (2, 2)}


def zigzag():
    """natural index of the k-th zigzag coefficient: the anti-diagonals of the 8 x 8 block, alternating direction"""
    order = sorted(((r + c, r if (r + c) % 2 else c, 8 * r + c) for r in range(8) for c in range(8)))
    return np.array([n for _, _, n in order])


def tables(quality):
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((t * scale + 50) // 100, 1, 255) for t in (K1, K2)]


def codes(spec):
    """symbol -> its code as a bit string (Annex C: codes of one length count upwards, then a zero is appended)"""
    out, code, k = {}, 0, 0
    for length, count in enumerate(spec[0], 1):
        for _ in range(count):
            out[spec[1][k]] = format(code, '0%db' % length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def category(v):
    return int(abs(int(v))).bit_length()


def value_bits(v):
    n = category(v)
    return format(v if v >= 0 else v - 1 + (1 << n), '0%db' % n) if n else ''


def planes(image, hs, vs):
    """the component planes, padded to whole blocks: [(plane int64 [8 hb, 8 wb], real blocks hb, wb)]"""
    image = np.asarray(image).astype(np.int64)
    h, w = image.shape[:2]
    if image.ndim == 2:
        comps = [(image, 1, 1)]
    else:
        r, g, b = image[..., 0], image[..., 1], image[..., 2]
        comps = [((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, 1, 1),
                 ((-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16, hs, vs),
                 ((32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16, hs, vs)]
    out = []
    for p, fh, fv in comps:
        wc, hc = -(-w // fh), -(-h // fv)
        wb, hb = -(-wc // 8), -(-hc // 8)
        p = np.pad(p, ((0, hc * fv - h), (0, 8 * wb * fh - w)), 'edge')        # the image's columns and rows, before any averaging
        if fh == 2:
            bias = np.tile([1, 2] if fv == 2 else [0, 1], 4 * wb)
            if fv == 2:
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            else:
                p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        p = np.pad(p, ((0, 8 * hb - hc), (0, 0)), 'edge')                      # then the COMPONENT's last row
        out.append((p, hb, wb))
    return out


def _pass(d, shift, first):
    """the butterfly along the last axis of d [..., 8]"""
    D = lambda x: (x + (1 << (shift - 1))) >> shift
    t0, t1, t2, t3 = d[..., 0] + d[..., 7], d[..., 1] + d[..., 6], d[..., 2] + d[..., 5], d[..., 3] + d[..., 4]
    t7, t6, t5, t4 = d[..., 0] - d[..., 7], d[..., 1] - d[..., 6], d[..., 2] - d[..., 5], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0], o[4] = ((t10 + t11) << 2, (t10 - t11) << 2) if first else ((t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2)
    z = (t12 + t13) * 4433
    o[2], o[6] = D(z + t13 * 6270), D(z - t12 * 15137)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = D(t4 + z1 + z3), D(t5 + z2 + z4), D(t6 + z2 + z3), D(t7 + z1 + z4)
    return np.stack(o, -1)


def coefficients(plane, qnat):
    """[hb8, wb8] quantised blocks in zigzag order: [hb8 wb8][64]"""
    H, W = plane.shape
    b = (plane - 128).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)           # [by, bx, row, col]
    b = _pass(b, 11, True)
    b = _pass(b.transpose(0, 1, 3, 2), 15, False).transpose(0, 1, 3, 2)
    Q = 8 * qnat.reshape(8, 8)
    a = (np.abs(b) + (Q >> 1)) // Q
    return np.where(b < 0, -a, a).reshape(H // 8, W // 8, 64)[..., zigzag()]


def scan_bits(image, qtabs, hs, vs):
    """the entropy-coded data before fill and stuffing, as a bit string"""
    grey = np.asarray(image).ndim == 2
    comps = planes(image, 1 if grey else hs, 1 if grey else vs)
    coefs = [coefficients(p, qtabs[min(c, 1)]) for c, (p, _, _) in enumerate(comps)]
    dc = [codes(DC_LUMA)] + [codes(DC_CHROMA)] * 2
    ac = [codes(AC_LUMA)] + [codes(AC_CHROMA)] * 2
    fh, fv = (1, 1) if grey else (hs, vs)
    h, w = np.asarray(image).shape[:2]
    pred, last, out = [0, 0, 0], None, []

    def block(c, zz):
        bits = [dc[c][category(zz[0] - pred[c])], value_bits(int(zz[0] - pred[c]))]
        pred[c] = int(zz[0])
        run = 0
        for v in zz[1:]:
            if v == 0:
                run += 1
                continue
            bits += [ac[c][0xF0]] * (run >> 4) + [ac[c][((run & 15) << 4) | category(v)], value_bits(int(v))]
            run = 0
        if run:
            bits.append(ac[c][0])
        out.extend(bits)

    for my in range(-(-h // (8 * fv))):
        for mx in range(-(-w // (8 * fh))):
            for j in range(fv * fh):
                by, bx = my * fv + j // fh, mx * fh + j % fh
                if by < comps[0][1] and bx < comps[0][2]:
                    block(0, coefs[0][by, bx])
                else:
                    out.extend([dc[0][0], ac[0][0]])                              # a dummy: the DC of the block before it, no AC
            for c in range(1, len(comps)):
                block(c, coefs[c][my, mx])
    return ''.join(out)


def stuffed(bits):
    bits += '1' * (-len(bits) % 8)
    raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    return raw.replace(b'\xff', b'\xff\x00')


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + body


def header(w, h, grey, hs, vs, qtabs):
    zz = zigzag()
    out = b'\xff\xd8' + _seg(0xE0, b'JFIF\0\x01\x01\0\0\x01\0\x01\0\0')
    for i in range(1 if grey else 2):
        out += _seg(0xDB, bytes([i]) + bytes(int(v) for v in qtabs[i][zz]))
    comps = [(1, 0x11, 0)] if grey else [(1, (hs << 4) | vs, 0), (2, 0x11, 1), (3, 0x11, 1)]
    out += _seg(0xC0, bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([len(comps)]) + b''.join(bytes(c) for c in comps))
    for ident, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))[:2 if grey else 4]:
        out += _seg(0xC4, bytes([ident]) + bytes(spec[0]) + bytes(spec[1]))
    return out + _seg(0xDA, bytes([len(comps)]) + b''.join(bytes([c[0], c[2] * 0x11]) for c in comps) + b'\0\x3f\0')


def encode(image, quality=75, subsampling='4:2:0'):
    """image uint8 [h, w, 3] (RGB) or [h, w] (grey) -> the file"""
    image = np.asarray(image)
    grey = image.ndim == 2
    hs, vs = (1, 1) if grey else SAMPLING[subsampling]
    q = tables(quality)
    return header(image.shape[1], image.shape[0], grey, hs, vs, q) + stuffed(scan_bits(image, q, hs, vs)) + b'\xff\xd9'
