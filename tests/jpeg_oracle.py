"""A numpy / plain-Python restatement of baseline JPEG decoding as libjpeg's default path does it (the "islow" inverse DCT, "fancy"
triangle upsampling, 16-bit fixed-point YCbCr -> RGB), written from the standard and the arithmetic the issue spells out.  It shares
nothing with spatialaudiogen_amd/jpeg.py (its own marker walk) nor with csrc/jpeg_core.h (bit strings instead of a bit window,
whole-plane numpy instead of per-pixel functions), and is slow: meant for the tiny streams of tests/golden/jpeg_v1.npz.

    decode(data) -> uint8 [h, w, 3]
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _segments(data):
    """{marker: [payload, ...]} up to SOS, then the scan's bytes (to the first marker that is neither FF00 nor RSTn)."""
    assert data[:2] == b'\xff\xd8'
    pos, seen = 2, {}
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        length = (data[pos + 2] << 8) | data[pos + 3]
        seen.setdefault(m, []).append(data[pos + 4:pos + 2 + length])
        pos += 2 + length
        if m == 0xDA:
            break
    end = pos
    while not (data[end] == 0xFF and data[end + 1] not in (0x00, 0xFF) and not 0xD0 <= data[end + 1] <= 0xD7):
        end += 1
    return seen, data[pos:end]


def _huffman(payloads):
    """{(class, id): {(length, code): symbol}}"""
    out = {}
    for p in payloads:
        i = 0
        while i < len(p):
            counts = list(p[i + 1:i + 17])
            syms = p[i + 17:i + 17 + sum(counts)]
            table, code, k = {}, 0, 0
            for length in range(1, 17):
                for _ in range(counts[length - 1]):
                    table[(length, code)] = syms[k]
                    code += 1
                    k += 1
                code <<= 1
            out[(p[i] >> 4, p[i] & 15)] = table
            i += 17 + sum(counts)
    return out


class _Bits(object):
    def __init__(self, chunk):
        raw = chunk.replace(b'\xff\x00', b'\xff')
        self.bits = ''.join('{:08b}'.format(b) for b in raw) + '0' * 64
        self.pos = 0

    def take(self, n):
        v = int(self.bits[self.pos:self.pos + n], 2) if n else 0
        self.pos += n
        return v

    def symbol(self, table):
        for length in range(1, 17):
            s = table.get((length, int(self.bits[self.pos:self.pos + length], 2)))
            if s is not None:
                self.pos += length
                return s
        raise ValueError('no code')


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _idct_pass(x, rounding, shift):
    """x [..., 8] int64 -> [..., 8]: the even / odd parts of the issue, then (v + rounding) >> shift"""
    i0, i1, i2, i3, i4, i5, i6, i7 = [x[..., k] for k in range(8)]
    z1 = (i2 + i6) * 4433
    tmp2, tmp3 = z1 - i6 * 15137, z1 + i2 * 6270
    tmp0, tmp1 = (i0 + i4) << 13, (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], -1)
    assert np.abs(out).max() < 2 ** 31                      # the 32-bit claim of the issue, checked on what is decoded
    return (out + rounding) >> shift


def idct(block):
    """block [8, 8] dequantised, natural order -> uint8 [8, 8]"""
    b = np.asarray(block, np.int64)
    cols = _idct_pass(b.T, 1024, 11).T                      # the column pass first
    rows = _idct_pass(cols, 1 << 17, 18)
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


def _h2v1(p):
    p = p.astype(np.int64)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _h2v2(p):
    p = p.astype(np.int64)
    above = np.concatenate([p[:1], p[:-1]], 0)
    below = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for parity, other in ((0, above), (1, below)):
        colsum = 3 * p + other
        last = np.concatenate([colsum[:, :1], colsum[:, :-1]], 1)
        nxt = np.concatenate([colsum[:, 1:], colsum[:, -1:]], 1)
        even, odd = (3 * colsum + last + 8) >> 4, (3 * colsum + nxt + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * colsum[:, 0] + 8) >> 4, (4 * colsum[:, -1] + 7) >> 4
        out[parity::2, 0::2], out[parity::2, 1::2] = even, odd
    return out


def _fix(v):
    return int(v * 65536 + 0.5)


def decode(data):
    data = bytes(data)
    seen, scan = _segments(data)
    sof = seen[0xC0][0]
    assert sof[0] == 8
    h, w, nc = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    comps = [(sof[6 + 3 * i], sof[7 + 3 * i] >> 4, sof[7 + 3 * i] & 15, sof[8 + 3 * i]) for i in range(nc)]
    if nc == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    qt = {}
    for p in seen[0xDB]:
        for i in range(0, len(p), 65):
            qt[p[i] & 15] = list(p[i + 1:i + 65])
    huff = _huffman(seen[0xC4])
    restart = (seen[0xDD][0][0] << 8 | seen[0xDD][0][1]) if 0xDD in seen else 0
    sos = seen[0xDA][0]
    tables = {sos[1 + 2 * i]: (sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15) for i in range(sos[0])}
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    planes = [np.zeros((my * 8 * c[2], mx * 8 * c[1]), np.uint8) for c in comps]
    # the scan, cut at the restart markers
    chunks, start, i = [], 0, 0
    while i < len(scan) - 1:
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            chunks.append(scan[start:i])
            start = i + 2
            i += 2
        else:
            i += 1
    chunks.append(scan[start:])
    mcu = 0
    for chunk in chunks:
        bits, pred = _Bits(chunk), [0] * nc
        for _ in range(restart if restart else mx * my):
            if mcu == mx * my:
                break
            for ci, (cid, ch, cv, tq) in enumerate(comps):
                for by in range(cv):
                    for bx in range(ch):
                        coef = [0] * 64
                        t = bits.symbol(huff[(0, tables[cid][0])])
                        pred[ci] += _extend(bits.take(t), t)
                        coef[0] = pred[ci] * qt[tq][0]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(huff[(1, tables[cid][1])])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            coef[ZIGZAG[k]] = _extend(bits.take(s), s) * qt[tq][k]
                            k += 1
                        y0, x0 = ((mcu // mx) * cv + by) * 8, ((mcu % mx) * ch + bx) * 8
                        planes[ci][y0:y0 + 8, x0:x0 + 8] = idct(np.array(coef).reshape(8, 8))
            mcu += 1
    assert mcu == mx * my
    lum = planes[0][:h, :w].astype(np.int64)
    if nc == 1:
        return np.stack([lum] * 3, -1).astype(np.uint8)
    full = []
    for ci in (1, 2):
        hs, vs = hmax // comps[ci][1], vmax // comps[ci][2]
        p = planes[ci][:-(-h // vs), :-(-w // hs)]         # the downsampled plane's true size: the edges are replicated HERE
        up = p.astype(np.int64) if (hs, vs) == (1, 1) else (_h2v1(p) if (hs, vs) == (2, 1) else _h2v2(p))
        full.append(up[:h, :w] - 128)
    cb, cr = full
    r = lum + ((_fix(1.402) * cr + 32768) >> 16)
    g = lum + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = lum + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
