"""Restart intervals on top of tests/jpeg_enc_oracle.py, as libjpeg writes them: in front of MCU number k R (k >= 1, never behind the
last MCU) the bits are filled with ones to a byte, that byte is stuffed like any other, FF D0+((k-1) & 7) follows unstuffed, and every
component's DC prediction goes back to 0.  encode(image, quality, subsampling, interval) -> the complete file PIL's
Image.save(..., 'JPEG', quality=, subsampling=, restart_marker_blocks=interval) writes.  It shares nothing with
spatialaudiogen_amd/jpeg.py or csrc/jpeg_enc_core.h.

Test infrastructure (tests/test_jpeg_rst_host.py checks it against files PIL wrote on libjpeg-turbo)."""
import numpy as np

import jpeg_enc_oracle as JE


def segment_bits(image, qtabs, hs, vs, interval):
    """the entropy-coded data of each restart segment before fill and stuffing: a list of bit strings (one without an interval)"""
    image = np.asarray(image)
    grey = image.ndim == 2
    fh, fv = (1, 1) if grey else (hs, vs)
    comps = JE.planes(image, fh, fv)
    coefs = [JE.coefficients(p, qtabs[min(c, 1)]) for c, (p, _, _) in enumerate(comps)]
    dc = [JE.codes(JE.DC_LUMA)] + [JE.codes(JE.DC_CHROMA)] * 2
    ac = [JE.codes(JE.AC_LUMA)] + [JE.codes(JE.AC_CHROMA)] * 2
    h, w = image.shape[:2]
    mcus_y, mcus_x = -(-h // (8 * fv)), -(-w // (8 * fh))
    segments, pred = [[]], [0, 0, 0]

    def block(c, zz):
        out = segments[-1]
        diff = int(zz[0]) - pred[c]
        pred[c] = int(zz[0])
        out += [dc[c][JE.category(diff)], JE.value_bits(diff)]
        run = 0
        for v in zz[1:]:
            if v == 0:
                run += 1
                continue
            out += [ac[c][0xF0]] * (run >> 4) + [ac[c][((run & 15) << 4) | JE.category(v)], JE.value_bits(int(v))]
            run = 0
        if run:
            out.append(ac[c][0])

    for m in range(mcus_y * mcus_x):
        if interval and m and m % interval == 0:
            segments.append([])
            pred = [0, 0, 0]
        my, mx = divmod(m, mcus_x)
        for j in range(fv * fh):
            by, bx = my * fv + j // fh, mx * fh + j % fh
            if by < comps[0][1] and bx < comps[0][2]:
                block(0, coefs[0][by, bx])
            else:
                segments[-1] += [dc[0][0], ac[0][0]]                       # a dummy repeats the DC in front of it: difference 0, no AC
        for c in range(1, len(comps)):
            block(c, coefs[c][my, mx])
    return [''.join(s) for s in segments]


def scan(segments):
    """fill, stuffing and the markers between the segments"""
    out = b''
    for k, bits in enumerate(segments):
        if k:
            out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        out += JE.stuffed(bits)
    return out


def header(w, h, grey, hs, vs, qtabs, interval):
    head = JE.header(w, h, grey, hs, vs, qtabs)
    if not interval:
        return head
    at = head.rindex(b'\xff\xda')                                          # (no FF DA inside the tables: the header of these files)
    return head[:at] + b'\xff\xdd\x00\x04' + int(interval).to_bytes(2, 'big') + head[at:]


def encode(image, quality=75, subsampling='4:2:0', interval=0):
    image = np.asarray(image)
    grey = image.ndim == 2
    hs, vs = (1, 1) if grey else JE.SAMPLING[subsampling]
    q = JE.tables(quality)
    return header(image.shape[1], image.shape[0], grey, hs, vs, q, interval) + scan(segment_bits(image, q, hs, vs, interval)) + b'\xff\xd9'
