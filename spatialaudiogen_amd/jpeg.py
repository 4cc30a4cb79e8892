"""Baseline JPEG frames decoded on the device (include/sagen.h: sagen_jpeg_decode, csrc/jpeg.hip): the host walks the markers,
the device gets the file bytes and produces [N, H, W, 3] uint8, byte for byte what PIL's Image.open(...).convert('RGB') gives
(libjpeg's default path).  It stands in for feeder.imread (feeder.py:18-23 in the reference) in front of the frame consumers.

    parse(data)                         -> JpegInfo, JpegUnsupported(reason) outside the scope, ValueError for no JPEG at all
    JpegDecoder(device).decode(items)   -> torch.uint8 [N, H, W, 3] on the device; items: bytes or paths
    load_frames_device(names, device)   the drop-in for torch.as_tensor(frames.load_frames(names)).to(device); frames.FrameReader chooses

    JpegDecoder(device, entropy='split')  the same pixels with many lanes per frame (sagen_jpeg_decode_split, csrc/jpeg_split.hip): for files
                                        without restart markers; chunk_bytes, rounds: its options; last_paths: who decoded the frames
    split_chunks(packed, chunk_bytes)   the chunks of a packed call: the capacity decode_packed(entropy='split') asks for

Scope (the header has the details): SOF0, 8 bit, Huffman, one interleaved scan, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, optional
restart interval.  A file outside it is decoded by feeder.imread and copied in, with one warning per decoder.

And the way back (sagen_jpeg_encode, csrc/jpeg_enc.hip): frames on the device in, complete files out, byte for byte what PIL's
Image.fromarray(f).save(path, quality=q, subsampling=s) writes on libjpeg (standard Huffman tables, no restart interval).  The device
produces the entropy-coded data; the header and FF D9 are put around it here.

    quality_tables(quality)             -> uint16 [2][64], natural order (libjpeg's scaling of Annex K.1 / K.2)
    encode_header(w, h, components, hs, vs, qtabs, restart_interval=0) -> bytes: SOI .. SOS
    restart_interval_of(w, h, components, hs, vs, restart_rows, restart_blocks) -> MCUs, by PIL's rule (rows win)
    JpegEncoder(device, quality, subsampling, restart_rows=0, restart_blocks=0).encode(frames) -> list of bytes; frames uint8
                                        [n, h, w, 3] or [n, h, w] on the device; with a restart interval (sagen_jpeg_encode_rst) the
                                        files are PIL's for restart_marker_rows / restart_marker_blocks
                                        frames.FrameWriter(out_dir, 'jpg', encode='device') puts them into a folder

Files that exist get their restart interval without a pixel being computed (sagen_jpeg_transcode: the decoder's entropy stage into
coefficients, the encoder's entropy half out of them):

    transcode_files(datas, restart_rows=1, device=None) -> list of bytes, the coefficients of each file unchanged
    python -m spatialaudiogen_amd.jpeg restart IN_DIR OUT_DIR [--rows 1 | --blocks N] [--block 256] [--overwrite]
"""
import collections
import ctypes as C
import warnings

import numpy as np

from . import _lib

JpegInfo = collections.namedtuple('JpegInfo', 'width height components hs vs qtabs dctabs actabs restart_interval scan_offset scan_bytes segments')
JpegInfo.__doc__ = """What the device needs of one file.  qtabs: per component 64 uint16 in the file's (zigzag) order; dctabs / actabs: per
component 272 bytes (16 counts + 256 symbols, unused symbols zero); scan_offset / scan_bytes: the entropy-coded data (restart markers
included, EOI not); segments: int32 offsets inside the scan of each restart segment's first byte (one zero without an interval)."""

FRAME_DTYPE = np.dtype([('scan_offset', '<i8'), ('scan_bytes', '<i4'), ('restart_interval', '<i4'), ('first_segment', '<i4'),
                        ('n_segments', '<i4'), ('qtab', '<i4', 3), ('dctab', '<i4', 3), ('actab', '<i4', 3), ('reserved', '<i4')])
assert FRAME_DTYPE.itemsize == C.sizeof(_lib.SagenJpegFrame) == 64
HUFF_SPEC = 272
MAX_DIM = 16384

_SOF_NAMES = {0xC1: 'extended sequential DCT', 0xC2: 'progressive DCT', 0xC3: 'lossless', 0xC5: 'differential sequential DCT',
              0xC6: 'differential progressive DCT', 0xC7: 'differential lossless', 0xC9: 'arithmetic coding', 0xCA: 'arithmetic coding',
              0xCB: 'arithmetic coding', 0xCD: 'arithmetic coding', 0xCE: 'arithmetic coding', 0xCF: 'arithmetic coding'}


class JpegFallbackWarning(UserWarning):
    """A file outside the device decoder's scope was decoded on the host."""


class JpegUnsupported(Exception):
    """A JPEG file outside what the device decodes; .reason says why."""

    def __init__(self, reason):
        Exception.__init__(self, reason)
        self.reason = reason


def _be16(data, pos):
    return (data[pos] << 8) | data[pos + 1]


def parse(data):
    """The marker walk: SOI, APPn, DQT, DHT, SOF0, DRI, SOS; restart markers and the end of the scan from one vectorised search."""
    data = bytes(data)
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError('not a JPEG file (no SOI marker)')
    qt, dc, ac = {}, {}, {}
    sof, restart, adobe = None, 0, None
    pos, n = 2, len(data)
    while True:
        if pos + 4 > n:
            raise ValueError('JPEG file ends before a scan')
        if data[pos] != 0xFF:
            raise ValueError('JPEG file: no marker at byte %d' % pos)
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise ValueError('JPEG file ends inside a marker')
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise ValueError('JPEG file ends before a scan')
        if pos + 2 > n:
            raise ValueError('JPEG file ends inside a marker segment')
        length = _be16(data, pos)
        if length < 2 or pos + length > n:
            raise ValueError('JPEG file: marker segment of %d bytes at byte %d' % (length, pos))
        body = data[pos + 2:pos + length]
        if m in _SOF_NAMES:
            raise JpegUnsupported(_SOF_NAMES[m])
        if m == 0xC0:
            if sof is not None or len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError('JPEG file: bad frame header')
            if body[0] != 8:
                raise JpegUnsupported('%d-bit samples' % body[0])
            sof = (_be16(body, 1), _be16(body, 3), [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])])
        elif m == 0xC4:
            i = 0
            while i < len(body):
                if i + 17 > len(body):
                    raise ValueError('JPEG file: bad Huffman table')
                counts = body[i + 1:i + 17]
                total = sum(counts)
                if total > 256 or i + 17 + total > len(body) or (body[i] & 15) > 3 or (body[i] >> 4) > 1:
                    raise ValueError('JPEG file: bad Huffman table')
                (ac if body[i] >> 4 else dc)[body[i] & 15] = counts + body[i + 17:i + 17 + total] + bytes(256 - total)
                i += 17 + total
        elif m == 0xDB:
            i = 0
            while i < len(body):
                if body[i] >> 4:
                    raise JpegUnsupported('16-bit quantisation tables')
                if i + 65 > len(body) or (body[i] & 15) > 3:
                    raise ValueError('JPEG file: bad quantisation table')
                qt[body[i] & 15] = np.frombuffer(body, np.uint8, 64, i + 1).astype(np.uint16)
                i += 65
        elif m == 0xDD:
            if len(body) != 2:
                raise ValueError('JPEG file: bad restart interval')
            restart = _be16(body, 0)
        elif m == 0xEE and len(body) >= 12 and body[:5] == b'Adobe':
            adobe = body[11]
        elif m == 0xDA:
            break
        pos += length
    if sof is None:
        raise ValueError('JPEG file: a scan before the frame header')
    height, width, comps = sof
    if len(comps) == 4:
        raise JpegUnsupported('four components (CMYK / YCCK)')
    if len(comps) not in (1, 3):
        raise JpegUnsupported('%d components' % len(comps))
    if width < 1 or height < 1:
        raise ValueError('JPEG file: an empty frame (or a height left to a DNL marker)')
    if width > MAX_DIM or height > MAX_DIM:
        raise JpegUnsupported('a dimension above %d' % MAX_DIM)
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        raise ValueError('JPEG file: bad scan header')
    if body[0] != len(comps):
        raise JpegUnsupported('more than one scan')
    ss, se, ahal = body[1 + 2 * body[0]:]
    if (ss, se, ahal) != (0, 63, 0):
        raise JpegUnsupported('a scan of part of the spectrum')
    if len(comps) == 3:
        if [c[0] for c in comps] == [ord('R'), ord('G'), ord('B')]:
            raise JpegUnsupported('component ids R, G, B (no YCbCr)')
        if adobe is not None and adobe != 1:
            raise JpegUnsupported('Adobe marker with transform %d (no YCbCr)' % adobe)
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise JpegUnsupported('sampling factors %s' % ', '.join('%dx%d' % (c[1], c[2]) for c in comps))
    else:
        hs, vs = 1, 1                                     # one component: the scan is not interleaved, whatever the factors say
    qtabs, dctabs, actabs = [], [], []
    for i, (cid, _, _, tq) in enumerate(comps):
        if body[1 + 2 * i] != cid:
            raise ValueError('JPEG file: the scan names component %d, the frame %d' % (body[1 + 2 * i], cid))
        td, ta = body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
        if tq not in qt or td not in dc or ta not in ac:
            raise ValueError('JPEG file: component %d uses a table the file does not define' % cid)
        qtabs.append(qt[tq]), dctabs.append(dc[td]), actabs.append(ac[ta])
    scan_offset = pos + length
    # the scan ends at the first FF that is followed by neither 00 (a stuffed FF), D0..D7 (a restart marker) nor FF (fill)
    a = np.frombuffer(data, np.uint8, n - scan_offset, scan_offset)
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, np.int64)
    nxt = a[ff + 1]
    ends = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    if ends.size == 0:
        raise ValueError('JPEG file: the scan does not end (truncated file)')
    scan_bytes = int(ends[0])
    if a[scan_bytes + 1] != 0xD9:
        raise JpegUnsupported('more than one scan')
    while scan_bytes > 0 and a[scan_bytes - 1] == 0xFF:    # fill bytes in front of EOI belong to the marker
        scan_bytes -= 1
    inside = ff[ff < scan_bytes]
    rst = inside[(a[inside + 1] >= 0xD0) & (a[inside + 1] <= 0xD7)]
    segments = np.concatenate([np.zeros(1, np.int64), rst + 2]).astype(np.int32)
    mcus = -(-width // (8 * hs)) * -(-height // (8 * vs))
    want = -(-mcus // restart) if restart else 1
    if segments.size != want:
        raise ValueError('JPEG file: %d restart markers, a restart interval of %d MCUs over %d MCUs needs %d' % (segments.size - 1, restart, mcus, want - 1))
    return JpegInfo(width, height, len(comps), hs, vs, qtabs, dctabs, actabs, restart, scan_offset, scan_bytes, segments)


Packed = collections.namedtuple('Packed', 'buffer bytes_at total_bytes frames_at n segments_at n_segments qtabs_at n_qtabs hufftabs_at n_hufftabs geometry')
Packed.__doc__ = """One call's host side: `buffer` (numpy uint8) holds frames | segments | qtabs | hufftabs | file bytes at the *_at offsets
(each a multiple of 16), total_bytes is padded to a multiple of 4; geometry = (width, height, components, hs, vs)."""


def _align16(x):
    return (x + 15) // 16 * 16


def pack(datas, infos, buffer_factory=None):
    """Descriptors and tables of frames of ONE geometry, tables de-duplicated, everything in one staging buffer (buffer_factory(nbytes)
    -> writable numpy uint8, e.g. the view of a pinned tensor; default: plain numpy)."""
    geometry = tuple(infos[0][:5])
    if any(tuple(i[:5]) != geometry for i in infos):
        raise ValueError('pack() takes frames of one geometry')
    qindex, hindex = {}, {}
    frames = np.zeros(len(infos), FRAME_DTYPE)
    seg_rows, offset = [], 0
    for f, (d, i) in enumerate(zip(datas, infos)):
        fr = frames[f]
        fr['scan_offset'], fr['scan_bytes'], fr['restart_interval'] = offset + i.scan_offset, i.scan_bytes, i.restart_interval
        fr['first_segment'], fr['n_segments'] = sum(r.shape[0] for r in seg_rows), i.segments.size
        seg_rows.append(np.stack([np.full(i.segments.size, f, np.int32), i.segments], 1))
        for c in range(i.components):
            fr['qtab'][c] = qindex.setdefault(i.qtabs[c].tobytes(), len(qindex))
            fr['dctab'][c] = hindex.setdefault(i.dctabs[c], len(hindex))
            fr['actab'][c] = hindex.setdefault(i.actabs[c], len(hindex))
        offset += len(d)
    total = (offset + 3) // 4 * 4
    segs = np.concatenate(seg_rows, 0)
    parts = [frames.tobytes(), segs.tobytes(), b''.join(qindex), b''.join(hindex)]     # (dicts keep insertion order: index order)
    at, size = [], 0
    for p in parts:
        at.append(size)
        size = _align16(size + len(p))
    buf = (buffer_factory or (lambda nbytes: np.zeros(nbytes, np.uint8)))(size + total)
    for a, p in zip(at, parts):
        buf[a:a + len(p)] = np.frombuffer(p, np.uint8)
    pos = size
    for d in datas:
        buf[pos:pos + len(d)] = np.frombuffer(d, np.uint8)
        pos += len(d)
    buf[pos:size + total] = 0
    return Packed(buf, size, total, at[0], len(infos), at[1], segs.shape[0], at[2], len(qindex), at[3], len(hindex), geometry)


ENTROPY = ('lane', 'split')
SPLIT_CHUNK_BYTES, SPLIT_ROUNDS = 256, 8        # entropy='split' without further word: the defaults DESIGN.md's split table names


def split_chunks(packed, chunk_bytes):
    """The chunks sagen_jpeg_decode_split cuts the call `packed` into: max(1, ceil(bytes / chunk_bytes)) per restart segment (the whole
    scan where there is no interval) - the smallest max_chunks at which no frame comes out CAPACITY."""
    frames = packed.buffer[packed.frames_at:packed.frames_at + 64 * packed.n].view(FRAME_DTYPE)
    rows = packed.buffer[packed.segments_at:packed.segments_at + 8 * packed.n_segments].view(np.int32).reshape(-1, 2)
    total = 0
    for fr in frames:
        first, count = int(fr['first_segment']), int(fr['n_segments'])
        starts = rows[first:first + count, 1].astype(np.int64)
        ends = np.concatenate([starts[1:] - 2, [int(fr['scan_bytes'])]])
        total += int(np.maximum(-(-(ends - starts) // int(chunk_bytes)), 1).sum())
    return total


def _entropy_options(entropy, chunk_bytes, rounds):
    if entropy not in ENTROPY:
        raise ValueError('entropy %r is none of %s' % (entropy, ', '.join(ENTROPY)))
    if entropy == 'lane':
        if chunk_bytes is not None or rounds is not None:
            raise ValueError("chunk_bytes and rounds belong to entropy='split'")
        return None, None
    chunk_bytes = SPLIT_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    rounds = SPLIT_ROUNDS if rounds is None else int(rounds)
    if chunk_bytes % 4 or not 16 <= chunk_bytes <= 65536:
        raise ValueError('chunk_bytes %d is no multiple of 4 in [16, 65536]' % chunk_bytes)
    if not 1 <= rounds <= 64:
        raise ValueError('rounds %d is outside [1, 64]' % rounds)
    return chunk_bytes, rounds


def decode_packed(packed, staged, out=None, entropy='lane', chunk_bytes=None, rounds=None, want_path=False, max_chunks=None):
    """sagen_jpeg_decode on `staged`, the uint8 tensor holding packed.buffer where the library reads (device memory; the host with
    the CPU twin).  Returns (out [n, h, w, 3] uint8, status [n] int32) on that device; nothing is synchronised.
    entropy='split': sagen_jpeg_decode_split with chunk_bytes bytes of scan per lane and `rounds` synchronisation passes (defaults
    SPLIT_CHUNK_BYTES, SPLIT_ROUNDS), the same out and status; want_path adds path [n] int32 (who decoded each frame) as a third
    value; max_chunks (default: split_chunks(packed, chunk_bytes), the exact count) is the capacity of the chunk tables."""
    import torch
    from .ops import _ptr, _scratch64, _stream
    l = _lib.lib()
    chunk_bytes, rounds = _entropy_options(entropy, chunk_bytes, rounds)
    if entropy == 'lane' and (want_path or max_chunks is not None):
        raise ValueError("want_path and max_chunks belong to entropy='split'")
    w, h, comps, hs, vs = packed.geometry
    n = packed.n
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=staged.device)
    status = torch.empty(n, dtype=torch.int32, device=staged.device)
    base = staged.data_ptr()
    at = lambda off: C.c_void_p(base + off)
    if entropy == 'split':
        if max_chunks is None:
            max_chunks = split_chunks(packed, chunk_bytes)
        path = torch.empty(n, dtype=torch.int32, device=staged.device) if want_path else None
        nbytes = int(l.sagen_jpeg_decode_split_scratch_bytes(n, w, h, comps, hs, vs, packed.n_hufftabs, packed.n_segments, max_chunks))
        scratch = _scratch64(nbytes, staged.device)
        _lib.check(l.sagen_jpeg_decode_split(at(packed.bytes_at), packed.total_bytes, at(packed.frames_at), n, at(packed.segments_at),
                                             packed.n_segments, at(packed.qtabs_at), packed.n_qtabs, at(packed.hufftabs_at), packed.n_hufftabs, w, h,
                                             comps, hs, vs, _ptr(out), _ptr(status), _ptr(scratch), nbytes, _stream(), chunk_bytes, rounds, max_chunks,
                                             _ptr(path) if want_path else None))
        return (out, status, path) if want_path else (out, status)
    nbytes = int(l.sagen_jpeg_decode_scratch_bytes(n, w, h, comps, hs, vs, packed.n_hufftabs))
    scratch = _scratch64(nbytes, staged.device)
    _lib.check(l.sagen_jpeg_decode(at(packed.bytes_at), packed.total_bytes, at(packed.frames_at), n, at(packed.segments_at), packed.n_segments,
                                   at(packed.qtabs_at), packed.n_qtabs, at(packed.hufftabs_at), packed.n_hufftabs, w, h, comps, hs, vs,
                                   _ptr(out), _ptr(status), _ptr(scratch), nbytes, _stream()))
    return out, status


def status_text(code):
    return ' + '.join(name for bit, name in sorted(_lib.SAGEN_JPEG_STATUS.items()) if code & bit) or 'ok'


class JpegDecoder(object):
    """decode(items) -> uint8 [N, H, W, 3] on the device, in the order of `items` (bytes objects or paths of files).  Frames of
    several geometries (sampling, grey / colour) are decoded a group at a time; all must have one size.  `timing`, when set to a
    dict, receives 'parse' and 'pack' in host seconds of the last call.  entropy='split' decodes each restart segment - each frame of
    a file without an interval - on many lanes (sagen_jpeg_decode_split; chunk_bytes, rounds: its options, default SPLIT_CHUNK_BYTES
    and SPLIT_ROUNDS): the same pixels and the same errors.  last_paths then holds {path value: frames} of the last call (0: the split
    path; the SAGEN_JPEG_PATH_* values: decoded again by one lane per segment), read with the status that comes back anyway."""

    def __init__(self, device=None, entropy='lane', chunk_bytes=None, rounds=None):
        from .ops import default_device
        self.chunk_bytes, self.rounds = _entropy_options(entropy, chunk_bytes, rounds)
        self.entropy = entropy
        self.last_paths = {}
        self.device = default_device(device)
        self._warned = False
        self.timing = None

    def _staging(self, nbytes):
        import torch
        self._pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=self.device.type == 'cuda')
        return self._pinned.numpy()

    def decode(self, items):
        import time
        import torch
        t0 = time.perf_counter()
        names = [it if isinstance(it, str) else '<item %d>' % k for k, it in enumerate(items)]
        datas = []
        for it in items:
            if isinstance(it, str):
                with open(it, 'rb') as f:
                    datas.append(f.read())
            else:
                datas.append(bytes(it))
        groups, fallback, size = collections.OrderedDict(), [], None
        for k, d in enumerate(datas):
            try:
                info = parse(d)
                this = (info.width, info.height)
                groups.setdefault(tuple(info[:5]), []).append((k, info))
            except JpegUnsupported as e:
                if not self._warned:
                    warnings.warn('%s is decoded on the host (%s); further files of this kind are not reported' % (names[k], e.reason), JpegFallbackWarning)
                    self._warned = True
                fallback.append(k)
                this = _host_size(d)
            size = size or this
            if this != size:
                raise ValueError('%s is %dx%d, the first frame %dx%d (all frames must have one size)' % ((names[k],) + this + size))
        t1 = time.perf_counter()
        if not datas:
            return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=self.device)
        out = torch.empty((len(datas), size[1], size[0], 3), dtype=torch.uint8, device=self.device)
        pending, t_pack = [], 0.
        for members in groups.values():
            idx = [k for k, _ in members]
            tp = time.perf_counter()
            packed = pack([datas[k] for k in idx], [i for _, i in members], self._staging)
            t_pack += time.perf_counter() - tp
            staged = self._pinned.to(self.device, non_blocking=True)             # the one copy of this group
            whole = idx == list(range(len(datas)))
            if self.entropy == 'split':
                got, status, path = decode_packed(packed, staged, out if whole else None, 'split', self.chunk_bytes, self.rounds, want_path=True)
                status = torch.stack([status, path])                              # (one copy back for both)
            else:
                got, status = decode_packed(packed, staged, out if whole else None)
            if not whole:
                out[torch.as_tensor(idx, device=self.device)] = got
            pending.append((idx, status, self._pinned))                           # (the staging buffer lives until the copy has run)
        for k in fallback:
            out[k] = torch.as_tensor(_host_decode(datas[k])).to(self.device)
        self.last_paths = {}
        for idx, status, _ in pending:
            bad = status.cpu().numpy()
            if bad.ndim == 2:
                for v in bad[1].tolist():
                    self.last_paths[v] = self.last_paths.get(v, 0) + 1
                bad = bad[0]
            for j in np.flatnonzero(bad):
                raise IOError('%s: the JPEG stream is damaged (%s)' % (names[idx[j]], status_text(int(bad[j]))))
        if self.timing is not None:
            self.timing.update(parse=t1 - t0, pack=t_pack)
        return out


def _host_size(data):
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return im.size


def _host_decode(data):
    import io
    from .feeder import imread
    return np.array(imread(io.BytesIO(data)))                  # (a writable copy: PIL's buffer is read-only)


def load_frames_device(names, device=None, decoder=None):
    """[len(names), H, W, 3] uint8 on the device: what torch.as_tensor(frames.load_frames(names)).to(device) holds."""
    return (decoder or JpegDecoder(device)).decode(list(names))


# ---- encode ----------------------------------------------------------------------------------------------------------------------------
# Annex K.1 / K.2 in natural order; K.3 - K.6 as DHT holds them: 16 counts, then the symbols
_STD_Q = np.array([[16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                   [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32], np.int64)
_STD_HUFF = [bytes.fromhex(h) for h in (
    '00010501010101010100000000000000000102030405060708090a0b',
    '0002010303020403050504040000017d01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738'
    '393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3'
    'c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa',
    '00030101010101010101010000000000000102030405060708090a0b',
    '00020102040403040705040400010277000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637'
    '38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba'
    'c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')]          # DC0, AC0, DC1, AC1
_NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                     57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
SUBSAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}


def quality_tables(quality):
    """uint16 [2][64] in natural order: libjpeg's jpeg_set_quality (baseline: entries clamped to 1..255)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((_STD_Q * scale + 50) // 100, 1, 255).astype(np.uint16)


def _segment(marker, body):
    return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body


def encode_header(w, h, components, hs, vs, qtabs, restart_interval=0):
    """SOI, the JFIF APP0 PIL writes without dpi, DQT per table, SOF0, DHT per table, (DRI,) SOS: everything in front of the entropy-coded
    data.  qtabs: [2][64] in natural order; restart_interval: MCUs, 0 for none - libjpeg puts DRI directly in front of SOS."""
    if not 0 <= int(restart_interval) <= 65535:
        raise ValueError('a restart interval of %d MCUs is outside 0..65535 (what DRI can name)' % restart_interval)
    if components not in (1, 3) or (components == 1 and (hs, vs) != (1, 1)) or (hs, vs) not in SUBSAMPLING.values():
        raise ValueError('components %d with sampling %dx%d is outside baseline grey / 4:4:4 / 4:2:2 / 4:2:0' % (components, hs, vs))
    qtabs = np.asarray(qtabs)
    out = b'\xff\xd8' + _segment(0xE0, b'JFIF\0\x01\x01\0\0\x01\0\x01\0\0')
    for i in range(1 if components == 1 else 2):
        out += _segment(0xDB, bytes([i]) + qtabs[i][_NATURAL].astype(np.uint8).tobytes())
    comps = [(1, (hs << 4) | vs, 0), (2, 0x11, 1), (3, 0x11, 1)][:components]
    out += _segment(0xC0, bytes([8, h >> 8, h & 255, w >> 8, w & 255, components]) + b''.join(bytes(c) for c in comps))
    for ident, spec in zip((0x00, 0x10, 0x01, 0x11), _STD_HUFF[:2 if components == 1 else 4]):
        out += _segment(0xC4, bytes([ident]) + spec)
    if restart_interval:
        out += _segment(0xDD, bytes([int(restart_interval) >> 8, int(restart_interval) & 255]))
    return out + _segment(0xDA, bytes([components]) + b''.join(bytes([c[0], c[2] * 0x11]) for c in comps) + b'\0\x3f\0')


def restart_interval_of(w, h, components, hs, vs, restart_rows=0, restart_blocks=0):
    """The interval in MCUs as PIL's restart_marker_rows / restart_marker_blocks give it: rows win, and mean rows x MCUs per row.  An
    interval DRI cannot name is refused, not clamped."""
    if restart_rows < 0 or restart_blocks < 0:
        raise ValueError('restart_rows and restart_blocks must not be negative')
    fh, fv = (hs, vs) if components == 3 else (1, 1)
    interval = int(restart_rows) * (-(-w // (8 * fh))) if restart_rows else int(restart_blocks)
    if interval > 65535:
        raise ValueError('a restart interval of %d MCUs (%s) is above 65535, the most a DRI segment can name'
                         % (interval, 'restart_rows=%d at %d MCUs per row' % (restart_rows, -(-w // (8 * fh))) if restart_rows else 'restart_blocks'))
    return interval


def encode_streams(frames, qtabs, hs, vs, stride, out=None, restart_interval=0):
    """sagen_jpeg_encode on `frames` (uint8 [n, h, w, 3] or [n, h, w], device memory; the host with the CPU twin); qtabs uint16 [2][64] in
    natural order (host); with a restart_interval (MCUs, the caller's DRI) sagen_jpeg_encode_rst.  Returns (out [n, stride] uint8,
    sizes [n] int32, status [n] int32) on that device; nothing is synchronised."""
    import torch
    from .ops import _ptr, _scratch64, _stream
    l = _lib.lib()
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
        raise TypeError('frames must be uint8 [n, h, w, 3] (RGB) or [n, h, w] (grey)')
    frames = frames.contiguous()
    n, h, w = (int(v) for v in frames.shape[:3])
    comps = 3 if frames.dim() == 4 else 1
    dev = frames.device
    zz = torch.as_tensor(np.ascontiguousarray(np.asarray(qtabs, np.uint16)[:, _NATURAL]).view(np.int16)).to(dev)
    if out is None:
        out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if restart_interval:
        if not 0 < int(restart_interval) <= 65535:
            raise ValueError('a restart interval of %d MCUs is outside 0..65535 (what DRI can name)' % restart_interval)
        nbytes = int(l.sagen_jpeg_encode_rst_scratch_bytes(n, w, h, comps, hs, vs, int(restart_interval), stride))
        scratch = _scratch64(nbytes, dev)
        _lib.check(l.sagen_jpeg_encode_rst(_ptr(frames), n, w, h, comps, hs, vs, int(restart_interval), _ptr(zz), _ptr(out), stride, _ptr(sizes),
                                           _ptr(status), _ptr(scratch), nbytes, _stream()))
        return out, sizes, status
    nbytes = int(l.sagen_jpeg_encode_scratch_bytes(n, w, h, comps, hs, vs, stride))
    scratch = _scratch64(nbytes, dev)
    _lib.check(l.sagen_jpeg_encode(_ptr(frames), n, w, h, comps, hs, vs, _ptr(zz), _ptr(out), stride, _ptr(sizes), _ptr(status), _ptr(scratch),
                                   nbytes, _stream()))
    return out, sizes, status


class JpegEncoder(object):
    """encode(frames) -> list of complete files (bytes), one per frame: what PIL writes for the same pixels at `quality` and `subsampling`
    ('4:4:4', '4:2:2', '4:2:0'; grey frames [n, h, w] have none).  One device call per block of frames, one copy of sizes + status, one
    copy of the streams cut at the longest; a frame whose stream does not fit the stride is encoded again, alone, at the bound.
    restart_rows / restart_blocks: PIL's restart_marker_rows / restart_marker_blocks (rows win; rows x MCUs per row): the files then
    hold a DRI segment and restart markers, and the device decoder reads them with one lane per segment."""

    def __init__(self, device=None, quality=95, subsampling='4:2:0', stride=None, restart_rows=0, restart_blocks=0):
        from .ops import default_device
        _lib.lib()
        if subsampling not in SUBSAMPLING:
            raise ValueError('subsampling %r is none of %s' % (subsampling, ', '.join(sorted(SUBSAMPLING))))
        self.device = default_device(device)
        self.quality, self.subsampling, self.stride = quality, subsampling, stride
        if restart_rows < 0 or restart_blocks < 0:
            raise ValueError('restart_rows and restart_blocks must not be negative')
        self.restart_rows, self.restart_blocks = int(restart_rows), int(restart_blocks)
        self.qtabs = quality_tables(quality)

    def encode(self, frames, first=0):
        """`first`: the number of frames[0], for the message of a frame that cannot be coded."""
        import torch
        from .ops import encode_with_retry
        if not isinstance(frames, torch.Tensor) or frames.device.type != self.device.type:
            raise TypeError('frames must be a uint8 tensor on %s' % self.device)
        n = int(frames.shape[0])
        if n == 0:
            return []
        h, w = int(frames.shape[1]), int(frames.shape[2])
        comps = 3 if frames.dim() == 4 else 1
        hs, vs = SUBSAMPLING[self.subsampling] if comps == 3 else (1, 1)
        stride = self.stride if self.stride is not None else max((w * h * comps + 63) // 64 * 64, 4096)
        rst = restart_interval_of(w, h, comps, hs, vs, self.restart_rows, self.restart_blocks)
        head = encode_header(w, h, comps, hs, vs, self.qtabs, rst)
        bound = (int(_lib.lib().sagen_jpeg_encode_rst_max_bytes(w, h, comps, hs, vs, rst)) + 3) // 4 * 4

        def run(part, at):
            return encode_streams(frames[part], self.qtabs, hs, vs, at, restart_interval=rst)

        def out_of_range(f, st):
            return ValueError('frame %d: a coefficient outside what baseline JPEG can code (DC category > 11 or AC category > 10)' % (first + f))
        return encode_with_retry(run, n, stride, bound, _lib.SAGEN_JPEG_ENC_ST_CAPACITY, wrap=lambda stream, f: head + stream + b'\xff\xd9',
                                 fatal=_lib.SAGEN_JPEG_ENC_ST_RANGE, fatal_error=out_of_range, label=lambda f: 'frame %d' % (first + f))


# ---- re-segmenting files that exist ------------------------------------------------------------------------------------------------------
def transcode_header(data, info, restart_interval):
    """The header of `data` (SOI .. SOS) for its re-coded scan: the file's own segments in their order, each DHT replaced by the standard
    tables (the four of Annex K, two for grey, where the first DHT stood), any DRI dropped, the new one directly in front of SOS, and
    the scan header naming tables 0 for luma and 1 for chroma."""
    out, pos, tables = b'\xff\xd8', 2, False
    while True:
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        length = _be16(data, pos)
        body = data[pos + 2:pos + length]
        pos += length
        if m == 0xC4:
            if not tables:
                for ident, spec in zip((0x00, 0x10, 0x01, 0x11), _STD_HUFF[:2 if info.components == 1 else 4]):
                    out += _segment(0xC4, bytes([ident]) + spec)
            tables = True
        elif m == 0xDA:
            if restart_interval:
                out += _segment(0xDD, bytes([restart_interval >> 8, restart_interval & 255]))
            sel = b''.join(bytes([body[1 + 2 * i], 0x11 if i else 0x00]) for i in range(info.components))
            return out + _segment(0xDA, bytes([info.components]) + sel + b'\0\x3f\0')
        elif m != 0xDD:
            out += _segment(m, body)


def transcode_streams(packed, staged, restart_interval, stride):
    """sagen_jpeg_transcode on `staged`, the uint8 tensor holding packed.buffer where the library reads.  Returns (out [n, stride] uint8,
    sizes [n] int32, status [n] int32) on that device; nothing is synchronised."""
    import torch
    from .ops import _ptr, _scratch64, _stream
    l = _lib.lib()
    w, h, comps, hs, vs = packed.geometry
    n = packed.n
    out = torch.empty((n, stride), dtype=torch.uint8, device=staged.device)
    sizes = torch.empty(n, dtype=torch.int32, device=staged.device)
    status = torch.empty(n, dtype=torch.int32, device=staged.device)
    nbytes = int(l.sagen_jpeg_transcode_scratch_bytes(n, w, h, comps, hs, vs, packed.n_hufftabs, restart_interval, stride))
    scratch = _scratch64(nbytes, staged.device)
    at = lambda off: C.c_void_p(staged.data_ptr() + off)
    _lib.check(l.sagen_jpeg_transcode(at(packed.bytes_at), packed.total_bytes, at(packed.frames_at), n, at(packed.segments_at), packed.n_segments,
                                      at(packed.hufftabs_at), packed.n_hufftabs, w, h, comps, hs, vs, restart_interval, _ptr(out), stride,
                                      _ptr(sizes), _ptr(status), _ptr(scratch), nbytes, _stream()))
    return out, sizes, status


def transcode_status_text(code):
    enc = [name for bit, name in ((1, 'capacity'), (2, 'range')) if (code >> 8) & bit]
    return ' + '.join(([status_text(code & 255)] if code & 255 else []) + ['encode ' + e for e in enc]) or 'ok'


def transcode_files(datas, restart_rows=1, device=None, restart_blocks=0, names=None):
    """The files `datas` (bytes) with a restart interval of `restart_rows` rows of MCUs (or `restart_blocks` MCUs; rows win, as in PIL),
    re-coded on the device WITHOUT a pixel being computed: the coefficients of each written file equal those of its source
    (sagen_jpeg_transcode).  One parse per file; the header is the file's own with the standard Huffman tables and the new DRI
    (transcode_header).  A file outside the decoder's scope is passed through byte for byte, with one JpegFallbackWarning per call.
    A damaged file raises IOError."""
    import torch
    from .ops import default_device, encode_with_retry
    device = default_device(device)
    datas = [bytes(d) for d in datas]
    names = names or ['<item %d>' % k for k in range(len(datas))]
    result, groups, warned = list(datas), collections.OrderedDict(), False
    for k, d in enumerate(datas):
        try:
            info = parse(d)
            groups.setdefault(tuple(info[:5]), []).append((k, info))
        except JpegUnsupported as e:
            if not warned:
                warnings.warn('%s is passed through as it is (%s); further files of this kind are not reported' % (names[k], e.reason), JpegFallbackWarning)
                warned = True
    for geometry, members in groups.items():
        w, h, comps, hs, vs = geometry
        rst = restart_interval_of(w, h, comps, hs, vs, restart_rows, restart_blocks)
        idx, infos = [k for k, _ in members], [i for _, i in members]
        bound = (int(_lib.lib().sagen_jpeg_transcode_max_bytes(w, h, comps, hs, vs, rst)) + 3) // 4 * 4
        mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
        # the standard tables can be longer than a file's own: half as much again, the markers and their fills, and a floor
        stride = min(bound, (max(i.scan_bytes for i in infos) * 3 // 2 + 4 * mcus + 4096 + 63) // 64 * 64)

        def run(part, at):
            packed = pack([datas[k] for k in idx[part]], infos[part])
            return transcode_streams(packed, torch.as_tensor(packed.buffer).to(device), rst, at)

        def wrap(stream, j):
            return transcode_header(datas[idx[j]], infos[j], rst) + stream + b'\xff\xd9'

        def damaged(j, st):
            return IOError('%s: the JPEG stream cannot be re-segmented (%s)' % (names[idx[j]], transcode_status_text(st)))
        capacity = _lib.SAGEN_JPEG_ENC_ST_CAPACITY << 8                         # by itself: with any other bit the file is damaged
        done = encode_with_retry(run, len(idx), stride, bound, capacity, wrap, fatal=~capacity, fatal_error=damaged, label=lambda j: names[idx[j]])
        for j, k in enumerate(idx):
            result[k] = done[j]
    return result


def main(argv=None):
    """python -m spatialaudiogen_amd.jpeg restart IN_DIR OUT_DIR [--rows 1 | --blocks N] [--block 256] [--overwrite]"""
    import argparse
    import os
    parser = argparse.ArgumentParser(prog='python -m spatialaudiogen_amd.jpeg', description='Tools around the JPEG frames of a clip folder.')
    sub = parser.add_subparsers(dest='command', required=True)
    p = sub.add_parser('restart', help='give the .jpg files of a folder a restart interval, losslessly (the coefficients stay; the device decoder '
                                       'then reads each frame with one lane per segment)')
    p.add_argument('in_dir', help='folder of .jpg files')
    p.add_argument('out_dir', help='folder for the re-segmented files, same names')
    which = p.add_mutually_exclusive_group()
    which.add_argument('--rows', type=int, default=None, help='rows of MCUs per restart interval (default 1)')
    which.add_argument('--blocks', type=int, default=None, help='MCUs per restart interval')
    p.add_argument('--block', type=int, default=256, help='files per device call')
    p.add_argument('--overwrite', action='store_true', help='Whether to replace .jpg files already in the output folder.')
    p.add_argument('--gpu', type=int, default=0, help='GPU id')
    args = parser.parse_args(argv)
    rows, blocks = (0, args.blocks) if args.blocks is not None else (1 if args.rows is None else args.rows, 0)
    if rows < 0 or blocks < 0 or (rows == 0 and blocks == 0):
        raise SystemExit('jpeg restart: --rows and --blocks take a positive number')
    if args.block < 1:
        raise SystemExit('jpeg restart: --block takes a positive value')
    if not os.path.isdir(args.in_dir):
        raise SystemExit('jpeg restart: %s is not a folder' % args.in_dir)
    files = sorted(f for f in os.listdir(args.in_dir) if f.lower().endswith(('.jpg', '.jpeg')))
    if not files:
        raise SystemExit('jpeg restart: %s holds no .jpg file' % args.in_dir)
    if os.path.abspath(args.in_dir) == os.path.abspath(args.out_dir):
        raise SystemExit('jpeg restart: the output folder is the input folder')
    held = [f for f in os.listdir(args.out_dir) if f.lower().endswith(('.jpg', '.jpeg'))] if os.path.isdir(args.out_dir) else []
    if held and not args.overwrite:
        raise SystemExit('jpeg restart: %s already holds frames (--overwrite)' % args.out_dir)
    from .ops import select_device
    select_device(args.gpu)
    for f in held:
        os.remove(os.path.join(args.out_dir, f))
    os.makedirs(args.out_dir, exist_ok=True)
    before = after = 0
    for i in range(0, len(files), args.block):
        part = files[i:i + args.block]
        datas = []
        for f in part:
            with open(os.path.join(args.in_dir, f), 'rb') as fh:
                datas.append(fh.read())
        try:
            done = transcode_files(datas, rows, None, blocks, [os.path.join(args.in_dir, f) for f in part])
        except (ValueError, IOError) as e:
            raise SystemExit('jpeg restart: %s' % e)
        for f, d in zip(part, done):
            with open(os.path.join(args.out_dir, f), 'wb') as fh:
                fh.write(d)
        before, after = before + sum(len(d) for d in datas), after + sum(len(d) for d in done)
    print('wrote %d files to %s: %d bytes before, %d after (%+.2f %%)' % (len(files), args.out_dir, before, after, 100. * (after - before) / before))


if __name__ == '__main__':
    main()
