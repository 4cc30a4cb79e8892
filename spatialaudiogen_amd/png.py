"""PNG frames encoded on the device: what overlay and deploy --overlay_dir write, without the raw copy and without the host's zlib.

The reference muxes lossless frames (myutils.gen_360video, myutils.py:246-279); the overlay writers here called Image.save per frame, one
host thread.  This module is the device path (include/sagen.h: sagen_png_filter, sagen_deflate; csrc/png.hip):

    rows = filter_rows(frames)              [n, h, 1 + w c] uint8: per row the filter's number and the filtered bytes
    out, sizes, status = deflate(rows)      one zlib stream per frame: per-block Huffman codes and runs at distance 1
    png_file(w, h, c, stream)               signature, IHDR, one IDAT, IEND; the chunk CRCs are zlib.crc32 on the host

8 bit, RGB or grey, no interlace.  The files' bytes differ from PIL's; every file decodes to the pixels it was given.
frames.FrameWriter(out_dir, 'png', encode='device') puts the files of PngEncoder into a folder.
"""
import struct
import zlib

from . import _lib

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def filter_rows(frames):
    """sagen_png_filter on `frames` (uint8 [n, h, w, 3] or [n, h, w], device memory; the host with the CPU twin) -> [n, h, 1 + w c]."""
    import torch
    from .ops import _ptr, _stream
    l = _lib.lib()
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
        raise TypeError('frames must be a uint8 tensor [n, h, w, 3] (RGB) or [n, h, w] (grey)')
    frames = frames.contiguous()
    n, h, w = (int(v) for v in frames.shape[:3])
    comps = 3 if frames.dim() == 4 else 1
    rows = torch.empty((n, h, 1 + w * comps), dtype=torch.uint8, device=frames.device)
    _lib.check(l.sagen_png_filter(_ptr(frames), n, w, h, comps, _ptr(rows), _stream()))
    return rows


def max_bytes(length):
    """The stride that can never be too small for strings of `length` bytes, up to a multiple of 4."""
    return (int(_lib.lib().sagen_deflate_max_bytes(int(length))) + 3) // 4 * 4


def deflate(rows, stride=None, out=None):
    """sagen_deflate on `rows` (uint8 [n, ...], device memory; the host with the CPU twin): everything behind the first axis is one byte
    string.  Returns (out [n, stride] uint8, sizes [n] int32, status [n] int32) on that device; nothing is synchronised.  stride: None
    for the bound."""
    import torch
    from .ops import _ptr, _scratch64, _stream
    l = _lib.lib()
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8 or rows.dim() < 1:
        raise TypeError('rows must be a uint8 tensor [n, ...]')
    rows = rows.contiguous()
    n = int(rows.shape[0])
    length = int(rows.numel() // n) if n else 0
    if stride is None:
        stride = max_bytes(length)
    dev = rows.device
    if out is None:
        out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    nbytes = int(l.sagen_deflate_scratch_bytes(n, length, stride))
    scratch = _scratch64(nbytes, dev)
    _lib.check(l.sagen_deflate(_ptr(rows) if length else None, n, length, _ptr(out), stride, _ptr(sizes), _ptr(status), _ptr(scratch), nbytes,
                               _stream()))
    return out, sizes, status


def _chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xffffffff)


def png_file(w, h, components, zstream):
    """The file around one zlib stream: 57 bytes of framing."""
    if components not in (1, 3):
        raise ValueError('components must be 1 (grey) or 3 (RGB)')
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 2 if components == 3 else 0, 0, 0, 0)
    return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', bytes(zstream)) + _chunk(b'IEND', b'')


class PngEncoder(object):
    """encode(frames) -> list of complete files (bytes), one per frame.  One device call per block of frames, one copy of sizes + status,
    one copy of the streams cut at the longest; a frame whose stream does not fit the stride is encoded again, alone, at the bound.
    stride: bytes per frame of the streams' buffer; None: the bound, which no frame exceeds (the copy to the host is cut at the longest
    stream either way)."""

    def __init__(self, device=None, stride=None):
        from .ops import default_device
        self.device = default_device(device)
        self.stride = stride

    def encode(self, frames, first=0):
        """`first`: the number of frames[0], for the message of a frame that cannot be coded."""
        import torch
        from .ops import encode_with_retry
        if not isinstance(frames, torch.Tensor) or frames.device.type != self.device.type:
            raise TypeError('frames must be a uint8 tensor on %s' % self.device)
        n = int(frames.shape[0])
        if n == 0:
            return []
        rows = filter_rows(frames)
        h, w = int(frames.shape[1]), int(frames.shape[2])
        comps = 3 if frames.dim() == 4 else 1
        bound = max_bytes(h * (1 + w * comps))
        return encode_with_retry(lambda part, at: deflate(rows[part], at), n, self.stride if self.stride is not None else bound, bound,
                                 _lib.SAGEN_DEFLATE_ST_CAPACITY, wrap=lambda stream, f: png_file(w, h, comps, stream), label=lambda f: 'frame %d' % (first + f))
