"""Frames in a folder: %06d.jpg (or .png) from 000000 on.  What overlay, project, flow and deploy --overlay_dir share: listing and checking
the input folder, clearing the output folder, reading a block of frames onto the device (PIL on the host, or jpeg.JpegDecoder), writing
a block from the device (PIL on the host, or jpeg.JpegEncoder / png.PngEncoder), and the command-line options that choose among these.

    names = frame_names(folder); check_frame_sizes(names, tool); w, h = frame_size(names[0])
    prepare_output_dir(out_dir, overwrite, tool, ...)          the last refusal: what it does not refuse it clears
    FrameReader(device, decode).read(names)                    -> uint8 [n, h, w, 3] on the device
    FrameWriter(out_dir, fmt, encode, device, restart_rows).write(frames, first)

(The feeder lists a training clip's folder in sorted order instead: another contract, feeder.py.)
"""
import os

import numpy as np


def frame_names(folder):
    """The %06d.jpg frames of a folder from 000000 on, in order."""
    names = []
    while os.path.exists(os.path.join(folder, '%06d.jpg' % len(names))):
        names.append(os.path.join(folder, '%06d.jpg' % len(names)))
    return names


def frame_size(name):
    """(width, height) from the file's header alone."""
    from PIL import Image
    with Image.open(name) as im:
        return im.size


def check_frame_sizes(names, tool):
    """Refuse frames of differing sizes from the files' headers alone (nothing is decoded)."""
    first = None
    for n in names:
        size = frame_size(n)
        first = first or size
        if size != first:
            raise SystemExit('%s: %s is %dx%d, the first frame %dx%d (all frames must have one size)' % ((tool, n) + size + first))


def load_frames(names):
    from .feeder import imread
    return np.stack([imread(n) for n in names], 0)


def prepare_output_dir(out_dir, overwrite, tool, extensions=('.png',), extras=(), refuse_any=False):
    """Refuses, without --overwrite, a folder that holds frames (files ending in one of `extensions`, or named in `extras`) - with
    refuse_any a folder that holds anything; otherwise removes those files, leaves every other one, and makes the folder."""
    listing = os.listdir(out_dir) if os.path.isdir(out_dir) else []
    held = [f for f in listing if f.endswith(tuple(extensions)) or f in extras]
    if refuse_any and listing and not overwrite:
        raise SystemExit('%s: %s is not empty (--overwrite)' % (tool, out_dir))
    if held and not overwrite:
        raise SystemExit('%s: %s already holds frames (--overwrite)' % (tool, out_dir))
    for f in held:
        os.remove(os.path.join(out_dir, f))
    os.makedirs(out_dir, exist_ok=True)


class FrameReader(object):
    """read(names) -> uint8 [n, h, w, 3] on `device`.  decode 'host': PIL, one thread, then one copy; 'device': the files' bytes go to the
    device and jpeg.JpegDecoder decodes them there; the same pixels.  entropy ('device' only): 'lane', one lane per restart segment, or
    'split', many lanes per segment (jpeg.JpegDecoder)."""

    def __init__(self, device, decode='host', entropy='lane'):
        self.device, self.decoder = device, None
        check_entropy(None, decode, entropy)
        if decode == 'device':
            from .jpeg import JpegDecoder
            self.decoder = JpegDecoder(device, entropy=entropy)

    def read(self, names):
        import torch
        if self.decoder is not None:
            return self.decoder.decode(names)
        return torch.as_tensor(load_frames(names)).to(self.device)


class FrameWriter(object):
    """write(frames, first): frames (uint8 [n, h, w, 3] on the device) -> out_dir/%06d.<fmt> from number `first` on.  encode 'host': the raw
    frames come back and PIL writes them, png, or jpg at quality 95 (4:2:0); 'device': jpeg.JpegEncoder (the same files) or png.PngEncoder
    (other bytes, the same pixels) on `device`, and only the files' bytes come back.  restart_rows (jpg only): rows of MCUs per restart
    interval, PIL's restart_marker_rows; 0: none.  Nothing is loaded before the first write, so the refusals here cost nothing."""

    def __init__(self, out_dir, fmt, encode='host', device=None, restart_rows=0):
        if restart_rows < 0 or (restart_rows and fmt != 'jpg'):
            raise ValueError('restart_rows takes 0 or a positive number of MCU rows and belongs to jpg (restart_rows=%d fmt=%s)' % (restart_rows, fmt))
        self.out_dir, self.fmt, self.encode, self.device, self.restart_rows = out_dir, fmt, encode, device, int(restart_rows)
        self._encoder = None

    @property
    def encoder(self):
        """The device encoder of encode='device' (made on first use), None on the host path."""
        if self._encoder is None and self.encode == 'device':
            if self.fmt == 'jpg':
                from .jpeg import JpegEncoder
                self._encoder = JpegEncoder(self.device, restart_rows=self.restart_rows)     # quality 95, 4:2:0: what the host path writes
            else:
                from .png import PngEncoder
                self._encoder = PngEncoder(self.device)
        return self._encoder

    def write_files(self, datas, first=0):
        """datas: complete files (bytes), as an encoder returns them."""
        for i, data in enumerate(datas):
            with open(os.path.join(self.out_dir, '%06d.%s' % (first + i, self.fmt)), 'wb') as f:
                f.write(data)

    def write(self, frames, first=0):
        if self.encode == 'device':
            return self.write_files(self.encoder.encode(frames, first), first)
        from PIL import Image
        extra = dict(quality=95) if self.fmt == 'jpg' else {}
        if self.restart_rows:
            extra['restart_marker_rows'] = self.restart_rows
        for i, f in enumerate(frames.cpu().numpy()):
            Image.fromarray(f).save(os.path.join(self.out_dir, '%06d.%s' % (first + i, self.fmt)), **extra)


# ---- command line ---------------------------------------------------------------------------------------------------------------
DECODE_HELP = "where the input frames are decoded: host (PIL, one thread) or device (jpeg.py: the files' bytes go to the device; same pixels)"

ENCODE_HELP = ("where the output frames are encoded (--format jpg only): host (PIL, one thread, after the raw frames came back) or device "
               "(jpeg.py: only the files' bytes leave the device; the same files).  Measured on one MI355X, 224x448 at quality 95 (profiles/jpeg_encode_rate.jsonl): host 2 949 frames/s; device 44 575 in blocks of 16, "
               "91 255 in blocks of 64, 111 778 in blocks of 256: it pays from --block 16, the smallest measured, up.")

ENTROPY_HELP = ("how --decode device reads a frame's entropy-coded data: lane (one lane per restart segment: one per frame for a file without "
                "restart markers, which is every file ffmpeg or PIL writes by default) or split (many lanes per segment, which find their "
                "places in the stream by themselves; the same pixels and the same errors).  Refused with --decode host.")

RESTART_HELP = ("rows of MCUs (16 pixel rows at 4:2:0) per restart interval of the jpg files written, 0: none (--format jpg only).  The device "
                "decoder (--decode device) runs one lane per restart segment, so it reads such a folder in parallel inside each frame; every "
                "other reader sees the same pixels.  The same files with --encode host (PIL's restart_marker_rows) and --encode device.")


def add_frame_arguments(parser, block, encode_help=ENCODE_HELP, restart_rows=False, block_help='frames per device call',
                        overwrite_help='Whether to replace frames already in the output folder.'):
    parser.add_argument('--overwrite', action='store_true', help=overwrite_help)
    parser.add_argument('--gpu', type=int, default=0, help='GPU id')
    parser.add_argument('--block', type=int, default=block, help=block_help)
    parser.add_argument('--decode', default='host', choices=['host', 'device'], help=DECODE_HELP)
    parser.add_argument('--entropy', default='lane', choices=['lane', 'split'], help=ENTROPY_HELP)
    parser.add_argument('--encode', default='host', choices=['host', 'device'], help=encode_help)
    if restart_rows:
        parser.add_argument('--restart_rows', type=int, default=0, metavar='N', help=RESTART_HELP)


def check_entropy(tool, decode, entropy):
    """the refusals of --entropy, in front of any file (tool None: the same as ValueError, for the classes)"""
    problem = None
    if entropy not in ('lane', 'split'):
        problem = "entropy must be 'lane' or 'split', not %r" % (entropy,)
    elif entropy != 'lane' and decode != 'device':
        problem = '--entropy %s belongs to --decode device (--decode %s decodes with PIL)' % (entropy, decode)
    if problem and tool is None:
        raise ValueError(problem)
    if problem:
        raise SystemExit('%s: %s' % (tool, problem))


def check_restart_rows(tool, restart_rows, fmt, w):
    """the refusals of --restart_rows, in front of any file: negative, png, or an interval DRI cannot name (16 x 16 MCUs: 4:2:0)"""
    if restart_rows < 0:
        raise SystemExit('%s: --restart_rows takes 0 or a positive number of MCU rows' % tool)
    if restart_rows and fmt != 'jpg':
        raise SystemExit('%s: --restart_rows belongs to --format jpg (--format %s)' % (tool, fmt))
    if restart_rows * (-(-w // 16)) > 65535:
        raise SystemExit('%s: --restart_rows %d at %d MCUs per row is an interval above 65535 MCUs, the most a JPEG file can name'
                         % (tool, restart_rows, -(-w // 16)))
