"""Estimate dense optical flow on the device and write the flow folder of a clip.

    python -m spatialaudiogen_amd.flow VIDEO_DIR FLOW_DIR [--levels L] [--warps W] [--iters I] [--alpha A] [--no_wrap] [--block 64]
        [--format {jpg,png}] [--encode {host,device}] [--restart_rows N] [--overwrite]

VIDEO_DIR holds the frames %06d.jpg (what `python -m spatialaudiogen_amd.project ... --size 224 448` writes); FLOW_DIR receives
%06d.jpg (or .png) and flow_limits.npy, float32 [n, 2]: the folder feeder.FlowFrames decodes and the flow encoder reads.  Frame k
holds the flow from frame k - 1 to frame k; frame 0 is paired with itself, so its flow is zero (scraping/preprocess.py:176-181).

What is computed (include/sagen.h: sagen_optical_flow, sagen_flow_encode; csrc/flow_core.h, csrc/flow.hip): a pyramidal
Horn-Schunck flow with warping that treats the frame as closed in x (the equirectangular seam), stored in the reference's polar
byte coding (scraping/preprocess.py:183-196).  The reference makes this folder offline with FlowNet2 under caffe; this is a
classical estimator of our own, so a checkpoint trained on FlowNet2 flows sees another estimator here, while a model trained on
these flows sees the same ones at deploy time.
"""
import os

import numpy as np


def auto_levels(h, w, want=5):
    """The largest pyramid depth <= want that halves h and w exactly and leaves at least 4 pixels of each on the coarsest level."""
    best = 1
    for levels in range(1, int(want) + 1):
        k = 1 << (levels - 1)
        if h % k == 0 and w % k == 0 and h // k >= 4 and w // k >= 4:
            best = levels
    return best


class FlowParams(object):
    """The estimator's parameters (sagen_flow_params).  levels None: auto_levels of the frames, at most 5."""

    def __init__(self, levels=None, warps=3, iters=30, alpha=8., wrap=True, fuse=0):
        if levels is not None and not 1 <= int(levels) <= 8:
            raise ValueError('levels takes 1..8, got %r' % (levels,))
        if not 1 <= int(warps) <= 16:
            raise ValueError('warps takes 1..16, got %r' % (warps,))
        if not 1 <= int(iters) <= 1000:
            raise ValueError('iters takes 1..1000, got %r' % (iters,))
        if not (np.isfinite(float(alpha)) and float(alpha) > 0.):
            raise ValueError('alpha must be positive and finite, got %r' % (alpha,))
        if not 0 <= int(fuse) <= 8:
            raise ValueError('fuse takes 0..8 (0: the library chooses), got %r' % (fuse,))
        self.levels = None if levels is None else int(levels)
        self.warps, self.iters, self.alpha, self.wrap, self.fuse = int(warps), int(iters), float(alpha), bool(wrap), int(fuse)

    def levels_for(self, h, w):
        levels = self.levels if self.levels is not None else auto_levels(h, w)
        k = 1 << (levels - 1)
        if h % k or w % k:
            raise ValueError('frames of %dx%d cannot be halved %d times (levels %d)' % (h, w, levels - 1, levels))
        if h // k < 4 or w // k < 4:
            raise ValueError('levels %d leaves fewer than 4 pixels of a %dx%d frame' % (levels, h, w))
        if h > 4096 or w > 4096:
            raise ValueError('frames of at most 4096 pixels a side, got %dx%d' % (h, w))
        return levels

    def struct(self, h, w):
        from . import _lib
        return _lib.SagenFlowParams(self.levels_for(h, w), self.warps, self.iters, int(self.wrap), self.fuse, self.alpha)


def block_ranges(n, block):
    """[(first, stop)] of the frames each device call reads: blocks of `block` new frames, each but the first preceded by the last
    frame of the block before it (the overlap of one)."""
    if block < 1:
        raise ValueError('block takes a positive value')
    return [(max(i - 1, 0), min(i + block, n)) for i in range(0, n, block)]


class FlowEstimator(object):
    """process(frames [n, h, w, 3] uint8 on the device, prev=None) -> [n, h, w, 2] float32 on the device: one flow per frame of the
    block, each against the frame before it.  prev [h, w, 3]: the last frame of the block before; None: the first frame is paired
    with itself, whose flow is exactly zero.  Nothing is kept between calls."""

    def __init__(self, params=None, device=None):
        from . import ops
        self.params = params if params is not None else FlowParams()
        self.device = ops.default_device(device)

    def process(self, frames, prev=None):
        import torch
        from . import ops
        if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
            raise ValueError('process() takes uint8 [n, h, w, 3] RGB frames')
        n, h, w = frames.shape[:3]
        if n == 0:
            return torch.empty((0, h, w, 2), dtype=torch.float32, device=frames.device)
        if prev is not None and not (isinstance(prev, torch.Tensor) and prev.dtype == torch.uint8 and tuple(prev.shape) == (h, w, 3)):
            raise ValueError('prev is the uint8 [h, w, 3] frame before the block')
        first = frames[:1] if prev is None else prev[None].to(frames.device)
        return ops.optical_flow(torch.cat([first, frames], 0), self.params.struct(h, w))


def write_flow_folder(video_dir, flow_dir, params=None, block=64, fmt='jpg', device=None, decode='host', encode='host', restart_rows=0,
                      entropy='lane'):
    """Flow folder of the frames %06d.jpg of video_dir: flow_dir/%06d.<fmt> + flow_dir/flow_limits.npy.  Returns (n, h, w, levels).
    decode 'device': the frames are decoded on the device (jpeg.load_frames_device) instead of by PIL on the host; same pixels.
    encode 'device' (jpg only): the flow frames are encoded on the device (jpeg.JpegEncoder) instead of by PIL on the host; same files.
    restart_rows (jpg only): rows of MCUs per restart interval of the files written, 0 for none; same files either way.
    entropy (decode 'device' only): 'lane' or 'split', frames.FrameReader's option; same pixels."""
    if encode == 'device' and fmt != 'jpg':
        raise ValueError('encode=device writes jpg only (fmt=%s)' % fmt)
    from . import frames as F, ops
    writer = F.FrameWriter(flow_dir, fmt, encode, device, restart_rows)       # (its refusals; nothing is loaded or written yet)
    params = params if params is not None else FlowParams()
    names = F.frame_names(video_dir)
    if not names:
        raise ValueError('%s holds no frame 000000.jpg' % video_dir)
    est = FlowEstimator(params, device)
    reader = F.FrameReader(est.device, decode, entropy)
    limits, prev, hw = [], None, None
    for first, stop in block_ranges(len(names), block):
        start = first if prev is None else first + 1
        frames = reader.read(names[start:stop])
        rgb, lim = ops.flow_encode(est.process(frames, prev))
        writer.write(rgb, start)
        limits.append(lim.cpu().numpy())
        prev, hw = frames[-1], tuple(frames.shape[1:3])
    np.save(os.path.join(flow_dir, 'flow_limits.npy'), np.concatenate(limits, 0).astype(np.float32))
    return len(names), hw[0], hw[1], params.levels_for(*hw)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def parse_arguments(argv=None):
    import argparse
    from .frames import add_frame_arguments
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('video_dir', help='Folder of the frames %%06d.jpg.')
    parser.add_argument('flow_dir', help='Folder for the flow frames and flow_limits.npy.')
    parser.add_argument('--levels', type=int, default=None, help='pyramid levels, 1..8 (default: as many as the frame size allows, at most 5)')
    parser.add_argument('--warps', type=int, default=3, help='warps per level')
    parser.add_argument('--iters', type=int, default=30, help='Jacobi iterations per warp')
    parser.add_argument('--alpha', type=float, default=8., help='smoothness weight, in levels of 0..255')
    parser.add_argument('--no_wrap', action='store_true', help='the frames do not close on themselves in x (not equirectangular)')
    parser.add_argument('--format', default='jpg', choices=['jpg', 'png'], help='jpg (quality 95: what the feeder reads) or png (lossless)')
    add_frame_arguments(parser, block=64, restart_rows=True, block_help='new frames per device call',
                        overwrite_help='Whether to replace a flow folder that is not empty.')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_arguments(argv)
    from . import frames as F
    if args.encode == 'device' and args.format != 'jpg':
        raise SystemExit('flow: --encode device writes jpg only (--format %s)' % args.format)
    if args.block < 1:
        raise SystemExit('flow: --block takes a positive value')
    F.check_entropy('flow', args.decode, args.entropy)
    if not os.path.isdir(args.video_dir):
        raise SystemExit('flow: %s is not a folder' % args.video_dir)
    names = F.frame_names(args.video_dir)
    if not names:
        raise SystemExit('flow: %s holds no frame 000000.jpg' % args.video_dir)
    F.check_frame_sizes(names, 'flow')
    w, h = F.frame_size(names[0])
    try:
        params = FlowParams(args.levels, args.warps, args.iters, args.alpha, not args.no_wrap)
        levels = params.levels_for(h, w)
    except ValueError as e:
        raise SystemExit('flow: %s' % e)
    F.check_restart_rows('flow', args.restart_rows, args.format, w)
    F.prepare_output_dir(args.flow_dir, args.overwrite, 'flow', ('.png', '.jpg'), extras=('flow_limits.npy',), refuse_any=True)   # every refusal is behind us
    from . import ops
    ops.select_device(args.gpu)
    n, h, w, levels = write_flow_folder(args.video_dir, args.flow_dir, params, args.block, args.format, decode=args.decode, encode=args.encode,
                                          restart_rows=args.restart_rows, entropy=args.entropy)
    print('wrote %d flow frames of %dx%d to %s (levels %d, warps %d, iters %d)' % (n, h, w, args.flow_dir, levels, params.warps, params.iters))


if __name__ == '__main__':
    main()
