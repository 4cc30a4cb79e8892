"""Reproject 360-degree frames on the device: equirectangular, 3x2 cube maps, YouTube's equi-angular cube map (EAC), top-bottom
stereo, and the pinhole view of a listener who turns their head.

    python -m spatialaudiogen_amd.project IN_DIR OUT_DIR --from {er,er_tb,cube,eac,eac_stereo} --to {er,cube,eac,view} --size H W
        [--hfov DEG] [--yaw DEG ..] [--pitch DEG ..] [--roll DEG ..] [--supersample S] [--format {jpg,png}] [--encode {host,device}] [--restart_rows N] [--overwrite]

IN_DIR holds the frames %06d.jpg; OUT_DIR receives %06d.jpg (or .png).  `--from eac --to er --size 224 448` turns an EAC clip into
the video folder deploy and the feeder read.  `--to view --hfov 90 --yaw 0 90` writes what a listener sees whose head turns from 0
to 90 degrees over the clip: the same angles given to render's head trajectory yield the matching sound.

What is computed (include/sagen.h: sagen_reproject; csrc/project_core.h, csrc/project.hip): every destination pixel is the mean
of S x S sub-samples; a sub-sample has a direction in the head frame, world = Rot . head, and the world direction is fetched
bilinearly from the source.  This replaces the reference's offline conversion: scraping/preprocess.py:37-95 (first-eye crop),
scraping/utils.py:91-144 (EAC unwarp, x / y remap tables) and the vendored vrProjector's cube <-> equirect step.

World frame (ambisonics.py): x front, y left, z up.  The 3x2 layouts, as utils.py:126-135 reads them (cells of n x n pixels):

    top row      left (+y)     front (+x)          right (-y)                     as stored
    bottom row   bottom (-z)   back (-x)           top (+z)
                 rot90(., -1)  rot90(., 1)         rot90(., -1) of the cell is vrProjector's face image

and for stereo material the first eye is the left half of the frame turned by rot90(., -1) (utils.py:122-123).
"""
import os

import numpy as np

from . import ambisonics

KIND_ER, KIND_CUBE, KIND_EAC, KIND_VIEW = 0, 1, 2, 3                 # SAGEN_PROJ_* of include/sagen.h
FACE_NAMES = ('front', 'back', 'left', 'right', 'top', 'bottom')    # faces 0..5: axis +x -x +y -y +z -z
# vrProjector's face images in the world frame (CubemapProjection.py:82-121, its y / z negated): column direction, row direction
_CANON = (((0, -1, 0), (0, 0, -1)), ((0, 1, 0), (0, 0, -1)), ((1, 0, 0), (0, 0, -1)), ((-1, 0, 0), (0, 0, -1)),
          ((0, -1, 0), (1, 0, 0)), ((0, -1, 0), (-1, 0, 0)))


def face_vectors(face, orient):
    """(axis, right, down) of face 0..5 stored with orientation 0..7: the world vectors along which the CELL's columns and rows grow
    (csrc/project_core.h: proj_face_frame).  Bit 2 mirrors the image left-right first; bits 0-1 count quarter turns, one turn
    meaning that the cell is np.rot90(image)."""
    axis = np.zeros(3)
    axis[face // 2] = -1. if face & 1 else 1.
    r, d = np.array(_CANON[face][0], np.float64), np.array(_CANON[face][1], np.float64)
    if orient & 4:
        r = -r
    for _ in range(orient & 3):
        r, d = d, -r
    return axis, r, d


def layout3x2(n, x0=0, y0=0):
    """The mono 3x2 arrangement (utils.py:126-135) with cells of n pixels at (x0, y0): [(x0, y0, n, orient)] for faces 0..5."""
    cells = {'left': (0, 0, 0), 'front': (1, 0, 0), 'right': (2, 0, 0), 'bottom': (0, 1, 1), 'back': (1, 1, 3), 'top': (2, 1, 1)}
    return [(x0 + cells[f][0] * n, y0 + cells[f][1] * n, n, cells[f][2]) for f in FACE_NAMES]


def layout3x2_stereo(n, frame_h):
    """The first eye of stereo EAC material (utils.py:122-123): eye = np.rot90(frame[:, :W / 2], -1), read as the mono 3x2.  Pixel
    (i, j) of the eye is pixel (frame_h - 1 - j, i) of the frame, so the eye's cell at column c0, row r0 is the frame's cell at
    x0 = r0, y0 = frame_h - c0 - n, and the eye's own turn adds a quarter turn to the cell's."""
    return [(y, frame_h - x - n, n, (o + 1) & 3) for x, y, n, o in layout3x2(n)]


class Projection(object):
    """What a frame holds: kind ('er', 'cube', 'eac', 'view'), the stereo arrangement, the field of view."""

    def __init__(self, kind, stereo=None, hfov_deg=None, rect=None):
        self.kind, self.stereo, self.hfov_deg, self.rect = kind, stereo, hfov_deg, rect

    def code(self):
        return {'er': KIND_ER, 'cube': KIND_CUBE, 'eac': KIND_EAC, 'view': KIND_VIEW}[self.kind]

    def image_rect(self, h, w):
        """(x0, y0, w, h) of the image inside an h x w frame (er / view)."""
        if self.rect is not None:
            return tuple(int(v) for v in self.rect)
        if self.kind == 'er' and self.stereo == 'top_bottom':            # preprocess.py:51-52: crop=in_w:in_h/2:0:0
            return (0, 0, w, h // 2)
        return (0, 0, w, h)

    def faces(self, h, w):
        """[(x0, y0, n, orient)] for faces 0..5 inside an h x w frame (cube / eac)."""
        if self.stereo:
            if h % 3 or w % 4 or h // 3 != w // 4:
                raise ValueError('a stereo 3x2 frame is 3 n x 4 n pixels (each eye 3 n x 2 n, turned), not %dx%d' % (h, w))
            return layout3x2_stereo(h // 3, h)
        if h % 2 or w % 3 or h // 2 != w // 3:
            raise ValueError('a 3x2 frame is 2 n x 3 n pixels with square faces, not %dx%d: scale the frame first' % (h, w))
        return layout3x2(h // 2)

    def check(self, h, w):
        """Raises ValueError where an h x w frame cannot hold this projection."""
        if h < 1 or w < 1:
            raise ValueError('an empty %dx%d frame' % (h, w))
        if self.kind in ('cube', 'eac'):
            self.faces(h, w)
        else:
            x0, y0, rw, rh = self.image_rect(h, w)
            if rw < 1 or rh < 1 or x0 < 0 or y0 < 0 or x0 + rw > w or y0 + rh > h:
                raise ValueError('the rectangle %s does not lie inside the %dx%d frame' % ((x0, y0, rw, rh), h, w))
        if self.kind == 'view' and not (self.hfov_deg is not None and 0. < self.hfov_deg < 180.):
            raise ValueError('a perspective view takes 0 < hfov < 180 degrees')

    def struct(self, h, w):
        """The _lib.SagenProjection of this projection in an h x w frame."""
        from . import _lib
        self.check(h, w)
        p = _lib.SagenProjection()
        p.kind = self.code()
        if self.kind in ('cube', 'eac'):
            for f, (x0, y0, n, o) in enumerate(self.faces(h, w)):
                p.face[f].x0, p.face[f].y0, p.face[f].w, p.face[f].h, p.face[f].orient = x0, y0, n, n, o
        else:
            p.x0, p.y0, p.w, p.h = self.image_rect(h, w)
            p.hfov = np.pi / 180. * self.hfov_deg if self.kind == 'view' else 0.
        return p

    def density(self, h, w):
        """Pixels per radian at the image's centre: ER W / 2 pi, cube and EAC 2 n / pi, view (W / 2) / tan(hfov / 2)."""
        if self.kind in ('cube', 'eac'):
            return 2. * self.faces(h, w)[0][2] / np.pi
        rw = self.image_rect(h, w)[2]
        if self.kind == 'view':
            return (rw / 2.) / np.tan(np.pi / 360. * self.hfov_deg)
        return rw / (2. * np.pi)

    def directions(self, h, w):
        """[h, w, 3] float64: the (unnormalised) head-frame direction of every pixel centre of an h x w frame, NaN where a pixel
        belongs to no cell - the host statement of the geometry, for checks and plots."""
        self.check(h, w)
        out = np.full((h, w, 3), np.nan)
        if self.kind in ('cube', 'eac'):
            for f, (x0, y0, n, o) in enumerate(self.faces(h, w)):
                axis, r, d = face_vectors(f, o)
                p = 2. * (np.arange(n) + 0.5) / n - 1.
                if self.kind == 'eac':
                    p = np.tan(np.pi * p / 4.)
                out[y0:y0 + n, x0:x0 + n] = axis[None, None, :] + p[None, :, None] * r[None, None, :] + p[:, None, None] * d[None, None, :]
            return out
        x0, y0, rw, rh = self.image_rect(h, w)
        xf, yf = (np.arange(rw) + 0.5) / rw, (np.arange(rh) + 0.5) / rh
        if self.kind == 'er':
            az, el = (np.pi - 2. * np.pi * xf)[None, :], (np.pi / 2. - np.pi * yf)[:, None]
            v = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], -1)
        else:
            t = np.tan(np.pi / 360. * self.hfov_deg)
            v = np.stack(np.broadcast_arrays(1., (t * (1. - 2. * xf))[None, :], (t * (float(rh) / rw) * (1. - 2. * yf))[:, None]), -1)
        out[y0:y0 + rh, x0:x0 + rw] = v
        return out


def equirect(stereo=None):
    if stereo not in (None, 'top_bottom'):
        raise ValueError("equirect: stereo is None or 'top_bottom'")
    return Projection('er', stereo=stereo)


def cubemap3x2():
    return Projection('cube')


def eac3x2(stereo=False):
    return Projection('eac', stereo='left_half_turned' if stereo else None)


def perspective(hfov_deg):
    if not 0. < float(hfov_deg) < 180.:
        raise ValueError('perspective: 0 < hfov < 180 degrees expected, got %r' % (hfov_deg,))
    return Projection('view', hfov_deg=float(hfov_deg))


def auto_supersample(src, src_shape, dst, dst_shape):
    """S = min(8, max(1, ceil(rho_src / rho_dst))), rho in pixels per radian: as many sub-samples per destination pixel and axis as
    source pixels fall into it, so that a downscale averages instead of skipping."""
    ratio = src.density(*src_shape) / dst.density(*dst_shape)
    return int(min(8, max(1, np.ceil(ratio - 1e-9))))


def view_trajectory(yaw_deg, pitch_deg=None, roll_deg=None):
    """[n, 3, 3] head rotations Rot = rotation_xyz(yaw, pitch, roll) from per-frame angles in degrees: the arguments of
    render.head_trajectory, which turns the SAME angles into the matching sound-field rotations (Rot^T)."""
    yaw = np.atleast_1d(np.asarray(yaw_deg, np.float64))
    pitch = np.zeros_like(yaw) if pitch_deg is None else np.broadcast_to(np.asarray(pitch_deg, np.float64), yaw.shape)
    roll = np.zeros_like(yaw) if roll_deg is None else np.broadcast_to(np.asarray(roll_deg, np.float64), yaw.shape)
    rad = np.pi / 180.
    return np.stack([ambisonics.rotation_xyz(y * rad, p * rad, r * rad) for y, p, r in zip(yaw, pitch, roll)], 0)


class Projector(object):
    """process(frames [n, h, w, 3] uint8 on the device, rotation=None) -> [n, H, W, 3] uint8 on the device, size = (H, W).
    rotation: None, one [3, 3] matrix or [n, 3, 3] (view_trajectory), numpy or a float64 tensor; world = Rot . head.  Nothing is
    kept between calls: a clip cut into pieces gives the frames of the whole.  supersample None: auto_supersample per source size."""

    def __init__(self, src, dst, size, supersample=None, device=None):
        if src.kind == 'view':
            raise ValueError('a perspective view cannot be a source')
        if supersample is not None and not 1 <= int(supersample) <= 8:
            raise ValueError('supersample takes 1..8')
        self.src, self.dst, self.size, self.supersample = src, dst, (int(size[0]), int(size[1])), supersample
        self.dst_struct = dst.struct(*self.size)
        from . import ops
        self.device = ops.default_device(device)

    def process(self, frames, rotation=None):
        import torch
        from . import ops
        if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
            raise ValueError('process() takes uint8 [n, h, w, 3] RGB frames')
        n, h, w = frames.shape[:3]
        S = self.supersample if self.supersample is not None else auto_supersample(self.src, (h, w), self.dst, self.size)
        rot = None
        if rotation is not None:
            rot = torch.as_tensor(np.ascontiguousarray(rotation, np.float64) if not isinstance(rotation, torch.Tensor) else rotation).to(frames.device)
            if rot.dtype != torch.float64 or tuple(rot.shape[-2:]) != (3, 3) or not (rot.dim() == 2 or (rot.dim() == 3 and rot.shape[0] in (1, n))):
                raise ValueError('rotation is a float64 [3, 3] matrix or [n, 3, 3], n = %d frames' % n)
        return ops.reproject(frames, self.src.struct(h, w), self.size, self.dst_struct, rot, S)


# ---- command line ---------------------------------------------------------------------------------------------------------------
SOURCES = {'er': lambda: equirect(), 'er_tb': lambda: equirect('top_bottom'), 'cube': cubemap3x2, 'eac': eac3x2, 'eac_stereo': lambda: eac3x2(True)}
TARGETS = {'er': equirect, 'cube': cubemap3x2, 'eac': eac3x2}


def frame_angles(values, n):
    """One angle per frame from the command line's control points: one value holds, several are spread evenly over the clip."""
    v = np.asarray(values, np.float64)
    return np.full(n, v[0]) if v.size == 1 or n < 2 else np.interp(np.arange(n) / float(n - 1), np.linspace(0., 1., v.size), v)


def parse_arguments(argv=None):
    import argparse
    from .frames import add_frame_arguments
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('input_dir', help='Folder of the frames %%06d.jpg.')
    parser.add_argument('output_dir', help='Folder for the reprojected frames.')
    parser.add_argument('--from', dest='src', required=True, choices=sorted(SOURCES), help='what the input frames hold')
    parser.add_argument('--to', dest='dst', required=True, choices=sorted(TARGETS) + ['view'], help='what to produce')
    parser.add_argument('--size', type=int, nargs=2, required=True, metavar=('H', 'W'), help='size of the output frames')
    parser.add_argument('--hfov', type=float, default=None, metavar='DEG', help='horizontal field of view of --to view')
    for name in ('yaw', 'pitch', 'roll'):
        parser.add_argument('--' + name, type=float, nargs='+', default=[0.], metavar='DEG',
                            help='head %s in degrees: one value, or control points spread evenly over the clip' % name)
    parser.add_argument('--supersample', type=int, default=None, metavar='S', help='sub-samples per pixel and axis, 1..8 (default: from the sizes)')
    parser.add_argument('--format', default='jpg', choices=['jpg', 'png'], help='jpg (quality 95: what deploy and overlay read) or png (lossless)')
    add_frame_arguments(parser, block=16, restart_rows=True)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_arguments(argv)
    from . import frames as F
    if args.encode == 'device' and args.format != 'jpg':
        raise SystemExit('project: --encode device writes jpg only (--format %s)' % args.format)
    F.check_entropy('project', args.decode, args.entropy)
    F.check_restart_rows('project', args.restart_rows, args.format, args.size[1])
    if args.dst == 'view' and args.hfov is None:
        raise SystemExit('project: --to view needs --hfov')
    if args.dst != 'view' and args.hfov is not None:
        raise SystemExit('project: --hfov belongs to --to view')
    if args.supersample is not None and not 1 <= args.supersample <= 8:
        raise SystemExit('project: --supersample takes 1..8')
    if args.block < 1:
        raise SystemExit('project: --block takes a positive value')
    if not os.path.isdir(args.input_dir):
        raise SystemExit('project: %s is not a folder' % args.input_dir)
    names = F.frame_names(args.input_dir)
    if not names:
        raise SystemExit('project: %s holds no frame 000000.jpg' % args.input_dir)
    F.check_frame_sizes(names, 'project')
    w, h = F.frame_size(names[0])
    try:
        src = SOURCES[args.src]()
        dst = perspective(args.hfov) if args.dst == 'view' else TARGETS[args.dst]()
        src.check(h, w)
        dst.check(*args.size)
    except ValueError as e:
        raise SystemExit('project: %s' % e)
    F.prepare_output_dir(args.output_dir, args.overwrite, 'project', ('.png', '.jpg'))      # every refusal is behind us
    from . import ops
    ops.select_device(args.gpu)
    n = len(names)
    turned = any(np.any(np.asarray(getattr(args, k)) != 0.) for k in ('yaw', 'pitch', 'roll'))
    rot = view_trajectory(frame_angles(args.yaw, n), frame_angles(args.pitch, n), frame_angles(args.roll, n)) if turned else None
    pr = Projector(src, dst, args.size, args.supersample)
    reader = F.FrameReader(pr.device, args.decode, args.entropy)
    writer = F.FrameWriter(args.output_dir, args.format, args.encode, pr.device, args.restart_rows)
    for i in range(0, n, args.block):
        out = pr.process(reader.read(names[i:i + args.block]), None if rot is None else rot[i:i + args.block])
        writer.write(out, i)
    S = pr.supersample or auto_supersample(src, (h, w), dst, pr.size)
    print('wrote %d frames of %dx%d to %s (%s -> %s, supersample %d)' % (n, pr.size[0], pr.size[1], args.output_dir, args.src, args.dst, S))


if __name__ == '__main__':
    main()
