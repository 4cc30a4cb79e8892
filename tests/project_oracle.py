"""fp64 numpy restatement of the frame reprojection (include/sagen.h: sagen_reproject), for tests/test_gpu_project.py and
tests/test_project_host.py.  It shares nothing with csrc/project_core.h or spatialaudiogen_amd/project.py and is built the other
way round: where the product stores, per face, a rectangle and an orientation and works with the cell's own axes, this file keeps,
per face, the INDEX GRID of the face image the way the reference assembles it (an array of frame coordinates cut, turned with
np.rot90 and handed over as vrProjector's `front`, `right`, ... images: scraping/utils.py:116-135) and works in vrProjector's
own frame (x front, y right, z down) with its own (u, v) formulas per face (CubemapProjection.py:81-121 as a source, :145-175 as a
destination).  A frame pixel is reached THROUGH the index grid, so a wrong turn in the product's table shows as a wrong pixel here.

reproject() returns the means BEFORE rounding and, for cube sources, the face-decision margin of every sample: the gap between the
two largest |components| of the unit direction (a sample this close to a cube edge may be fetched from either face)."""
import numpy as np

FACES = ('front', 'back', 'left', 'right', 'top', 'bottom')


def er(rect=None):
    return {'kind': 'er', 'rect': rect}


def view(hfov_deg):
    return {'kind': 'view', 'rect': None, 'hfov': np.pi / 180. * hfov_deg}


def cube(eac=False, stereo=False):
    return {'kind': 'eac' if eac else 'cube', 'stereo': stereo}


def face_grids(h, w, stereo):
    """name -> [n, n, 2] (frame x, frame y) of every pixel of vrProjector's face image."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    grid = np.stack([xs, ys], -1)
    if stereo:                                   # the first eye: the left half, turned clockwise
        grid = np.rot90(grid[:, :w // 2], -1)
    hs, ws = grid.shape[0] // 2, grid.shape[1] // 3
    assert hs == ws and hs * 2 == grid.shape[0] and ws * 3 == grid.shape[1], 'square cells expected'
    top, bot = grid[:hs], grid[hs:]
    return {'left': top[:, :ws], 'front': top[:, ws:2 * ws], 'right': top[:, 2 * ws:],
            'bottom': np.rot90(bot[:, :ws], -1), 'back': np.rot90(bot[:, ws:2 * ws], 1), 'top': np.rot90(bot[:, 2 * ws:], -1)}


def _to_vr(d):
    """world (x front, y left, z up) -> vrProjector (x front, y right, z down); its own inverse."""
    return d * np.array([1., -1., -1.])


def _rect(p, h, w):
    return (0, 0, w, h) if p.get('rect') is None else p['rect']


def _dst_samples(dst, h, w, S):
    """(ys, xs, dirs): frame coordinates of the P destination pixels and the head-frame directions [P, S S, 3] of their samples."""
    sub = (np.arange(S) + 0.5) / S
    if dst['kind'] in ('er', 'view'):
        x0, y0, rw, rh = _rect(dst, h, w)
        jj, ii = np.meshgrid(np.arange(rh), np.arange(rw), indexing='ij')
        xf = (ii[..., None, None] + sub[None, None, None, :]) / rw                    # [rh, rw, b, a]
        yf = (jj[..., None, None] + sub[None, None, :, None]) / rh
        xf, yf = np.broadcast_arrays(xf, yf)
        if dst['kind'] == 'er':
            az, el = np.pi - 2. * np.pi * xf, np.pi / 2. - np.pi * yf
            d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
        else:
            t = np.tan(dst['hfov'] / 2.)
            d = np.stack([np.ones_like(xf), t * (1. - 2. * xf), t * (float(rh) / rw) * (1. - 2. * yf)], -1)
        return (jj + y0).reshape(-1), (ii + x0).reshape(-1), d.reshape(rh * rw, S * S, 3)
    grids = face_grids(h, w, dst['stereo'])
    ys, xs, dirs = [], [], []
    for name in FACES:
        g = grids[name]
        n = g.shape[0]
        rows, cols = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        u = 2. * (cols[..., None, None] + sub[None, None, None, :]) / n - 1.           # along the face image's columns
        v = 2. * (rows[..., None, None] + sub[None, None, :, None]) / n - 1.
        u, v = np.broadcast_arrays(u, v)
        if dst['kind'] == 'eac':
            u, v = np.tan(np.pi * u / 4.), np.tan(np.pi * v / 4.)
        one = np.ones_like(u)
        vr = {'front': (one, u, v), 'right': (-u, one, v), 'left': (u, -one, v), 'back': (-one, -u, v), 'bottom': (-v, u, one),
              'top': (v, u, -one)}[name]
        dirs.append(_to_vr(np.stack(vr, -1)).reshape(n * n, S * S, 3))
        xs.append(g[..., 0].reshape(-1))
        ys.append(g[..., 1].reshape(-1))
    return np.concatenate(ys), np.concatenate(xs), np.concatenate(dirs, 0)


def _bilinear(frames, gy, gx, fx, fy):
    """frames [h, w, 3]; gy / gx [4, M] frame coordinates of the taps (top-left, top-right, bottom-left, bottom-right)."""
    t = [frames[gy[k], gx[k]].astype(np.float64) for k in range(4)]
    fx, fy = fx[:, None], fy[:, None]
    return (1. - fy) * ((1. - fx) * t[0] + fx * t[1]) + fy * ((1. - fx) * t[2] + fx * t[3])


def _src_taps(src, h, w, d):
    """d [M, 3] world directions -> (gy [4, M], gx [4, M], fx, fy, margin or None)."""
    if src['kind'] == 'er':
        x0, y0, rw, rh = _rect(src, h, w)
        az = np.arctan2(d[:, 1], d[:, 0])
        el = np.arctan2(d[:, 2], np.hypot(d[:, 0], d[:, 1]))
        x = (np.pi - az) / (2. * np.pi) * rw - 0.5
        y = np.clip((np.pi / 2. - el) / np.pi * rh - 0.5, 0., rh - 1.)
        xl, yl = np.floor(x), np.floor(y)
        ix0, ix1 = np.mod(xl, rw).astype(int), np.mod(xl + 1, rw).astype(int)
        iy0 = yl.astype(int)
        iy1 = np.minimum(iy0 + 1, rh - 1)
        gx = np.stack([ix0, ix1, ix0, ix1]) + x0
        gy = np.stack([iy0, iy0, iy1, iy1]) + y0
        return gy, gx, x - xl, y - yl, None
    grids = face_grids(h, w, src['stereo'])
    n = grids['front'].shape[0]
    vr = _to_vr(d)
    unit = np.sort(np.abs(vr) / np.linalg.norm(vr, axis=1, keepdims=True), axis=1)
    margin = unit[:, 2] - unit[:, 1]
    X, Y, Z = vr[:, 0], vr[:, 1], vr[:, 2]
    big = np.argmax(np.abs(vr), axis=1)
    gy, gx = np.zeros((4, d.shape[0]), int), np.zeros((4, d.shape[0]), int)
    fx, fy = np.zeros(d.shape[0]), np.zeros(d.shape[0])
    # (name, who, u numerator, v numerator, denominator): u = .5 + .5 num / den, CubemapProjection.py:81-121
    rules = [('front', (big == 0) & (X > 0), Y, Z, X), ('back', (big == 0) & (X <= 0), -Y, Z, -X),
             ('right', (big == 1) & (Y > 0), -X, Z, Y), ('left', (big == 1) & (Y <= 0), X, Z, -Y),
             ('bottom', (big == 2) & (Z > 0), Y, -X, Z), ('top', (big == 2) & (Z <= 0), Y, X, -Z)]
    for name, who, un, vn, den in rules:
        if not who.any():
            continue
        p, q = un[who] / den[who], vn[who] / den[who]
        if src['kind'] == 'eac':
            p, q = np.arctan(p) * 4. / np.pi, np.arctan(q) * 4. / np.pi
        x = np.clip((p + 1.) / 2. * n - 0.5, 0., n - 1.)
        y = np.clip((q + 1.) / 2. * n - 0.5, 0., n - 1.)
        xl, yl = np.floor(x).astype(int), np.floor(y).astype(int)
        xr, yb = np.minimum(xl + 1, n - 1), np.minimum(yl + 1, n - 1)
        g = grids[name]
        for k, (r, c) in enumerate(((yl, xl), (yl, xr), (yb, xl), (yb, xr))):
            gx[k, who], gy[k, who] = g[r, c, 0], g[r, c, 1]
        fx[who], fy[who] = x - xl, y - yl
    return gy, gx, fx, fy, margin


def reproject(frames, src, dst, dst_hw, rot=None, S=1):
    """frames [n, h, w, 3] uint8 -> (pre [n, H, W, 3] float64 means before rounding, NaN where the destination has no pixel;
    margin: the smallest face margin over all samples, or None for an equirectangular source)."""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    H, W = dst_hw
    ys, xs, dirs = _dst_samples(dst, H, W, S)
    pre = np.full((n, H, W, 3), np.nan)
    rot = None if rot is None else np.asarray(rot, np.float64).reshape(-1, 3, 3)
    margin = None
    taps = None
    for f in range(n):
        if taps is None or (rot is not None and rot.shape[0] > 1):
            d = dirs.reshape(-1, 3)
            if rot is not None:
                d = d @ rot[f if rot.shape[0] > 1 else 0].T
            taps = _src_taps(src, h, w, d)
            if taps[4] is not None:
                margin = taps[4].min() if margin is None else min(margin, taps[4].min())
        val = _bilinear(frames[f], taps[0], taps[1], taps[2], taps[3]).reshape(dirs.shape[0], S * S, 3)
        pre[f, ys, xs] = val.sum(1) / float(S * S)
    return pre, margin


def direction_painting(h, w):
    """[h, w, 3] uint8: the equirectangular frame painted 127.5 (1 + d) of each pixel centre's direction d, rounded."""
    az = np.pi - 2. * np.pi * (np.arange(w) + 0.5) / w
    el = np.pi / 2. - np.pi * (np.arange(h) + 0.5) / h
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :],
                  np.sin(el)[:, None] * np.ones(w)[None, :]], -1)
    return np.floor(127.5 * (1. + d) + 0.5).clip(0, 255).astype(np.uint8), d
