"""fp64 numpy restatement of the optical flow estimator and of the flow folder's byte coding (include/sagen.h: sagen_optical_flow,
sagen_flow_encode), written from the description of the algorithm - whole-array np.roll / index arrays, no per-pixel code and
nothing taken from csrc/flow_core.h.  Test infrastructure only.

Neighbour rule: rows clamp, columns wrap (wrap=True) or clamp."""
import numpy as np


def shifted(a, dy, dx, wrap):
    """a[..., y + dy, x + dx] under the neighbour rule."""
    h, w = a.shape[-2:]
    ys = np.clip(np.arange(h) + dy, 0, h - 1)
    xs = np.mod(np.arange(w) + dx, w) if wrap else np.clip(np.arange(w) + dx, 0, w - 1)
    return a[..., ys[:, None], xs[None, :]]


def luma(frames):
    f = frames.astype(np.float64)
    return 0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]


def halve(a):
    return 0.25 * (a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2])


def smooth(a, wrap):
    k = (1., 4., 6., 4., 1.)
    rows = sum(k[i] * shifted(a, 0, i - 2, wrap) for i in range(5)) / 16.
    return sum(k[i] * shifted(rows, i - 2, 0, wrap) for i in range(5)) / 16.


def bilinear(a, x, y, wrap):
    h, w = a.shape
    y = np.clip(y, 0., h - 1.)
    if not wrap:
        x = np.clip(x, 0., w - 1.)
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = x0 + 1, np.minimum(y0 + 1, h - 1)
    if wrap:
        x0, x1 = np.mod(x0, w), np.mod(x1, w)
    else:
        x1 = np.minimum(x1, w - 1)
    return (1. - ay) * ((1. - ax) * a[y0, x0] + ax * a[y0, x1]) + ay * ((1. - ax) * a[y1, x0] + ax * a[y1, x1])


def hs_average(u, wrap):
    edges = shifted(u, -1, 0, wrap) + shifted(u, 1, 0, wrap) + shifted(u, 0, -1, wrap) + shifted(u, 0, 1, wrap)
    diagonals = shifted(u, -1, -1, wrap) + shifted(u, -1, 1, wrap) + shifted(u, 1, -1, wrap) + shifted(u, 1, 1, wrap)
    return edges / 6. + diagonals / 12.


def flow_pair(g1, g2, levels=5, warps=3, iters=30, alpha=8., wrap=True):
    """Flow from luma image g1 to g2, fp64 [h, w, 2] (u to the right, v down)."""
    p1, p2 = [g1], [g2]
    for _ in range(1, levels):
        p1.append(halve(p1[-1]))
        p2.append(halve(p2[-1]))
    u = v = None
    for l in range(levels - 1, -1, -1):
        s1, s2 = smooth(p1[l], wrap), smooth(p2[l], wrap)
        h, w = s1.shape
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
        if u is None:
            u, v = np.zeros((h, w)), np.zeros((h, w))
        else:
            cx, cy = (xx + 0.5) / 2. - 0.5, (yy + 0.5) / 2. - 0.5
            u, v = 2. * bilinear(u, cx, cy, wrap), 2. * bilinear(v, cx, cy, wrap)
        for _ in range(warps):
            u0, v0 = u, v
            warped = bilinear(s2, xx + u0, yy + v0, wrap)
            ix = ((shifted(warped, 0, 1, wrap) - shifted(warped, 0, -1, wrap)) + (shifted(s1, 0, 1, wrap) - shifted(s1, 0, -1, wrap))) / 4.
            iy = ((shifted(warped, 1, 0, wrap) - shifted(warped, -1, 0, wrap)) + (shifted(s1, 1, 0, wrap) - shifted(s1, -1, 0, wrap))) / 4.
            it = warped - s1
            for _ in range(iters):
                ub, vb = hs_average(u, wrap), hs_average(v, wrap)
                t = (ix * (ub - u0) + iy * (vb - v0) + it) / (alpha * alpha + ix * ix + iy * iy)
                u, v = ub - ix * t, vb - iy * t
    return np.stack([u, v], -1)


def optical_flow(frames, levels=5, warps=3, iters=30, alpha=8., wrap=True):
    """frames [n, h, w, 3] uint8 -> fp64 [n - 1, h, w, 2] BEFORE the rounding to fp32."""
    g = luma(frames)
    return np.stack([flow_pair(g[k], g[k + 1], levels, warps, iters, alpha, wrap) for k in range(len(frames) - 1)], 0)


def encode(flow):
    """flow [n, h, w, 2] float32 -> (pre [n, h, w, 3] fp64: the byte values BEFORE truncation, limits [n, 2] float32)."""
    flow = np.asarray(flow, np.float32)
    u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    mag = np.sqrt(u * u + v * v).astype(np.float32)
    ang = np.arctan2(v, u) + np.pi
    ang[mag < np.float32(0.005)] = 0.
    lo, hi = mag.min(axis=(1, 2)), mag.max(axis=(1, 2))
    hi = np.where(hi - lo < np.float32(1.), lo + np.float32(1.), hi).astype(np.float32)
    lo64, hi64 = lo.astype(np.float64)[:, None, None], hi.astype(np.float64)[:, None, None]
    pre = np.zeros(flow.shape[:3] + (3,))
    pre[..., 0] = ang * 255. / (np.pi * 2.)
    pre[..., 2] = (mag.astype(np.float64) - lo64) / (hi64 - lo64) * 255.
    return pre, np.stack([lo, hi], -1).astype(np.float32)


def pattern(h, w, dx=0., dy=0., seed=0, waves=24):
    """A smooth random pattern, periodic in x, displaced by (dx, dy): a sum of `waves` cosines scaled into 27.5 .. 227.5 levels."""
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64) - dy, np.arange(w, dtype=np.float64) - dx, indexing='ij')
    out = np.zeros((h, w))
    for _ in range(waves):
        kx, ky, ph, a = r.randint(-6, 7), r.uniform(-6., 6.), r.uniform(0., 2. * np.pi), r.uniform(0.3, 1.)
        out += a * np.cos(2. * np.pi * (kx * xx / w + ky * yy / (2. * h)) + ph)
    return 127.5 + 100. * out / np.abs(out).max()


def pattern_frames(h, w, shifts, seed=0):
    """uint8 RGB frames [len(shifts), h, w, 3] of the pattern at the given (dx, dy); the channels are the pattern at three gains, so
    that the luma weights matter."""
    frames = []
    for dx, dy in shifts:
        p = pattern(h, w, dx, dy, seed)
        frames.append(np.stack([np.floor(p + 0.5), np.floor(0.9 * p + 12. + 0.5), np.floor(1.05 * p - 4. + 0.5)], -1))
    return np.clip(np.stack(frames, 0), 0, 255).astype(np.uint8)
