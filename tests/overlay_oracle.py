"""fp64 numpy restatement of the power-map overlay the reference paints over the 360-degree frames (myutils.py:246-279 over
SphericalAmbisonicsVisualizer, pyutils/ambisonics/distance.py:16-59), written from the contract - the long way round: every
node's projection per sample for the maps, whole-array numpy for the blend.  It imports nothing from the product except
`ambisonics.spherical_mesh`; the harmonics are its own, in Cartesian form.

    d = ambix[::decimate];  window = int((5 / fps) * (rate / decimate)) samples;  n_maps = len(d) // window
    map m: rms[p] = sqrt(mean_t (d[t] . sh[p])^2) over window m on spherical_mesh(res), then flipud
    normalise (r - r.min()) / (r.max() - r.min() + 0.005);  per pair (prev, cur) and i < 5, beta = i / 5:
        v = (1 - beta) prev + beta cur;  v = v 2 - 0.7;  v[v < 0] = 0;  idx = min(int(v 255), 255);  colour = YlOrRd256[idx]
        dir = resize(colour, (H, W)) 255;  alpha = resize(v[:, :, None], (H, W)) 0.6;  out = uint8(alpha dir + (1 - alpha) frame)

resize is scikit-image 0.13.1's (order 1, mode 'constant', cval 0, clip=True) as the contract fixes it; parity with the library
itself is UNPINNED until tools/overlay_pin.py has been run where that version is installed (tests/test_overlay_host.py).
"""
import numpy as np

from spatialaudiogen_amd import ambisonics

# ColorBrewer YlOrRd, 9 classes
ANCHORS = np.array([[255, 255, 204], [255, 237, 160], [254, 217, 118], [254, 178, 76], [253, 141, 60], [252, 78, 42], [227, 26, 28],
                    [189, 0, 38], [128, 0, 38]], np.float64)


def ylorrd_table():
    """The 256 entries of matplotlib's YlOrRd: entry k is the piecewise-linear curve through the anchors (at j / 8) at k / 255."""
    out = np.zeros((256, 3))
    for k in range(256):
        x = k / 255. * 8.
        j = min(int(np.floor(x)), 7)
        out[k] = (ANCHORS[j] + (x - j) * (ANCHORS[j + 1] - ANCHORS[j])) / 255.
    return out


def harmonics(phi, nu, order):
    """[..., (order + 1)^2] real spherical harmonics, ACN order, SN3D normalisation, as polynomials of the unit vector
    (x front, y left, z up): W = 1; Y = y, Z = z, X = x; V = sqrt3 x y, T = sqrt3 y z, R = (3 z^2 - 1) / 2, S = sqrt3 x z,
    U = sqrt3 (x^2 - y^2) / 2."""
    phi, nu = np.broadcast_arrays(np.asarray(phi, np.float64), np.asarray(nu, np.float64))
    x, y, z = np.cos(nu) * np.cos(phi), np.cos(nu) * np.sin(phi), np.sin(nu)
    rows = [np.ones_like(x), y, z, x]
    if order >= 2:
        q = np.sqrt(3.)
        rows += [q * x * y, q * y * z, (3. * z * z - 1.) / 2., q * x * z, q * (x * x - y * y) / 2.]
    assert order in (1, 2)
    return np.stack(rows, -1)


def plane_wave(az_deg, el_deg, signal, order):
    """A source signal [n] encoded from one direction: [n, (order + 1)^2]."""
    return np.asarray(signal, np.float64)[:, None] * harmonics(np.deg2rad(az_deg), np.deg2rad(el_deg), order)[None, :]


def maps(ambix, order, res=5.0, decimate=5, fps=10, rate=48000, frames_per_map=5):
    """[n_maps, rows, columns] fp64 maps in image orientation (flipud applied)."""
    ambix = np.asarray(ambix, np.float64)
    assert ambix.shape[1] == (order + 1) ** 2
    d = ambix[::decimate]
    window = int((float(frames_per_map) / fps) * (rate / float(decimate)))
    return maps_of(d, order, res, window)


def maps_of(d, order, res, window):
    """The maps of an already decimated stream with `window` samples per map."""
    d = np.asarray(d, np.float64)
    phi, nu = ambisonics.spherical_mesh(res)
    sh = harmonics(phi.reshape(-1), nu.reshape(-1), order)                          # [P, C], 'projection' decoding
    n_maps = d.shape[0] // window
    out = np.zeros((n_maps,) + phi.shape)
    for m in range(n_maps):
        decoded = d[m * window:(m + 1) * window] @ sh.T                             # [window, P]
        out[m] = np.flipud(np.sqrt(np.mean(decoded ** 2, 0)).reshape(phi.shape))
    return out


def resize(a, H, W):
    """a [mh, mw] or [mh, mw, channels] -> [H, W(, channels)], fp64."""
    a = np.asarray(a, np.float64)
    flat = a.ndim == 2
    a3 = a[:, :, None] if flat else a
    mh, mw, nc = a3.shape
    lo, hi = a3.min(), a3.max()

    def get(i, j):
        if i < 0 or i >= mh or j < 0 or j >= mw:
            return np.zeros(nc)
        return a3[i, j]

    out = np.zeros((H, W, nc))
    for y in range(H):
        r = (y + 0.5) * (mh / float(H)) - 0.5
        r0, r1 = int(np.floor(r)), int(np.ceil(r))
        dr = r - r0
        for x in range(W):
            c = (x + 0.5) * (mw / float(W)) - 0.5
            c0, c1 = int(np.floor(c)), int(np.ceil(c))
            dc = c - c0
            top = (1 - dc) * get(r0, c0) + dc * get(r0, c1)
            bot = (1 - dc) * get(r1, c0) + dc * get(r1, c1)
            out[y, x] = (1 - dr) * top + dr * bot
    if lo <= 0 <= hi:
        out = np.clip(out, lo, hi)
    else:
        out = np.where(out == 0.0, 0.0, np.clip(out, lo, hi))
    return out[:, :, 0] if flat else out


def resize_fast(a, H, W):
    """resize() with the per-pixel loop replaced by array indexing: the same operations on the same operands in the same order
    (tests/test_overlay_host.py holds the two to exact equality); the blend uses it to stay quick at 224 x 448."""
    a = np.asarray(a, np.float64)
    flat = a.ndim == 2
    a3 = a[:, :, None] if flat else a
    mh, mw, nc = a3.shape
    lo, hi = a3.min(), a3.max()
    pad = np.zeros((mh + 2, mw + 2, nc))
    pad[1:-1, 1:-1] = a3
    r = (np.arange(H) + 0.5) * (mh / float(H)) - 0.5
    c = (np.arange(W) + 0.5) * (mw / float(W)) - 0.5
    r0, r1, c0, c1 = np.floor(r).astype(int), np.ceil(r).astype(int), np.floor(c).astype(int), np.ceil(c).astype(int)
    dr, dc = (r - r0)[:, None, None], (c - c0)[None, :, None]
    g = lambda i, j: pad[(i + 1)[:, None], (j + 1)[None, :]]
    top = (1 - dc) * g(r0, c0) + dc * g(r0, c1)
    bot = (1 - dc) * g(r1, c0) + dc * g(r1, c1)
    out = (1 - dr) * top + dr * bot
    if lo <= 0 <= hi:
        out = np.clip(out, lo, hi)
    else:
        out = np.where(out == 0.0, 0.0, np.clip(out, lo, hi))
    return out[:, :, 0] if flat else out


def normalise(m):
    m = np.asarray(m, np.float64)
    return (m - m.min()) / (m.max() - m.min() + 0.005)


def mix(prev_n, cur_n, beta):
    """The interpolated, shifted, clamped map v of one frame from two NORMALISED maps."""
    v = (1 - beta) * prev_n + beta * cur_n
    v = v * 2. - 0.7
    v[v < 0] = 0
    return v


def blend(raw_maps, frames, lut, frames_per_map=5, map0=0, frame0=0, resize_fn=resize_fast):
    """raw_maps [n_maps, mh, mw] (any float type; taken to fp64 first) from absolute map index map0, frames [n, H, W, 3] uint8 from
    absolute frame index frame0 -> (out uint8 [n, H, W, 3], pre fp64 [n, H, W, 3] = every pixel before the truncation,
    v255 [n, mh, mw] = v 255 of every node, whose integer part is the colour index).  Every frame given must have both its maps."""
    raw_maps = np.asarray(raw_maps, np.float64)
    frames = np.asarray(frames)
    n, H, W = frames.shape[:3]
    norm = [normalise(m) for m in raw_maps]
    out = np.zeros(frames.shape, np.uint8)
    pre = np.zeros(frames.shape, np.float64)
    v255 = np.zeros((n,) + raw_maps.shape[1:])
    for f in range(n):
        F = frame0 + f
        prev, i = F // frames_per_map - map0, F % frames_per_map
        assert prev >= 0 and prev + 1 < len(norm), 'frame %d needs a map that was not given' % F
        beta = i / float(frames_per_map)
        v = mix(norm[prev], norm[prev + 1], beta)
        v255[f] = v * 255
        idx = (v * 255).astype(int)
        idx[idx > 255] = 255
        dir_map = resize_fn(lut[idx], H, W) * 255
        alpha = resize_fn(v[:, :, None], H, W) * 0.6
        pre[f] = alpha * dir_map + (1 - alpha) * frames[f]
        out[f] = pre[f].astype(np.uint8)
    return out, pre, v255


def overlay(ambix, frames, order, res=5.0, decimate=5, fps=10, rate=48000, frames_per_map=5):
    """The whole of myutils.py:246-279: (frames written [min(n, 5 (n_maps - 1)), H, W, 3], maps)."""
    m = maps(ambix, order, res, decimate, fps, rate, frames_per_map)
    n = max(0, min(len(frames), frames_per_map * (len(m) - 1)))
    if n == 0:
        return np.asarray(frames)[:0], m
    return blend(m, np.asarray(frames)[:n], ylorrd_table(), frames_per_map)[0], m
