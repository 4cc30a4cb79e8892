"""fp64 numpy oracle of the moving point sources (include/sagen.h: sagen_source_track / sagen_encode_sources /
sagen_binauralize_sources), written from the header's definitions and NOT from the product's code: each quantity once as a literal
loop per sample - the definition - and once vectorised for the longer cases; tests/test_sources_host.py holds the two equal.  The
harmonics come from the Legendre form (render_oracle.sh_lpmv) at the polar angles of the direction, not from the cartesian closed
forms the kernels use.

Conventions: x front, y left, z up; polar (phi, nu, r); ACN / SN3D."""
from math import cos, sin, floor, sqrt

import numpy as np

import render_oracle as RO

C_SOUND = 343.
EARS = np.array([[0., 0.1, 0.], [0., -0.1, 0.]])
TIE = 1e-12


def nframes_of(n_samples, rate):
    duration = n_samples / float(rate)
    return int(duration * rate)


# ---- the definition: one sample at a time ---------------------------------------------------------------------------------------
def tic(cp, n_samples, rate, i):
    """(phi, nu, r) of sample i."""
    cp = np.asarray(cp, np.float64).reshape(-1, 3)
    P = len(cp)
    duration = n_samples / float(rate)
    nframes = int(duration * rate)
    assert 0 <= i < nframes
    if P == 1:
        return tuple(cp[0])
    idx = P - 1 if i == nframes - 1 else int(floor(i * ((P - 1) / float(nframes - 1))))
    if idx == P - 1:
        return tuple(cp[-1])
    t = [duration if j == P - 1 else j * (duration / (P - 1)) for j in range(P)]
    alpha = (i * (1 / float(rate)) - t[idx]) / (t[idx + 1] - t[idx])
    return tuple(alpha * cp[idx + 1] + (1 - alpha) * cp[idx])


def unit(phi, nu, r):
    if r == 0:
        return np.array([1., 0., 0.])
    sg = -1. if r < 0 else 1.
    return sg * np.array([cos(phi) * cos(nu), sin(phi) * cos(nu), sin(nu)])


def harmonics(u, order):
    u = np.asarray(u, np.float64)
    return RO.sh_lpmv(np.arctan2(u[..., 1], u[..., 0]), np.arctan2(u[..., 2], np.hypot(u[..., 0], u[..., 1])), order)


def nearest(dirs, u):
    dots = dirs @ u
    return int(np.flatnonzero(dots >= dots.max() - TIE)[0])


def encode_loop(signals, cps, rate, order, t0, n, distance_model=False, radius=1.):
    out = np.zeros((n, (order + 1) ** 2))
    for a in range(n):
        t = t0 + a
        for sig, cp in zip(signals, cps):
            phi, nu, r = tic(cp, len(sig), rate, t)
            g, d = 1., 0
            if distance_model:
                dist = abs(r) - radius
                assert dist > 0
                d = int(dist / 343. * rate)
                g = 1. / (1. + dist)
            if t - d >= 0:
                out[a] += g * float(sig[t - d]) * harmonics(unit(phi, nu, r), order)
    return out


def mic_loop(signals, cps, rate, t0, n):
    out = np.zeros((n, 2))
    S = len(signals)
    for a in range(n):
        t = t0 + a
        for sig, cp in zip(signals, cps):
            phi, nu, r = tic(cp, len(sig), rate, t)
            pos = abs(r) * unit(phi, nu, r)
            for e in range(2):
                dist = sqrt(((pos - EARS[e]) ** 2).sum())
                d = int(dist / 343. * rate)
                if t - d >= 0:
                    out[a, e] += float(sig[t - d]) / (1. + dist) / S
    return out


def hrir_loop(signals, cps, rate, dirs, left, right, zero_before, t0, n):
    out = np.zeros((n, 2))
    K = left.shape[1]
    for a in range(n):
        t = t0 + a
        if t < zero_before:
            continue
        for sig, cp in zip(signals, cps):
            j = nearest(dirs, unit(*tic(cp, len(sig), rate, t)))
            for k in range(min(K, t + 1)):
                out[a, 0] += left[j, k] * float(sig[t - k])
                out[a, 1] += right[j, k] * float(sig[t - k])
    return out


# ---- vectorised -----------------------------------------------------------------------------------------------------------------
def track(cp, n_samples, rate, samples):
    """(polar [m, 3], unit [m, 3]) at the sample indices `samples`."""
    cp = np.asarray(cp, np.float64).reshape(-1, 3)
    i = np.asarray(samples, np.int64)
    P = len(cp)
    duration = n_samples / float(rate)
    nframes = int(duration * rate)
    assert i.min() >= 0 and i.max() < nframes
    if P == 1:
        pol = np.repeat(cp[:1], len(i), 0)
    else:
        idx = np.floor(i * ((P - 1) / float(max(nframes - 1, 1)))).astype(np.int64)
        idx[i == nframes - 1] = P - 1
        t = np.arange(P) * (duration / (P - 1))
        t[-1] = duration
        lo = np.minimum(idx, P - 2)
        alpha = ((i * (1 / float(rate)) - t[lo]) / (t[lo + 1] - t[lo]))[:, None]
        pol = alpha * cp[lo + 1] + (1 - alpha) * cp[lo]
        pol[idx == P - 1] = cp[-1]
    phi, nu, r = pol[:, 0], pol[:, 1], pol[:, 2]
    u = np.sign(r)[:, None] * np.stack([np.cos(phi) * np.cos(nu), np.sin(phi) * np.cos(nu), np.sin(nu)], -1)
    u[r == 0] = [1., 0., 0.]
    return pol, u


def nearest_all(dirs, u):
    """(nearest index [m], margin [m]): margin = how far below the maximum the best candidate that does NOT tie lies."""
    dots = u @ dirs.T
    mx = dots.max(1, keepdims=True)
    ties = dots >= mx - TIE
    rest = np.where(ties, -np.inf, dots).max(1)
    return ties.argmax(1), mx[:, 0] - rest, dots


def _delayed(sig, t, d):
    j = t - d
    ok = (j >= 0) & (j < len(sig))
    return np.where(ok, np.asarray(sig, np.float64)[np.clip(j, 0, len(sig) - 1)], 0.)


def encode(signals, cps, rate, order, t0, n, distance_model=False, radius=1.):
    t = np.arange(t0, t0 + n)
    out = np.zeros((n, (order + 1) ** 2))
    for sig, cp in zip(signals, cps):
        pol, u = track(cp, len(sig), rate, t)
        g, d = np.ones(n), np.zeros(n, np.int64)
        if distance_model:
            dist = np.abs(pol[:, 2]) - radius
            assert (dist > 0).all()
            d = (dist / 343. * rate).astype(np.int64)
            g = 1. / (1. + dist)
        out += (g * _delayed(sig, t, d))[:, None] * harmonics(u, order)
    return out


def mic(signals, cps, rate, t0, n):
    t = np.arange(t0, t0 + n)
    out = np.zeros((n, 2))
    for sig, cp in zip(signals, cps):
        pol, u = track(cp, len(sig), rate, t)
        pos = np.abs(pol[:, 2:3]) * u
        for e in range(2):
            dist = np.sqrt(((pos - EARS[e]) ** 2).sum(1))
            out[:, e] += _delayed(sig, t, (dist / 343. * rate).astype(np.int64)) / (1. + dist) / len(signals)
    return out


def hrir(signals, cps, rate, dirs, left, right, zero_before, t0, n):
    t = np.arange(t0, t0 + n)
    out = np.zeros((n, 2))
    K = left.shape[1]
    for sig, cp in zip(signals, cps):
        near = nearest_all(dirs, track(cp, len(sig), rate, t)[1])[0]
        x = np.concatenate([np.zeros(K - 1), np.asarray(sig, np.float64)])
        win = np.lib.stride_tricks.sliding_window_view(x, K)[t][:, ::-1]          # win[a, k] = sig[t - k]
        out[:, 0] += np.einsum('ak,ak->a', left[near], win)
        out[:, 1] += np.einsum('ak,ak->a', right[near], win)
    out[t < zero_before] = 0.
    return out


def source_maps(cps, duration, rate=10., angular_res=5):
    """distance.py:62-97: per frame 1 / S at the mesh node closest to each source; [n_frames, mh, mw], unflipped."""
    phi = np.flip(np.arange(-180., 180., angular_res) / 180. * np.pi, 0)
    nu = np.arange(-90., 90.1, angular_res) / 180. * np.pi
    phi, nu = np.meshgrid(phi, nu)
    mesh = np.stack([np.cos(nu) * np.cos(phi), np.cos(nu) * np.sin(phi), np.sin(nu)], -1).reshape(-1, 3)
    n_samples = int(duration * rate)
    n_frames = nframes_of(n_samples, rate)
    maps = np.zeros((n_frames, mesh.shape[0]))
    for cp in cps:
        near = nearest_all(mesh, track(cp, n_samples, rate, np.arange(n_frames))[1])[0]
        maps[np.arange(n_frames), near] += 1. / len(cps)
    return maps.reshape((n_frames,) + phi.shape)
