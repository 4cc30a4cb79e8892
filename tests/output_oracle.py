"""An exact fp32 restatement of the output stage (include/sagen.h: sagen_render_fir, sagen_encode_sources, sagen_binauralize_sources)
in the order of summation the header promises, pure numpy, importing nothing of the package: what csrc/render.hip and
csrc/sources.hip must produce BIT FOR BIT.  Geometry (trajectories, directions, nearest indices) and the fp64 references come from
render_oracle / sources_oracle; this module adds

  * fma32: a correctly rounded fp32 fused multiply-add, vectorised;
  * render_fir_fp32, encode_fp32, mic_fp32, hrir_fp32: every step of the header's sum in fp32, one accumulator per output,
    channels / sources outermost, taps ascending, one fma32 each;
  * per family the sum of magnitudes A and the term count n of every output (the elementwise bounds of test_gpu_output_ops.py);
  * the input conditions under which the device's fp64 front end (its own sin / cos) cannot move a coefficient, a delay or a
    nearest index away from this module's: distances to fp32 rounding ties, to integer delays, and nearest-index margins;
  * the case tables of the sweep (test_gpu_output_ops.py, test_cpu_twin_output_ops.py) and their operands, seeded.
test_output_oracle_host.py checks all of it without a device."""
import collections
import functools

import numpy as np

import render_oracle as RO
import sources_oracle as SO
from resample_oracle import tie_distance

F32 = np.float32
U = 2.0 ** -24
TIE_REL = 2.0 ** -40          # no fp64 coefficient closer than this (relative) to an fp32 rounding tie
TIE_ABS = 2.0 ** -46          # nor closer than this in absolute terms: fp64 sin / cos of two libraries differ by ~1e-16 ABSOLUTE, which
                              # is not small relative to a harmonic near a zero crossing; 1.4e-14 leaves two orders over that
DELAY_MARGIN = 1e-9           # no delay dist / 343 * rate this close to an integer
NEAR_LO, NEAR_HI = 1e-13, 1e-9     # no candidate direction this far below the maximum (test_gpu_sources.test_track_nearest's rule)
RMS_BAR = 1e-5


# ---- fp32 fused multiply-add ----------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """round_fp32(a * b + c) with ONE rounding, elementwise over fp32 arrays (broadcast).  The product of two fp32 values is exact
    in fp64; s = p + c is rounded once to fp64; float32(s) differs from the true fma only where s lies exactly on an fp32 rounding
    tie while p + c was inexact - then the TwoSum residual says on which side of the tie the true sum lies."""
    a, b, c = (np.asarray(v) for v in (a, b, c))
    assert a.dtype == b.dtype == c.dtype == np.float32, (a.dtype, b.dtype, c.dtype)
    a, b, c = np.broadcast_arrays(a.astype(np.float64), b.astype(np.float64), c.astype(np.float64))
    p = a * b
    s = p + c
    r = np.array(s.astype(np.float32), ndmin=1)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # TwoSum: p + c = s + err exactly
    d = np.asarray(s - r.reshape(s.shape).astype(np.float64)).reshape(-1)
    err = np.asarray(err).reshape(-1)
    cand = np.flatnonzero((err != 0) & (d != 0))
    if cand.size:
        rf = r.reshape(-1)
        rc, dc, ec = rf[cand], d[cand], err[cand]
        nb = np.nextafter(rc, np.where(dc > 0, np.inf, -np.inf).astype(np.float32))      # the other fp32 neighbour of s
        tie = (nb.astype(np.float64) - rc.astype(np.float64)) == 2.0 * dc                # s exactly halfway between rc and nb
        move = tie & ((ec > 0) == (dc > 0))                                              # and the true sum on nb's side
        rf[cand[move]] = nb[move]
        r = rf
    return r.reshape(s.shape)


# ---- sagen_render_fir -----------------------------------------------------------------------------------------------------------
def _rot_index(s, n_rot, rot_hop):
    m = np.minimum(s // rot_hop, n_rot - 1)
    return m, np.minimum(m + 1, n_rot - 1)


def rotate_fp32(x, s, rot, rot_hop):
    """x'[s] = M(s) x[s] in fp32: al = 0 where the matrix is held, else float32(s - m hop) / float32(hop); be = 1 - al;
    M = fma32(al, R[m1], be * R[m]); x'[c] accumulated over e ascending by fma32(M[c][e], x[e], acc)."""
    rot = np.asarray(rot)
    assert rot.dtype == np.float32 and x.dtype == np.float32
    m, m1 = _rot_index(s, len(rot), rot_hop)
    al = np.where(m1 == m, F32(0), (s - m * rot_hop).astype(F32) / F32(rot_hop)).astype(F32)
    be = F32(1) - al
    r0, r1 = rot[m], rot[m1]                             # [rows, C, C]
    acc = np.zeros_like(x)
    for e in range(x.shape[1]):
        M = fma32(al[:, None], r1[:, :, e], be[:, None] * r0[:, :, e])
        acc = fma32(M, x[:, e:e + 1], acc)
    return acc


def render_fir_fp32(x, n_hist, taps, rot=None, rot_hop=1, pos0=0, zero_before=0):
    """sagen_render_fir in the header's order, every step in fp32: x [n_hist + n, C] (the history rows first), taps [O, C, K],
    rot [n_rot, C, C] or None -> y [n, O].  Rows before x[0] count as zero; outputs at absolute t < zero_before are 0."""
    x, taps = np.asarray(x), np.asarray(taps)
    assert x.dtype == np.float32 and taps.dtype == np.float32
    rows, C = x.shape
    O, C2, K = taps.shape
    n = rows - n_hist
    assert C == C2 and n >= 1 and 0 <= n_hist <= pos0
    s = pos0 - n_hist + np.arange(rows, dtype=np.int64)
    xr = x if rot is None else rotate_fp32(x, s, rot, rot_hop)
    xp = np.concatenate([np.zeros((K - 1, C), F32), xr])
    acc = np.zeros((n, O), F32)
    for c in range(C):                                   # channels outermost
        for k in range(K):                               # taps ascending
            lo = K - 1 + n_hist - k
            acc = fma32(taps[None, :, c, k], xp[lo:lo + n, c][:, None], acc)
    acc[pos0 + np.arange(n, dtype=np.int64) < zero_before] = 0
    return acc


def render_ref(x, n_hist, taps, rot=None, rot_hop=1, pos0=0, zero_before=0):
    """The fp64 definition (render_oracle.rotated_fir) of the same call."""
    return RO.rotated_fir(x, taps, rot, rot_hop, zero_before, pos0=pos0 - n_hist)[n_hist:]


def render_abs_sum(x, n_hist, taps, rot=None, rot_hop=1, pos0=0, zero_before=0):
    """(A [n, O], terms [n, 1]): A = sum_c sum_k |h| Xbar, Xbar = |x| unrotated and sum_e ((1 - a)|R[m]| + a|R[m1]|)_ce |x_e| rotated;
    terms = C * (taps that reach a row of x).  A = 0 where the output is zeroed."""
    x, taps = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(taps, np.float64))
    rows, C = x.shape
    O, _, K = taps.shape
    n = rows - n_hist
    if rot is not None:
        rot = np.abs(np.asarray(rot, np.float64))
        s = pos0 - n_hist + np.arange(rows, dtype=np.int64)
        m, m1 = _rot_index(s, len(rot), rot_hop)
        a = np.where(m1 == m, 0., (s - m * rot_hop) / float(rot_hop))[:, None, None]
        x = np.einsum('sce,se->sc', (1. - a) * rot[m] + a * rot[m1], x)
    A = np.zeros((n, O))
    for o in range(O):
        for c in range(C):
            A[:, o] += np.convolve(x[:, c], taps[o, c])[n_hist:rows]
    A[pos0 + np.arange(n, dtype=np.int64) < zero_before] = 0.
    return A, (C * np.minimum(K, n_hist + 1 + np.arange(n)))[:, None]


# ---- the moving sources ---------------------------------------------------------------------------------------------------------
def harmonics_closed(u, order):
    """The header's closed forms, fp64, in the order of its table: W Y Z X | V T R S U."""
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    Y = [np.ones_like(x), y, z, x]
    if order == 2:
        s3 = 1.7320508075688772
        Y += [s3 * x * y, s3 * y * z, (3. * z * z - 1.) / 2., s3 * x * z, (s3 / 2.) * (x * x - y * y)]
    return np.stack(Y, -1)


class Conditions(object):
    """What the inputs of one case leave between this module's fp64 front end and another correct one (the device's)."""

    def __init__(self):
        self.tie_rel = self.tie_abs = self.delay = np.inf
        self.ambiguous = 0

    def coefficients(self, v):
        v = np.asarray(v, np.float64).reshape(-1)
        v = v[v != 0]                                    # (an exact zero comes from exact inputs: sin 0, the r == 0 rule)
        if v.size:
            rel = tie_distance(v)
            self.tie_rel = min(self.tie_rel, float(rel.min()))
            self.tie_abs = min(self.tie_abs, float((rel * np.abs(v)).min()))

    def delays(self, dd):
        dd = np.asarray(dd, np.float64)
        if dd.size:
            self.delay = min(self.delay, float(np.abs(dd - np.rint(dd)).min()))

    def nearest(self, dots):
        below = dots.max(1, keepdims=True) - dots
        self.ambiguous += int(((below > NEAR_LO) & (below < NEAR_HI)).sum())

    def problems(self):
        out = []
        if self.tie_rel < TIE_REL or self.tie_abs < TIE_ABS:
            out.append('a coefficient %.3g (relative) / %.3g (absolute) from an fp32 rounding tie' % (self.tie_rel, self.tie_abs))
        if self.delay < DELAY_MARGIN:
            out.append('a delay %.3g from an integer' % self.delay)
        if self.ambiguous:
            out.append('%d ambiguous nearest indices' % self.ambiguous)
        return out


Restated = collections.namedtuple('Restated', 'y A terms cond')       # y fp32 [n, outs]; A fp64 [n, outs]; terms [n, outs] or [n, 1]


def _gather(sig, nf, j):
    ok = (j >= 0) & (j < nf)
    return ok, np.where(ok, sig[np.clip(j, 0, len(sig) - 1)], F32(0)).astype(F32)


def _weighted(signals, rate, t, coefficients):
    """sum over the sources (outermost, in order) of fma32(float32(coef), sig[t - d], acc); `coefficients(sig, k)` yields per output
    column (coef64 [n], delay64 [n] or None) - the delay in samples before int()."""
    acc = A = terms = None
    cond = Conditions()
    for k, sig in enumerate(signals):
        assert sig.dtype == np.float32
        nf = SO.nframes_of(len(sig), rate)
        cols = coefficients(sig, k)
        if acc is None:
            acc, A, terms = np.zeros((len(t), len(cols)), F32), np.zeros((len(t), len(cols))), np.zeros((len(t), len(cols)), np.int64)
        for c, (coef, dd) in enumerate(cols):
            d = np.zeros(len(t), np.int64) if dd is None else dd.astype(np.int64)        # int(): towards zero
            ok, xs = _gather(sig, nf, t - d)
            acc[:, c] = np.where(ok, fma32(coef.astype(F32), xs, acc[:, c]), acc[:, c])
            A[:, c] += np.where(ok, np.abs(coef * xs), 0.)
            terms[:, c] += ok
            cond.coefficients(coef[ok])
            if dd is not None:
                cond.delays(dd)
    return Restated(acc, A, terms, cond)


def encode_fp32(signals, cps, rate, order, t0, n, distance_model=False, radius=1.):
    """sagen_encode_sources: coefficient float32(g Y_c) from the oracle's trajectory, rounded once; sources outermost."""
    t = np.arange(t0, t0 + n, dtype=np.int64)

    def coefficients(sig, k):
        pol, u = SO.track(cps[k], len(sig), rate, t)
        Y = harmonics_closed(u, order)
        g, dd = np.ones(n), None
        if distance_model:
            dist = np.abs(pol[:, 2]) - radius
            dd = dist / 343. * rate
            g = 1. / (1. + dist)
        return [(g * Y[:, c], dd) for c in range(Y.shape[1])]
    return _weighted(signals, rate, t, coefficients)


def mic_fp32(signals, cps, rate, t0, n):
    """sagen_binauralize_sources, SAGEN_SOURCES_MIC: coefficient float32((1 / S) / (1 + dist)) per ear."""
    t = np.arange(t0, t0 + n, dtype=np.int64)
    inv_s = 1. / float(len(signals))

    def coefficients(sig, k):
        pol, u = SO.track(cps[k], len(sig), rate, t)
        pos = np.abs(pol[:, 2:3]) * u
        out = []
        for e in range(2):
            dy = pos[:, 1] - SO.EARS[e, 1]
            dist = np.sqrt(pos[:, 0] * pos[:, 0] + dy * dy + pos[:, 2] * pos[:, 2])
            out.append((inv_s / (1. + dist), dist / 343. * rate))
        return out
    return _weighted(signals, rate, t, coefficients)


def hrir_fp32(signals, cps, rate, dirs, hrir, zero_before, t0, n):
    """sagen_binauralize_sources, SAGEN_SOURCES_HRIR: hrir [D, 2, K] fp32; the nearest index from sources_oracle.nearest_all; sources
    outermost, taps ascending; terms with t - k < 0 dropped (they are zeros)."""
    hrir = np.asarray(hrir)
    assert hrir.dtype == np.float32
    K = hrir.shape[2]
    t = np.arange(t0, t0 + n, dtype=np.int64)
    acc, A, terms = np.zeros((n, 2), F32), np.zeros((n, 2)), np.zeros((n, 1), np.int64)
    cond = Conditions()
    for sig, cp in zip(signals, cps):
        assert sig.dtype == np.float32
        nf = SO.nframes_of(len(sig), rate)
        near, _, dots = SO.nearest_all(dirs, SO.track(cp, len(sig), rate, t)[1])
        cond.nearest(dots)
        h = hrir[near]                                   # [n, 2, K]
        for k in range(K):
            ok, xs = _gather(sig, nf, t - k)
            acc = fma32(h[:, :, k], xs[:, None], acc)
            A += np.abs(h[:, :, k].astype(np.float64) * xs[:, None])
        terms[:, 0] += np.minimum(K, t + 1)
    z = t < zero_before
    acc[z] = 0
    A[z] = 0.
    return Restated(acc, A, terms, cond)


# ---- the cases of the sweep -----------------------------------------------------------------------------------------------------
TAPS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 23, 24, 511, 512)
LENGTHS = (1, 7, 8, 9, 511, 512, 513, 1023, 1024, 1025, 2049)          # the lane of 8, the item of 512, the tile of 1024
OUTPUTS = (1, 2, 3, 5, 32)
HIST_KINDS = ('0', '1', 'K-2', 'K-1', 'K+5')
ZERO_KINDS = ('before', 'pos0+3', 'pos0+700', 'past')
ROTATIONS = ((0, 1), (1, 1), (2, 3), (5, 8), (5, 1000), (2, 1), (1, 8), (5, 3), (2, 1000))        # (n_rot, rot_hop); n_rot 0: unrotated
FAR = 2 ** 33 + 5
INT_HOP = {1: 1, 3: 4, 8: 8, 1000: 256}                  # the power-of-two hop the integer run of a case uses

RenderCase = collections.namedtuple('RenderCase', 'name C K n O n_hist pos0 zero_before n_rot rot_hop seed')


def tap_paths(K):
    """(K % 4, full % 3): the partial last block's taps and the remainder loop's blocks of render_fir_kernel."""
    return K % 4, (K // 4) % 3


def _n_hist(kind, K):
    return {'0': 0, '1': 1, 'K-2': max(K - 2, 0), 'K-1': K - 1, 'K+5': K + 5}[kind]


def _zero_before(kind, pos0, n):
    return {'before': 0, 'pos0+3': pos0 + 3, 'pos0+700': pos0 + 700, 'past': pos0 + n + 10}[kind]


def _render_case(name, C, K, n, O, hist, far, zero, rotation, seed, pos0=None):
    n_hist = _n_hist(hist, K)
    pos0 = (FAR if far else n_hist) if pos0 is None else pos0
    return RenderCase(name, C, K, n, O, n_hist, pos0, _zero_before(zero, pos0, n), rotation[0], rotation[1], seed)


@functools.lru_cache(None)
def render_cases():
    """A selection, not a product: every K of TAPS for both C with the other dimensions cycled at strides that hit every value for each
    C (test_output_oracle_host.py asserts it), then the directed cases.  K >= 511 stays at n <= 1100."""
    out = []
    for C in (4, 9):
        off = 0 if C == 4 else 3
        for i, K in enumerate(TAPS):
            j = i + off
            n = LENGTHS[(2 * j) % len(LENGTHS)] if K < 511 else (513, 1025)[(i + off) % 2]
            O = OUTPUTS[j % len(OUTPUTS)] if K < 511 or OUTPUTS[j % len(OUTPUTS)] < 32 else 3
            zero = ZERO_KINDS[(j // 2) % 3]              # never 'past', and never a prefix that swallows the call: every K keeps checked values
            zero = 'before' if n <= 3 else 'pos0+3' if zero == 'pos0+700' and n <= 700 else zero
            out.append(_render_case('c%d_k%d' % (C, K), C, K, n, O, HIST_KINDS[j % 5], (i + (C == 9)) % 2 == 1, zero,
                                    ROTATIONS[j % len(ROTATIONS)], 1000 * C + K))
        # directed: the widest table at the longest taps; a seam inside the history rows (s = 2000 in 1990 .. 2002) and inside a tile
        # (3000, 4000), the trajectory ending inside the call (s = 4000 of 2003 .. 4051); a trajectory ending in the first tile; a
        # one-sample-per-control-point trajectory; mid-stream with a short history; zero_before inside a lane and inside a later tile;
        # zero_before past the end (the only case without a checked non-zero value)
        out.append(_render_case('c%d_k512_o32' % C, C, 512, 513, 32, 'K-1', True, 'before', (0, 1), 7000 + C))
        out.append(_render_case('c%d_seam_in_history' % C, C, 14, 2049, 2, 'K-1', False, 'before', (5, 1000), 7100 + C, pos0=2003))
        out.append(_render_case('c%d_ends_in_tile' % C, C, 23, 1025, 3, 'K-1', False, 'pos0+3', (5, 8), 7200 + C, pos0=25))
        out.append(_render_case('c%d_hop1' % C, C, 7, 9, 5, '1', False, 'before', (5, 1), 7300 + C, pos0=1))
        out.append(_render_case('c%d_short_history_midstream' % C, C, 24, 1023, 2, '1', True, 'pos0+700', (2, 3), 7400 + C))
        out.append(_render_case('c%d_zero_in_second_tile' % C, C, 9, 2049, 1, 'K-2', False, 'pos0+700', (0, 1), 7500 + C, pos0=4096 + 330))
        out.append(_render_case('c%d_seam_hop3' % C, C, 13, 513, 5, 'K+5', False, 'before', (5, 3), 7600 + C, pos0=18))
        out.append(_render_case('c%d_all_zeroed' % C, C, 6, 513, 2, 'K-1', False, 'past', (1, 1), 7700 + C))
    return tuple(out)


def _signed_permutations(r, n_rot, C):
    out = np.zeros((n_rot, C, C), F32)
    for m in range(n_rot):
        out[m, np.arange(C), r.permutation(C)] = r.choice([-1., 1.], size=C)
    return out


@functools.lru_cache(None)
def render_operands(case, integers=False):
    """(x [n_hist + n, C], taps [O, C, K], rot [n_rot, C, C] or None, rot_hop), fp32.  Random: noise and decaying random responses (as
    render_oracle.make_hrirs), near-orthogonal matrices.  Integers: samples -3..3, taps -2..2, signed permutations, a power-of-two hop:
    al, M, x' and every partial sum are then exact dyadics (C K 6 256 < 2^24)."""
    c = case
    r = np.random.RandomState(c.seed + (500000 if integers else 0))
    rows = c.n_hist + c.n
    if integers:
        x = r.randint(-3, 4, size=(rows, c.C)).astype(F32)
        taps = r.randint(-2, 3, size=(c.O, c.C, c.K)).astype(F32)
        rot = _signed_permutations(r, c.n_rot, c.C) if c.n_rot else None
        return x, taps, rot, INT_HOP[c.rot_hop]
    x = (0.3 * r.normal(size=(rows, c.C))).astype(F32)
    taps = (0.3 * r.normal(size=(c.O, c.C, c.K)) * np.exp(-np.arange(c.K) / (c.K / 6.))).astype(F32)
    rot = None
    if c.n_rot:
        rot = np.stack([np.linalg.qr(r.normal(size=(c.C, c.C)))[0] for _ in range(c.n_rot)], 0).astype(F32)
    return x, taps, rot, c.rot_hop


def render_call(case, operands):
    """The keyword arguments after (x, n_hist, taps) shared by render_fir_fp32, render_ref and render_abs_sum."""
    x, taps, rot, hop = operands
    return (x, case.n_hist, taps), dict(rot=rot, rot_hop=hop, pos0=case.pos0, zero_before=case.zero_before)


# sources -------------------------------------------------------------------------------------------------------------------------
SourceCase = collections.namedtuple('SourceCase', 'name op scene S rate order distance_model t0 n K D zero_before seed')
ENC_T0, ENC_N, ENC_S = (0, 1, 255, 300), (1, 255, 256, 257, 700), (1, 3, 64)
HRIR_K, HRIR_D = (1, 3, 4, 7, 200, 512), (1, 65, 2048, 2049, 4096)
RADIUS = 0.5


def _source_case(name, op, scene='random', S=1, rate=48000, order=1, distance_model=0, t0=0, n=1, K=0, D=0, zero_before=0, seed=0):
    return SourceCase(name, op, scene, S, rate, order, distance_model, t0, n, K, D, zero_before, seed)


@functools.lru_cache(None)
def source_cases():
    out = []
    for i in range(10):
        kw = dict(S=ENC_S[i % 3], t0=ENC_T0[i % 4], n=ENC_N[i % 5])
        out.append(_source_case('encode_%d' % i, 'encode', order=1 + i % 2, distance_model=(i // 2) % 2, seed=100 + i, **kw))
        out.append(_source_case('mic_%d' % i, 'mic', scene='ear', seed=200 + i, **kw))
    for op in ('encode', 'mic', 'hrir'):
        extra = dict(K=7, D=65) if op == 'hrir' else {}
        # r == 0 at the last control point of the shortest source, reached by the call; an r that runs negative
        out.append(_source_case(op + '_r0_and_negative_r', op, scene='r0', S=3, order=2, t0=650 - 257, n=257, seed=300, **extra))
        # nframes 1 and 2 with P > 1
        out.append(_source_case(op + '_nframes1', op, scene='nframes1', S=3, order=1, t0=0, n=1, seed=310, **extra))
        out.append(_source_case(op + '_nframes2', op, scene='nframes2', S=3, order=2, t0=0, n=2, seed=320, **extra))
        # nframes == N - 1: the sample at N - 1 exists and must not be read
        out.append(_source_case(op + '_nframes_n_minus_1_48000', op, scene='n-1', S=1, rate=48000, order=1, distance_model=1, t0=0, n=26, seed=330, **extra))
        out.append(_source_case(op + '_nframes_n_minus_1_44100', op, scene='n-1', S=1, rate=44100, order=2, t0=1, n=13, seed=340, **extra))
    zero = lambda kind, K, t0: {0: 0, 1: K - 1, 2: t0 + 100}[kind]
    for i in range(10):
        K, t0 = HRIR_K[i % 6], (0, 100, 300)[i % 3]
        out.append(_source_case('hrir_%d' % i, 'hrir', S=1 + i % 3, t0=t0, n=ENC_N[(i + 1) % 5], K=K, D=HRIR_D[i % 5], zero_before=zero(i % 3, K, t0),
                                seed=400 + i))
    out.append(_source_case('hrir_k512_d4096', 'hrir', S=2, t0=100, n=257, K=512, D=4096, zero_before=200, seed=450))
    out.append(_source_case('hrir_k200_d2049', 'hrir', S=3, t0=300, n=700, K=200, D=2049, zero_before=199, seed=451))
    out.append(_source_case('hrir_second_chunk', 'hrir', scene='second_chunk', S=2, t0=1, n=256, K=7, D=4096, seed=460))
    out.append(_source_case('hrir_tie_across_chunks', 'hrir', scene='tie', S=2, t0=0, n=255, K=4, D=4096, seed=470))
    return tuple(out)


Scene = collections.namedtuple('Scene', 'signals cps dirs hrir')


def _path(r, P, r_lo=0.7, r_hi=2.0):
    return np.stack([r.uniform(-3., 3., P), r.uniform(-1.4, 1.4, P), r.uniform(r_lo, r_hi, P)], 1)


@functools.lru_cache(None)
def source_scene(case, integers=False):
    """The sources of a case: signals (fp32, one array per source, lengths that differ), control points, and for hrir the direction
    set and the table [D, 2, K].  Seeded; every radius stays outside RADIUS for the distance model."""
    c = case
    r = np.random.RandomState(c.seed)
    need = c.t0 + c.n
    if c.scene == 'nframes1':
        lengths, cps = [1, 5, 9], [_path(r, 3), _path(r, 2), _path(r, 1)]
    elif c.scene == 'nframes2':
        lengths, cps = [7, 2, 4], [_path(r, 1), _path(r, 2), _path(r, 4)]
    elif c.scene == 'n-1':
        lengths = [{48000: 27, 44100: 15}[c.rate]]       # so short that only a path of a few samples' delay is heard at all
        cps = [np.stack([r.uniform(1.2, 1.9, 3), r.uniform(-0.3, 0.3, 3), r.uniform(0.08, 0.2, 3)], 1) if c.op == 'mic' else _path(r, 3, 0.52, 0.62)]
        assert SO.nframes_of(lengths[0], c.rate) == lengths[0] - 1
    elif c.scene == 'r0':
        lengths = [need + 40, need, need + 3]
        cps = [_path(r, 4), np.concatenate([_path(r, 2), [[0.4, -0.2, 0.]]]), np.array([[2.0, 0.4, 0.9], [-1.0, -0.3, -0.4]])]
    else:
        lengths = [need + 11 + 7 * (k % 5) for k in range(c.S)]
        lengths[c.S // 2] = need                         # the call ends at the shortest source's last frame
        moving = 4 if c.S > 8 else c.S                   # (64 moving sources would make a rounding tie all but certain: 60 are static)
        cps = [_path(r, (3, 1, 5, 2, 4)[k % 5] if k < moving else 1) for k in range(c.S)]
        if c.scene == 'ear':
            cps[-1] = np.array([[np.pi / 2, 0., 0.12]])       # 2 cm from the left ear
    if c.scene in ('random', 'ear', 'r0', 'second_chunk', 'tie'):
        lengths = [N if SO.nframes_of(N, c.rate) >= need else N + 1 for N in lengths]       # (int(N / rate * rate) can be N - 1)
    assert len(lengths) == c.S and min(SO.nframes_of(N, c.rate) for N in lengths) >= need
    if integers:
        signals = [r.randint(-3, 4, size=N).astype(F32) for N in lengths]
    else:
        signals = [(0.3 * r.normal(size=N)).astype(F32) for N in lengths]
    if c.scene == 'n-1':
        signals[0][-1] = F32(-3 if integers else 1e6)    # not NaN, so that a read of it changes a value instead of hiding in a guard
    dirs = hrir = None
    if c.op == 'hrir':
        dirs = r.normal(size=(c.D, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        if c.scene in ('second_chunk', 'tie'):
            cps[0] = _path(r, 1)
            u = SO.track(cps[0], lengths[0], c.rate, np.array([0]))[1][0]
            dirs[3000] = u
            if c.scene == 'tie':
                dirs[100] = u
        if integers:
            hrir = r.randint(-2, 3, size=(c.D, 2, c.K)).astype(F32)
        else:
            hrir = (0.3 * r.normal(size=(c.D, 2, c.K)) * np.exp(-np.arange(c.K) / (c.K / 6.))).astype(F32)
    return Scene(tuple(signals), tuple(cps), dirs, hrir)


def source_restate(case, scene):
    c, s = case, scene
    if c.op == 'encode':
        return encode_fp32(s.signals, s.cps, c.rate, c.order, c.t0, c.n, bool(c.distance_model), RADIUS)
    if c.op == 'mic':
        return mic_fp32(s.signals, s.cps, c.rate, c.t0, c.n)
    return hrir_fp32(s.signals, s.cps, c.rate, s.dirs, s.hrir, c.zero_before, c.t0, c.n)


def source_ref(case, scene):
    """The fp64 oracle (sources_oracle) of the same call."""
    c, s = case, scene
    sig = [x.astype(np.float64) for x in s.signals]
    if c.op == 'encode':
        return SO.encode(sig, s.cps, c.rate, c.order, c.t0, c.n, bool(c.distance_model), RADIUS)
    if c.op == 'mic':
        return SO.mic(sig, s.cps, c.rate, c.t0, c.n)
    h = s.hrir.astype(np.float64)
    return SO.hrir(sig, s.cps, c.rate, s.dirs, h[:, 0], h[:, 1], c.zero_before, c.t0, c.n)


def source_bound(case, restated):
    """The elementwise bound of test_gpu_output_ops.py: (S + 4) u A for encode and mic, (n + 8) u A for hrir."""
    if case.op == 'hrir':
        return (restated.terms + 8) * U * restated.A
    return (case.S + 4) * U * restated.A


def render_bound(case, A, terms):
    """(n + 8) u A unrotated, (C K + C + 12) u A' rotated."""
    if case.n_rot:
        return (case.C * case.K + case.C + 12) * U * A
    return (terms + 8) * U * A
