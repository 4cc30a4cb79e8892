"""tests/output_oracle.py without a device: fma32 against exact rational arithmetic, the fp32 restatements against the fp64 oracles
within the elementwise bounds of test_gpu_output_ops.py (printing the worst |err| / bound per family) and under its RMS bar, the
coverage of the case tables, and the input conditions of every case - a seed that fails one here is replaced, before any device
sees it."""
import fractions
import math

import numpy as np
import pytest

import output_oracle as OO
import sources_oracle as SO
from util import rel_rms_err

F32 = np.float32


def _round_f32(q):
    """The fp32 value nearest to the rational q, ties to even (normal and subnormal range)."""
    if q == 0:
        return 0.0
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = max(math.floor(math.log2(q)) - 1, -130)
    while fractions.Fraction(2) ** (e + 1) <= q:
        e += 1
    quantum = fractions.Fraction(2) ** (max(e, -126) - 23)
    m = q / quantum
    fl = m.numerator // m.denominator
    rem = m - fl
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return sign * float(fl * quantum)


def _exact(a, b, c):
    return np.array([_round_f32(fractions.Fraction(float(x)) * fractions.Fraction(float(y)) + fractions.Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)


def test_fma32_on_directed_ties():
    """p = +-h (1 + 2^-23)(1 - 2^-23) = +-h (1 - 2^-46) with h half an fp32 ulp of c: p + c lies 2^-70 |c| off a rounding tie, far below
    fp64's resolution, so s = fl64(p + c) IS the tie and float32(s) rounds it to even - wrong for half of the cases below."""
    a, b, c = [], [], []
    for scale in (1.0, 2.0 ** 20, 2.0 ** -60, 2.0 ** -120):
        h = scale * 2.0 ** -24
        for sa in (1.0, -1.0):
            for sc in (1.0, -1.0):
                for mant in range(8):
                    a.append(sa * h * (1 + 2.0 ** -23))
                    b.append(1 - 2.0 ** -23)
                    c.append(sc * scale * (1 + mant * 2.0 ** -23))
    a, b, c = (np.array(v, np.float64).astype(F32) for v in (a, b, c))
    want = _exact(a, b, c)
    got = OO.fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (naive.view(np.uint32) != want.view(np.uint32)).sum() >= len(a) // 4       # the cases do need the correction
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert OO.fma32(F32(3), F32(5), F32(-15)).view(np.uint32) == 0 and OO.fma32(F32(1.5), F32(2), F32(0.25)) == F32(3.25)


def test_fma32_on_random_operands():
    r = np.random.RandomState(1)
    n = 6000
    a = (r.normal(size=n) * 2.0 ** r.randint(-20, 20, n)).astype(F32)
    b = (r.normal(size=n) * 2.0 ** r.randint(-20, 20, n)).astype(F32)
    c = (r.normal(size=n) * 2.0 ** r.randint(-40, 40, n)).astype(F32)
    c[::3] = (-(a[::3].astype(np.float64) * b[::3]) * (1 + r.randint(-3, 4, len(c[::3])) * 2.0 ** -23)).astype(F32)      # cancellation
    c[1::7] = (a[1::7].astype(np.float64) * b[1::7] * 2.0 ** 24).astype(F32)                                        # p about half an ulp of c
    a[5::11] *= F32(2.0 ** -100)                                                                                  # subnormal results
    c[5::11] *= F32(2.0 ** -120)
    got, want = OO.fma32(a, b, c), _exact(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got2 = OO.fma32(a[:, None], b[None, :40], c[:, None])                # broadcasting
    assert np.array_equal(got2[:, 7].view(np.uint32), OO.fma32(a, np.full(n, b[7]), c).view(np.uint32))


# ---- the case tables ------------------------------------------------------------------------------------------------------------
def test_render_case_table_coverage():
    assert {OO.tap_paths(K) for K in OO.TAPS} == {(p, q) for p in range(4) for q in range(3)}
    assert {1, 2, 3, 511, 512} <= set(OO.TAPS)
    cases = OO.render_cases()
    assert len({c.name for c in cases}) == len(cases)
    for C in (4, 9):
        cs = [c for c in cases if c.C == C]
        assert {c.K for c in cs} >= set(OO.TAPS)
        assert {c.n for c in cs} >= set(OO.LENGTHS)
        assert {c.O for c in cs} >= set(OO.OUTPUTS)
        assert all(c.n <= 1100 for c in cs if c.K >= 511) and any(c.K == 512 and c.O == 32 for c in cs)
        for far in (False, True):                        # every history length at the start of a stream and far into one
            seen = {k for c in cs for k in OO.HIST_KINDS if c.n_hist == OO._n_hist(k, c.K) and (c.pos0 == OO.FAR) == far and (far or c.pos0 == c.n_hist)}
            assert seen == set(OO.HIST_KINDS), (C, far, seen)
        assert any(0 < c.n_hist < c.K - 1 and c.pos0 > c.n_hist for c in cs)           # a short history in mid-stream
        assert any(c.zero_before <= c.pos0 for c in cs) and any(c.zero_before >= c.pos0 + c.n for c in cs)
        assert any(c.zero_before == c.pos0 + 3 and c.n > 3 for c in cs)                # inside a lane
        assert any(c.zero_before == c.pos0 + 700 and c.n > 700 for c in cs)            # inside a tile
        rot = [c for c in cs if c.n_rot]
        assert {c.n_rot for c in rot} >= {1, 2, 5} and {c.rot_hop for c in rot} >= {1, 3, 8, 1000}
        seams = lambda c: [m * c.rot_hop for m in range(1, c.n_rot)]
        assert any(c.pos0 - min(c.n_hist, c.K - 1) <= s < c.pos0 for c in rot for s in seams(c))                      # inside the history rows
        assert any(c.pos0 < s < c.pos0 + c.n and (s - c.pos0) % 1024 for c in rot for s in seams(c))                # inside a tile
        assert any(c.n_rot > 1 and c.pos0 < (c.n_rot - 1) * c.rot_hop < c.pos0 + c.n for c in rot)                  # ends inside the call
        assert any(c.n_rot > 1 and (c.n_rot - 1) * c.rot_hop <= c.pos0 - c.n_hist for c in rot)                     # wholly past its end
        assert any(not c.n_rot for c in cs)
    assert all(c.rot_hop in OO.INT_HOP for c in cases if c.n_rot)
    assert all(c.C * c.K * 6 * max(OO.INT_HOP.values()) < 2 ** 24 for c in cases)      # the integer runs are exact


def test_source_case_table_coverage():
    cases = OO.source_cases()
    assert len({c.name for c in cases}) == len(cases)
    for op in ('encode', 'mic'):
        cs = [c for c in cases if c.op == op]
        assert {c.S for c in cs} >= set(OO.ENC_S) and {c.t0 for c in cs} >= set(OO.ENC_T0) and {c.n for c in cs} >= set(OO.ENC_N)
        assert {c.scene for c in cs} >= {'r0', 'nframes1', 'nframes2', 'n-1'}
    enc = [c for c in cases if c.op == 'encode']
    assert {(c.order, c.distance_model) for c in enc} >= {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert any(c.scene == 'ear' for c in cases if c.op == 'mic')
    assert {(c.rate, len(OO.source_scene(c).signals[0])) for c in cases if c.scene == 'n-1'} == {(48000, 27), (44100, 15)}
    h = [c for c in cases if c.op == 'hrir']
    assert {c.K for c in h} >= set(OO.HRIR_K) and {c.D for c in h} >= set(OO.HRIR_D)
    assert any(c.K % 4 == 0 for c in h) and any(c.K % 4 for c in h)                    # both kernel variants (and K % 4 == 0 runs both)
    assert any(c.D <= 2048 for c in h) and any(c.D > 2048 for c in h)                  # both chunk modes of the search
    assert any(c.K % 4 == 0 and c.D > 2048 for c in h) and any(c.K % 4 and c.D > 2048 for c in h)
    assert {c.scene for c in h} >= {'second_chunk', 'tie'}
    assert any(c.S > 1 for c in h) and any(c.t0 % 256 and c.t0 < c.K - 1 for c in h)    # t - k reaches before 0 from a t0 off the tile
    assert any(c.zero_before == 0 for c in h) and any(c.zero_before == c.K - 1 > 0 for c in h)
    assert any(c.t0 < c.zero_before < c.t0 + min(c.n, 256) for c in h)                 # mid-workgroup
    for c in h:
        if c.scene in ('second_chunk', 'tie'):
            s = OO.source_scene(c)
            near = SO.nearest_all(s.dirs, SO.track(s.cps[0], len(s.signals[0]), c.rate, np.arange(c.t0, c.t0 + c.n))[1])[0]
            assert (near == (100 if c.scene == 'tie' else 3000)).all()


# ---- the restatements against the fp64 oracles ------------------------------------------------------------------------------------
WORST = {}


def _hold(family, name, y, ref, bound):
    err = np.abs(y.astype(np.float64) - ref)
    assert (err <= bound).all(), (name, 'the restatement misses the elementwise bound', float((err / np.maximum(bound, 1e-300)).max()))
    assert not y[bound == 0].any(), name
    rms = rel_rms_err(y, ref)
    assert rms <= OO.RMS_BAR, (name, 'the restatement misses the RMS bar: choose another seed', rms)
    frac = float(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.).max())
    if frac > WORST.get(family, (-1., ''))[0]:
        WORST[family] = (frac, name)
    return frac


@pytest.mark.parametrize('case', OO.render_cases(), ids=lambda c: c.name)
def test_render_restatement_against_fp64(case):
    args, kw = OO.render_call(case, OO.render_operands(case))
    A, terms = OO.render_abs_sum(*args, **kw)
    y, ref = OO.render_fir_fp32(*args, **kw), OO.render_ref(*args, **kw)
    assert y.shape == ref.shape == (case.n, case.O)
    assert (A.any() and np.abs(ref).max() > 1e-3) != case.name.endswith('all_zeroed')         # every other case checks values, not zeros
    frac = _hold('render rotated' if case.n_rot else 'render', case.name, y, ref, OO.render_bound(case, A, terms))
    print('%s: worst |err| / bound %.3g' % (case.name, frac))
    # and the integer operands are exact: the fp32 restatement equals the fp64 reference
    args, kw = OO.render_call(case, OO.render_operands(case, True))
    assert np.array_equal(OO.render_fir_fp32(*args, **kw).astype(np.float64), OO.render_ref(*args, **kw))


@pytest.mark.parametrize('case', OO.source_cases(), ids=lambda c: c.name)
def test_source_restatement_against_fp64(case):
    scene = OO.source_scene(case)
    restated = OO.source_restate(case, scene)
    assert restated.cond.problems() == [], (case.name, 'choose another seed')          # (e), for every case
    ref = OO.source_ref(case, scene)
    frac = _hold(case.op, case.name, restated.y, ref, OO.source_bound(case, restated))
    print('%s: worst |err| / bound %.3g; tie distance %.3g relative, %.3g absolute; delay margin %.3g'
          % (case.name, frac, restated.cond.tie_rel, restated.cond.tie_abs, restated.cond.delay))
    if case.op == 'hrir':
        ints = OO.source_scene(case, True)
        assert OO.source_restate(case, ints).cond.problems() == []
        assert np.array_equal(OO.source_restate(case, ints).y.astype(np.float64), OO.source_ref(case, ints))
    if case.scene == 'r0':                               # the r == 0 control point is reached, and r does run negative
        t = np.arange(case.t0, case.t0 + case.n)
        r = [SO.track(cp, len(x), case.rate, t)[0][:, 2] for cp, x in zip(scene.cps, scene.signals)]
        assert r[1][-1] == 0. and (r[1][:-1] > 0).all() and (r[2] < 0).any() and (r[2] > 0).any()
    if case.scene == 'n-1':                              # the sample at N - 1 is loud and is not part of any output
        assert abs(float(scene.signals[0][-1])) == 1e6 and np.abs(ref).max() < 10. and np.abs(ref).max() > 0


def test_closed_form_harmonics_equal_the_legendre_form():
    u = np.random.RandomState(2).normal(size=(500, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for order in (1, 2):
        assert np.abs(OO.harmonics_closed(u, order) - SO.harmonics(u, order)).max() <= 1e-14


def test_worst_ratios_are_reported():
    """Runs after the sweeps above: the worst |err| / bound per family, for DESIGN.md section 4."""
    for family in sorted(WORST):
        print('worst |err| / bound, %s: %.3g (%s)' % ((family,) + WORST[family]))
    assert WORST
