"""The CPU references on the degenerate inputs of tests/degenerate_cases.py - no GPU.  tests/test_gpu_degenerate.py holds the HIP
path to max(project bar, 4 x e32) on them, e32 being the float32 reference's error against the float64 one, so the references
themselves are pinned here: the two independent fp64 implementations agree, everything is finite, and e32 stays where it was measured.
If a change of a reference made e32 balloon, this module fails before a GPU bar silently loosens.  (B = 10 runs in the GPU module only.)"""
import numpy as np
import pytest

import degenerate_cases as D
from degenerate_cases import rms

_REFS = {}


def refs(name, B):
    if (name, B) not in _REFS:
        enc = D.CASES[name][1]
        inp = D.make(name, B)
        _REFS[(name, B)] = (inp,) + D.references(D.weights(enc), enc, inp)
    return _REFS[(name, B)]


def test_the_table_is_what_it_says():
    """every case really is degenerate in the way its name says, and is otherwise the random batch"""
    for name, B in D.case_ids():
        enc = D.CASES[name][1]
        inp, rnd = D.make(name, B), D.random_batch(B, enc)
        assert set(inp) == set(enc) and all(inp[k].shape == rnd[k].shape and inp[k].dtype == rnd[k].dtype for k in inp)
        assert inp['audio'].dtype == np.float32 and ('video' not in inp or inp['video'].dtype == np.uint8)
        changed = {k for k in inp if not np.array_equal(inp[k], rnd[k])}
        want = {'silence': {'audio'}, 'constant': {'video'}, 'still': {'flow'}, 'all': set(enc)}[D.CASES[name][0]]
        assert changed == want, (name, changed)
        if name in ('silent_window', 'one_black', 'one_still', 'all_one_window'):
            for k in changed:
                assert not inp[k][1].any() and all(np.array_equal(inp[k][i], rnd[k][i]) for i in range(B) if i != 1)
    assert not D.make('all', 2)['audio'].any() and not D.make('all', 2)['video'].any() and not D.make('all', 2)['flow'].any()
    assert set(np.unique(D.make('dark_lsb', 2)['video'])) == {0, 1}
    assert np.all(D.frames_float(D.make('black', 2)['video']) == np.float32(-0.5))
    assert sorted(D.E32_MEASURED) == sorted(D.case_ids())


# the second fp64 implementation on every case of the table
@pytest.mark.parametrize('name,B', D.case_ids(host_only=True))
def test_the_two_fp64_references_agree(name, B):
    from oracle.np_oracle import SptAudioGenOracle
    enc = D.CASES[name][1]
    inp, out64, ends64, _, _ = refs(name, B)
    orc = SptAudioGenOracle(encoders=list(enc))
    out = orc.inference_ops(inp['audio'], D.weights(enc), video=D.frames_float(inp['video']) if 'video' in inp else None, flow=inp.get('flow'))
    assert np.isfinite(out).all() and np.isfinite(out64).all()
    assert rms(out - out64) <= 1e-9, rms(out - out64)                        # (measured: 1e-16 .. 3e-12)
    for n in ('bottleneck', 'localization/coeffs'):
        a, b = np.asarray(orc.ends[n], np.float64).reshape(ends64[n].shape), ends64[n]
        assert np.isfinite(a).all() and rms(a - b) <= 1e-9 * max(1.0, rms(b)), (n, rms(a - b))


@pytest.mark.parametrize('name,B', D.case_ids(host_only=True))
def test_the_fp32_reference_error_stays_where_it_was_measured(name, B):
    _, out64, ends64, e32, e32_rel = refs(name, B)
    assert np.isfinite(out64).all() and all(np.isfinite(v).all() for v in ends64.values())
    assert np.isfinite(e32) and all(np.isfinite(v) for v in e32_rel.values())
    was = D.E32_MEASURED[(name, B)]
    assert was / 3.0 <= e32 <= 3.0 * was, 'fp32 reference error %.3g on %s at B = %d, measured %.3g' % (e32, name, B, was)
    if name in D.PROJECT_BAR_HOLDS:          # plain fp32 keeps the project's bars with room there: 4 x e32 decides none of them
        assert D.FACTOR * e32 <= min(D.ABS_TOL, D.REL_TOL * rms(out64))
        for n, e in e32_rel.items():
            assert D.FACTOR * e <= (D.TRUNK_TOL if n.endswith('conv5_2') else D.BOTTLENECK_TOL if n == 'bottleneck' else D.REL_TOL), (n, e)

