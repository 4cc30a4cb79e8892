"""The layer-local trunk checks (trunk_oracle.py) proven on the host before they judge a kernel (test_gpu_trunk_layers.py): the CPU
emulation of conv3h_kernel's arithmetic stays inside the elementwise bound on benign and on adversarial data, and every planted fault
is caught by at least one of the two assertions the GPU test makes - the elementwise bound and the layer-local rel-RMS bar of 2e-5.
The geometries are the model's own at their smallest: stage 5 in full (B = 2, 7 x 14 x 512 -> 512) and stage 2 as a crop of 16 image
rows (B = 2, 16 x 112 x 64 -> 64).

Fault table (which assertion catches what, asserted below for both geometries and printed with the figures):
    (a) one tap dropped at one border pixel                        the elementwise bound (one of 10^3 .. 10^5 pixels: invisible to an RMS)
    (b) the activation lo plane dropped                            the rel-RMS bar       (2^-11 per term, incoherent: far inside a worst-case bound)
    (c) xl*wh dropped in one 16-channel chunk                      the rel-RMS bar
    (d) a row's closing zero pixel = the next row's first pixel    the elementwise bound
    (e) the last 37 rows of M left NaN                             the elementwise bound (an element that is not finite is outside it)
"""
import numpy as np
import pytest

import trunk_oracle as TO
import forward_oracle as FO

GEOMETRIES = {'stage5': (2, 7, 14, 512), 'stage2-crop16': (2, 16, 112, 64)}
EXPECTED = {'tap': 'elementwise', 'no_lo': 'rms', 'chunk_xlwh': 'rms', 'closing_pixel': 'elementwise', 'm_tail': 'elementwise'}


def _operands(geometry, kind):
    """(x float32 [B,H,W,C], w float32 [3,3,C,C], a_inv).  'bn': relu(gamma z + beta) as a batch-norm leaves it, under the scale the rule
    of DESIGN.md 3.2 derives from gamma and beta; 'adversarial': a third of the channels near zero, one channel x 100, so that under the
    scale the large channel dictates the small ones fall below fp16's normal range (6.1e-5)."""
    B, H, W, C = GEOMETRIES[geometry]
    r = np.random.default_rng(sum(map(ord, geometry + kind)))
    gamma, beta = r.uniform(0.5, 1.5, C), r.normal(0.0, 0.2, C)
    x = np.maximum(r.normal(size=(B, H, W, C)) * gamma + beta, 0.0)
    lim = np.sqrt(6.0 / (9 * C + 9 * C))
    w = r.uniform(-lim, lim, size=(3, 3, C, C))
    if kind == 'bn':
        a_inv = TO.rule_a_inv(*TO.bn_range(np.ones(C), B * H * W, gamma, beta))
    else:
        x[..., ::3] *= 1e-7
        x[..., 1] *= 100.0
        a_inv = TO.rule_a_inv(2.0 * float(x.max()), 0.0)
        assert 0 < float((x[..., ::3] / a_inv).max()) < 6.1e-5 and float(x.max()) / a_inv <= 65000.0
    return x.astype(np.float32), w.astype(np.float32), a_inv


@pytest.fixture(scope='module')
def layers():
    """Operands, reference and bound per (geometry, kind): computed once, never modified."""
    out = {}
    for g in GEOMETRIES:
        for kind in ('bn', 'adversarial'):
            x, w, a_inv = _operands(g, kind)
            out[g, kind] = (x, w, a_inv, TO.filter_inv_scale(w)) + TO.conv_layer(x, w, 1, 'h2', a_inv)
    return out


@pytest.mark.parametrize('kind', ['bn', 'adversarial'])
@pytest.mark.parametrize('geometry', list(GEOMETRIES))
def test_faithful_emulation_stays_inside_the_bound(layers, geometry, kind):
    x, w, a_inv, w_inv, ref, bound = layers[geometry, kind]
    assert TO.is_pow2(a_inv) and TO.is_pow2(w_inv) and 512 <= float(np.abs(w).max()) / w_inv < 1024
    res = TO.check_layer(TO.emulate_h2_conv(x, w, 1.0 / a_inv, 1.0 / w_inv), ref, bound)
    print('\n%s %s: rel-RMS %.2e, worst element %s at %.3g of its bound' % (geometry, kind, res['rel_rms'], res['at'], res['worst']))
    assert res['elementwise'] and res['rms'], res


@pytest.mark.parametrize('fault', TO.FAULTS)
@pytest.mark.parametrize('geometry', list(GEOMETRIES))
def test_every_planted_fault_is_caught(layers, geometry, fault):
    """A condition on the checks, not a measurement: a fault neither assertion sees means the checks are too weak."""
    x, w, a_inv, w_inv, ref, bound = layers[geometry, 'bn']
    res = TO.check_layer(TO.emulate_h2_conv(x, w, 1.0 / a_inv, 1.0 / w_inv, fault=fault), ref, bound)
    caught = [k for k in ('elementwise', 'rms') if not res[k]]
    print('\n%s %-62s caught by %-20s rel-RMS %.2e, worst element at %.3g of its bound' % (geometry, TO.FAULT_TEXT[fault], ' + '.join(caught) or 'NOTHING', res['rel_rms'], res['worst']))
    assert caught, (fault, res)
    assert EXPECTED[fault] in caught, (fault, caught, res)


def test_a_fault_free_run_of_another_block_size_is_not_a_fault(layers):
    """The bound covers any order and grouping of the fp32 sum: K blocks of 64 (KC = 4) and of 16 differ, both stay inside."""
    x, w, a_inv, w_inv, ref, bound = layers['stage5', 'bn']
    y16, y64 = (TO.emulate_h2_conv(x, w, 1.0 / a_inv, 1.0 / w_inv, block=b) for b in (16, 64))
    assert not np.array_equal(y16, y64)
    assert TO.check_layer(y64, ref, bound)['elementwise']


def test_split_then_decode_round_trips():
    r = np.random.default_rng(5)
    B, H, W, C = 2, 3, 5, 32
    v = (r.normal(size=(B, H, W, C)) * np.exp(r.uniform(-12, 3, size=(B, H, W, C)))).astype(np.float32)
    v[0, 0, 0, :4] = [0.0, -0.0, 2.0 ** -30, 1.0]
    sa = 2.0 ** 6
    hi, lo = TO.split_planes(v, sa)
    buf = TO.encode_planes(hi, lo)
    assert buf.dtype == np.float16 and buf.size == TO.plane_halfs(B, H, W, C)
    hi2, lo2, closing = TO.decode_planes(buf.view(np.uint16), B, H, W, C)               # (as the raw words a device buffer is read as)
    assert np.array_equal(hi2.view(np.uint16), hi.view(np.uint16)) and np.array_equal(lo2.view(np.uint16), lo.view(np.uint16))
    assert closing.shape == (C // 16, B, H, 2, 16) and not closing.view(np.uint16).any()
    # the layout itself: chunk, flat padded pixel, plane, channel within the chunk
    raw = buf.reshape(C // 16, B * H * (W + 1), 2, 16)
    assert raw[1, (1 * H + 2) * (W + 1) + 4, 0, 3] == hi[1, 2, 4, 19] and raw[1, (1 * H + 2) * (W + 1) + 4, 1, 3] == lo[1, 2, 4, 19]
    # the representation bound of the docstring: |v - (hi + lo) / sa| <= max(2^-22 |v|, 2^-25 / sa)
    back = (hi.astype(np.float64) + lo.astype(np.float64)) / sa
    assert (np.abs(v - back) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25 / sa)).all()
    assert hi[0, 0, 0, 3] == np.float16(64.0) and lo[0, 0, 0, 3] == 0


@pytest.mark.parametrize('shape', [(2, 7, 9, 5, 3, 3, 6, 1), (1, 9, 11, 4, 3, 3, 7, 2), (2, 5, 7, 6, 1, 1, 3, 2), (1, 11, 13, 3, 7, 7, 4, 2)])
def test_oracle_conv_equals_the_model_oracle(shape):
    from oracle.np_oracle import nn_convolution, max_pool_3x3_s2_same
    B, H, W, cin, kh, kw, cout, s = shape
    r = np.random.default_rng(H * W)
    x, w = r.normal(size=(B, H, W, cin)), r.normal(size=(kh, kw, cin, cout))
    want = nn_convolution(x, w, (s, s), 'SAME')
    got = FO.conv_ref(x, w, (s, s), 'SAME')
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    if kh == 3:        # ... and the pool of pool_layer is the model oracle's (scale 1, shift 0: relu(x))
        p, _ = TO.pool_layer(np.pad(x, ((0, 0), (0, H % 2), (0, W % 2), (0, 0))), 1.0, 0.0)
        assert np.array_equal(p, max_pool_3x3_s2_same(np.maximum(np.pad(x, ((0, 0), (0, H % 2), (0, W % 2), (0, 0))), 0.0)))


def test_stem_reference_in_space_to_depth_form_equals_the_direct_conv():
    r = np.random.default_rng(17)
    x, w = r.normal(size=(2, 12, 18, 3)), r.normal(size=(7, 7, 3, 5))
    want = FO.conv_ref(x, w, (2, 2), 'SAME')
    got = TO.stem_correlate(x, w)
    assert got.shape == want.shape == (2, 6, 9, 5) and np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # the uint8 form: conv(W, u') / 255 + (0.5 / 255) sum W with u' = -0.5 in the padding IS the conv of x = u / 255 - 0.5, zero padded
    u = r.integers(0, 256, size=(1, 8, 10, 3)).astype(np.uint8)
    ref, bound = TO.stem_layer(u, w, True)
    xf = u.astype(np.float64) / 255.0 - 0.5
    assert np.abs(ref - FO.conv_ref(xf, w, (2, 2), 'SAME')).max() <= 1e-13 * np.abs(ref).max()
    up = np.pad(u.astype(np.float64) - 128.0, ((0, 0), (2, 3), (2, 3), (0, 0)), constant_values=-0.5)
    A8 = FO._correlate((np.abs(up) + 0.5) / 255.0, np.abs(w), (2, 2), 'VALID')
    assert np.allclose(bound, (2 * 147 + 10) * TO.U * A8, rtol=1e-12)
    reff, boundf = TO.stem_layer(xf.astype(np.float32), w, False)
    assert (boundf >= (FO.conv_terms(xf.shape, w.shape, (2, 2), 'SAME') + 8) * TO.U * FO.conv_abs_ref(xf.astype(np.float32), w, (2, 2), 'SAME') * (1 - 1e-12)).all()


def test_scale_rule_and_accumulator_helpers():
    """rule_a_inv restates p3_tables: the statistical bound lands in [512, 1024) unless the rigorous one caps it at 64000."""
    for stat in (0.3, 1.0, 7.9, 8.0, 1000.0):
        a_inv = TO.rule_a_inv(stat, 0.0)
        assert TO.is_pow2(a_inv) and 512 <= stat / a_inv < 1024
    a_inv = TO.rule_a_inv(4.0, 4.0 * 300)            # sqrt(N) / 8 = 300: the rigorous bound decides
    assert TO.is_pow2(a_inv) and 32000 < 1200 / a_inv <= 64000 and 4.0 / a_inv < 512
    r = np.random.default_rng(9)
    y = r.normal(1.0, 2.0, size=(500, 64))
    acc = np.concatenate([y.sum(0), (y * y).sum(0)])
    sc, sh, var = TO.bn_coeffs(acc, 64, 500, np.full(64, 2.0), np.full(64, 0.5))
    z = y * sc + sh
    assert np.allclose(z.mean(0), 0.5) and np.allclose(z.var(0), 4.0 * var / (var + TO.BN_EPS))
    assert TO.stats_check(acc, 64, y) == 0.0
    acc[3] *= 1 + 1e-3
    assert TO.stats_check(acc, 64, y) > 1.0
