"""Moving point sources on the device (csrc/sources.hip through ops.source_track / encode_sources / binauralize_sources and
sources.SourceScene) against the fp64 oracle (tests/sources_oracle.py), and the drivers on top: the source maps, the tie to the
power map, and the two command lines.

Bars.  Directions: 1e-12 absolute - fp64 sin / cos differ by ulps (~1e-16) between libraries and the angles stay below 10 rad, which
leaves three orders of margin.  Nearest indices: exact (the test first shows that no sample is ambiguous).  Sample sums: relative RMS
error <= 1e-5 against the oracle, the bar and basis of tests/test_gpu_render.py (an fp32 restatement of a 200-term sum with one
sequential accumulator measures 6e-7).  A stream cut into pieces must equal the one-call result BIT FOR BIT.  What the RMS bar does
not see - one wrong sample, the one-tap-at-a-time hrir variant, the two-chunk direction search and its ties, nframes == N - 1 - is
held by tests/test_gpu_output_ops.py: the fp32 sums bit for bit in the header's order, an elementwise bound, integer known answers.

Base shape: rate 48000; three sources of 12000, 12001 and 11999 samples (not multiples of the 256-sample tile: the last workgroup
is partial) - one static, one with two control points crossing phi = +-pi the long way, one with five whose nu runs past pi / 2, with
an r = 0 control point (next to which the interpolated r turns slightly negative) and a position 2 cm from the left ear.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_sources.py)."""
import functools

import numpy as np
import pytest

import render_oracle as RO
import sources_oracle as SO
from util import rel_rms_err, ensure_lib

pytestmark = pytest.mark.gpu

BAR = 1e-5
UNIT_BAR = 1e-12
RATE = 48000
LENGTHS = (12000, 12001, 11999)
CONTROL = (np.array([[0.7, -0.3, 1.5]]),
           np.array([[3.0, 0.2, 2.0], [-3.0, -0.4, 1.2]]),
           np.array([[-1.0, 0.3, 1.0], [0.5, 1.8, 0.8], [1.2, 0.5, 0.0], [np.pi / 2, 0.0, 0.12], [2.5, -0.6, 1.4]]))
# the same paths kept outside a sphere of radius 0.5, for the distance model (encode_v2 refuses a source inside it)
CONTROL_FAR = CONTROL[:2] + (np.array([[-1.0, 0.3, 1.0], [0.5, 1.8, 0.8], [1.2, 0.5, 0.6], [np.pi / 2, 0.0, 0.9], [2.5, -0.6, 1.4]]),)
N = min(SO.nframes_of(n, RATE) for n in LENGTHS)
OP_CASES = ('test_track_unit or test_track_nearest or test_encode_matches_oracle or test_binauralize_matches_oracle or '
            'test_pieces_are_bit_identical or test_limits')


def _dev():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    if _lib.IS_CPU_TWIN:
        return 'cpu'
    import torch
    assert torch.cuda.is_available()
    return 'cuda'


@functools.lru_cache(None)
def _signals():
    """Seeded noise plus a chirp per source, fp32-representable (as test_gpu_render._signal)."""
    out = []
    for k, n in enumerate(LENGTHS):
        t = np.arange(n) / float(RATE)
        x = 0.2 * np.random.RandomState(11 + k).normal(size=n) + 0.5 * np.sin(2 * np.pi * (300. + 2000. * t) * t)
        out.append(x.astype(np.float32))
    return tuple(out)


@functools.lru_cache(None)
def _hrirs():
    return RO.make_hrirs(41)


@functools.lru_cache(None)
def _scene(far=False):
    from spatialaudiogen_amd import sources
    return sources.SourceScene(list(_signals()), list(CONTROL_FAR if far else CONTROL), RATE, device=_dev())


@functools.lru_cache(None)
def _hset():
    from spatialaudiogen_amd import render as R
    return R.HrirSet(*_hrirs(), rate=RATE)


@functools.lru_cache(None)
def _ref(kind, *key):
    """The oracle's result of one case, computed once."""
    sig = [s.astype(np.float64) for s in _signals()]
    if kind == 'encode':
        order, dm = key
        return SO.encode(sig, CONTROL_FAR if dm else CONTROL, RATE, order, 0, N, bool(dm), 0.5)
    if kind == 'mic':
        return SO.mic(sig, CONTROL, RATE, 0, N)
    dirs, left, right = _hrirs()
    return SO.hrir(sig, CONTROL, RATE, dirs, left, right, key[0], 0, N)


# ---- op level -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 4800])
def test_track_unit(stride):
    assert N == 11999
    scene = _scene()
    got = scene.directions(stride).cpu().numpy()
    at = np.arange(0, N, stride)
    ref = np.stack([SO.track(cp, n, RATE, at)[1] for cp, n in zip(CONTROL, LENGTHS)], 1)
    assert got.shape == ref.shape == (len(at), 3, 3) and got.dtype == np.float64
    err = np.abs(got - ref).max()
    print('track unit, stride %d: max abs err %.3g (bar %.0e)' % (stride, err, UNIT_BAR))
    assert err <= UNIT_BAR
    if stride == 1:
        r = SO.track(CONTROL[2], LENGTHS[2], RATE, at)[0][:, 2]
        assert (r < 0).any() and (r > 0).any()             # the shape does exercise the sign rule


@pytest.mark.parametrize('which', ['random64', 'cipic1150'])
def test_track_nearest(which):
    import torch
    from spatialaudiogen_amd import ops
    if which == 'random64':
        dirs = np.random.RandomState(5).normal(size=(64, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    else:
        dirs = _hrirs()[0]
        assert dirs.shape == (1150, 3) and (dirs[:, 2] > 1 - 1e-15).sum() == 23             # the coincident zenith directions
    scene = _scene()
    at = np.arange(N)
    ref, ties_seen = [], 0
    for cp, n in zip(CONTROL, LENGTHS):
        idx, margin, dots = SO.nearest_all(dirs, SO.track(cp, n, RATE, at)[1])
        below = dots.max(1, keepdims=True) - dots
        assert not ((below > 1e-13) & (below < 1e-9)).any(), 'a sample of the test trajectory is ambiguous: choose another trajectory'
        ties_seen += int(((below <= 1e-13).sum(1) > 1).sum())
        ref.append(idx)
    ref = np.stack(ref, 1)
    got = ops.source_track(scene.table, 0, N, 1, torch.as_tensor(dirs).to(scene.device), unit=False)[1].cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.int32
    print('track nearest %s: %d of %d indices differ; %d samples resolved by the tie rule' % (which, (got != ref).sum(), ref.size, ties_seen))
    assert np.array_equal(got, ref)
    if which == 'cipic1150':
        assert ties_seen > 0


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('distance_model', [0, 1])
def test_encode_matches_oracle(order, distance_model):
    got = _scene(bool(distance_model)).encode(order, distance_model=bool(distance_model), radius=0.5).cpu().numpy()
    ref = _ref('encode', order, distance_model)
    assert got.shape == ref.shape == (N, (order + 1) ** 2) and got.dtype == np.float32
    err = rel_rms_err(got, ref)
    print('encode order %d distance_model %d: rel rms err %.3g (bar %.0e)' % (order, distance_model, err, BAR))
    assert err <= BAR
    if distance_model:
        with pytest.raises(ValueError):
            _scene().encode(order, distance_model=True, radius=0.5)          # the base shape passes through the origin


@pytest.mark.parametrize('mode,static', [('mic', False), ('hrir', False), ('hrir', True)])
def test_binauralize_matches_oracle(mode, static):
    K = _hrirs()[1].shape[1]
    zb = K - 1 if static else 0
    got = _scene().binauralize(mode, _hset() if mode == 'hrir' else None, static=static).cpu().numpy()
    ref = _ref('mic') if mode == 'mic' else _ref('hrir', zb)
    assert got.shape == ref.shape == (N, 2) and got.dtype == np.float32
    err = rel_rms_err(got, ref)
    print('binauralize %s zero_before %d: rel rms err %.3g (bar %.0e)' % (mode, zb, err, BAR))
    assert err <= BAR
    if mode == 'hrir':
        assert not got[:zb].any() and got[zb].any() and got[zb:].any()


@pytest.mark.parametrize('what', ['encode', 'mic', 'hrir'])
def test_pieces_are_bit_identical(what):
    scene = _scene()
    run = {'encode': lambda t0, n: scene.encode(2, t0, n),
           'mic': lambda t0, n: scene.binauralize('mic', t0=t0, n=n),
           'hrir': lambda t0, n: scene.binauralize('hrir', _hset(), static=True, t0=t0, n=n)}[what]
    whole = run(0, N).cpu().numpy()
    cuts = [1, 255, 4097]
    cuts.append(N - sum(cuts))
    out, t0 = [], 0
    for n in cuts:
        out.append(run(t0, n).cpu().numpy())
        t0 += n
    assert np.array_equal(whole.view(np.uint32), np.concatenate(out, 0).view(np.uint32))


def test_limits():
    import ctypes as C
    import torch
    from spatialaudiogen_amd import _lib, ops
    dev = _dev()
    sig = torch.zeros(1, 64, dtype=torch.float32, device=dev)
    one = ops.SourceTable([[[0., 0., 1.]]], [64], RATE, dev)

    def code(fn, *a, **k):
        with pytest.raises(_lib.SagenError) as e:
            fn(*a, **k)
        return e.value.code

    assert code(ops.encode_sources, sig, one, 5, 0, 8) == -3                                   # channels
    many = ops.SourceTable([[[0., 0., 1.]]] * 65, [64] * 65, RATE, dev)
    assert code(ops.encode_sources, torch.zeros(65, 64, dtype=torch.float32, device=dev), many, 4, 0, 8) == -3
    assert code(ops.source_track, many, 0, 8) == -3
    dirs = torch.zeros(4, 3, dtype=torch.float64, device=dev)
    dirs[:, 0] = 1.
    assert code(ops.binauralize_sources, sig, one, 'hrir', 0, 8, dirs, torch.zeros(4, 2, 513, dtype=torch.float32, device=dev)) == -3
    big = torch.zeros(4097, 3, dtype=torch.float64, device=dev)
    assert code(ops.binauralize_sources, sig, one, 'hrir', 0, 8, big, torch.zeros(4097, 2, 4, dtype=torch.float32, device=dev)) == -3
    assert code(ops.source_track, one, 0, 8, 1, big) == -3
    assert code(ops.encode_sources, sig, one, 4, 60, 8) == -2                                  # past the source's last frame
    l = _lib.lib()
    assert l.sagen_encode_sources(*((C.c_void_p(sig.data_ptr()), 64) + one.args() + (4, 0, 1., 0, 8, None, None))) == -1
    assert l.sagen_binauralize_sources(*((C.c_void_p(sig.data_ptr()), 64) + one.args() + (0, None, None, 0, 0, 0, 0, 8, None, None))) == -1
    assert l.sagen_source_track(*(one.args() + (0, 8, 1, None, 0, None, None, None))) == -1
    # and the supported edges still run: D = 4096 in two chunks of the search with K = 512, and a K that is no multiple of 4 (the
    # taps are then loaded one at a time)
    x = np.random.RandomState(6).normal(size=700).astype(np.float32)
    cp = np.array([[0.3, -0.2, 1.0], [2.9, 1.0, 1.0]])
    tab = ops.SourceTable([cp], [700], RATE, dev)
    for D, K in ((4096, 512), (65, 7)):
        d = np.random.RandomState(3).normal(size=(D, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        h = (np.random.RandomState(4).normal(size=(D, 2, K)) * 0.1).astype(np.float32)
        got = ops.binauralize_sources(torch.as_tensor(x[None]).to(dev), tab, 'hrir', 0, 700, torch.as_tensor(d).to(dev), torch.as_tensor(h).to(dev)).cpu().numpy()
        ref = SO.hrir([x.astype(np.float64)], [cp], RATE, d, h[:, 0].astype(np.float64), h[:, 1].astype(np.float64), 0, 0, 700)
        err = rel_rms_err(got, ref)
        print('hrir D = %d K = %d: rel rms err %.3g (bar %.0e)' % (D, K, err, BAR))
        assert err <= BAR


# ---- driver level (needs the device) ----------------------------------------------------------------------------------------------
def test_source_maps_equal_the_oracle():
    import torch
    assert torch.cuda.is_available()
    got = _scene().source_maps(2.5, 10., 5)
    ref = SO.source_maps(CONTROL, 2.5, 10., 5)
    assert got.shape == ref.shape == (25, 37, 72)
    assert np.array_equal(got, ref) and np.allclose(got.sum((1, 2)), 1.)


def test_static_source_lands_on_its_power_map_node():
    """A static first-order source encoded at a mesh node puts the maximum of ops.power_map on that node: the new front end meets the
    existing back end."""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import ambisonics, ops, sources
    phi, nu = ambisonics.spherical_mesh(5.)
    node = 11 * 72 + 20                                       # elevation row 11 (-35 degrees), azimuth column 20
    x = _signals()[0][:4800]
    scene = sources.SourceScene([x], [[[phi.reshape(-1)[node], nu.reshape(-1)[node], 1.3]]], RATE)
    ambi = scene.encode(1)
    rms = ops.power_map(ambi.contiguous(), torch.as_tensor(ambisonics.sh_matrix(5.).astype(np.float32)).cuda()).cpu().numpy()
    assert int(rms.argmax()) == node


def test_encode_command_line(tmp_path):
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import feeder as F, sources
    sig = [0.4 * s[:9000 + 7 * k] for k, s in enumerate(_signals())] + [0.05 * _signals()[0][:9500]]
    names = ['a.wav', 'b.wav', 'c.wav', 'amb.wav']
    for name, s in zip(names, sig):
        F.save_wav(str(tmp_path / name), s[:, None], RATE, subtype='FLOAT')
    with open(str(tmp_path / 'pos.txt'), 'w') as f:
        f.write('<BGI>room.jpg<BGI>.\n')
        for k, (name, cp) in enumerate(zip(names, list(CONTROL) + [np.zeros((0, 3))])):
            f.write('s%d %s img%d.png %d\n' % (k, name, k, len(cp)))
            for p in cp:
                f.write('%r %r %r\n' % tuple(float(v) for v in p))
    out_fn = str(tmp_path / 'ambix.wav')
    sources.main(['encode', str(tmp_path / 'pos.txt'), '2', out_fn, '--rate', str(RATE)])
    got, rate = F.load_wav(out_fn)
    assert rate == RATE and got.shape == (9500, 9)
    scene = sources.SourceScene(sig, list(CONTROL) + [np.zeros((0, 3))], RATE)
    L = scene.length
    assert 8999 <= L <= 9000
    ref = np.zeros((9500, 9))
    ref[:L] = scene.encode(2).cpu().numpy()
    ref[L:, 0] = sig[3][L:]
    ref = ref / ref.max() * 0.95
    assert abs(got.max() * 32768. / 32767. - 0.95) <= 1. / 32767.                  # the peak sits at 0.95 of full scale
    assert np.array_equal(got, np.rint(np.clip(ref, -1, 1) * 32767.) / 32768.)     # save_wav rounds to PCM16, load_wav divides by 32768
    with pytest.raises(SystemExit):
        sources.main(['encode', str(tmp_path / 'pos.txt'), '2', out_fn, '--rate', str(RATE)])         # exists, no --overwrite
    with pytest.raises(SystemExit):
        sources.main(['encode', str(tmp_path / 'pos.txt'), '2', out_fn, '--rate', '24000', '--overwrite'])   # no resampler


def test_binauralize_command_line(tmp_path):
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from spatialaudiogen_amd import feeder as F, sources
    dirs, left, right = _hrirs()
    RO.write_cipic_dir(str(tmp_path / 'hrir'), left, right, RATE)
    x = 0.1 * _signals()[2][:6001]
    F.save_wav(str(tmp_path / 'mono.wav'), x[:, None], RATE, subtype='FLOAT')
    n = SO.nframes_of(6001, RATE)
    for name, cp, zb in (('moving', CONTROL[2], 0), ('static', CONTROL[0], left.shape[1] - 1)):
        with open(str(tmp_path / (name + '.txt')), 'w') as f:
            for p in cp:
                f.write('%r %r %r\n' % tuple(float(v) for v in p))
        out_fn = str(tmp_path / (name + '.wav'))
        sources.main(['binauralize', str(tmp_path / 'mono.wav'), str(tmp_path / (name + '.txt')), out_fn, '--use_hrtfs', '--hrtf_dir', str(tmp_path / 'hrir'),
                      '--float'])
        got, rate = F.load_wav(out_fn)
        ref = np.zeros((6001, 2))
        ref[:n] = SO.hrir([x.astype(np.float64)], [cp], RATE, dirs, left, right, zb, 0, n)
        assert rate == RATE and got.shape == ref.shape
        err = rel_rms_err(got, ref)
        print('binauralize CLI %s: rel rms err %.3g (bar %.0e)' % (name, err, BAR))
        assert err <= BAR
        assert not got[:zb].any() and got[zb].any() and not got[n:].any()
    out_fn = str(tmp_path / 'mic.wav')
    sources.main(['binauralize', str(tmp_path / 'mono.wav'), str(tmp_path / 'moving.txt'), out_fn])
    got, _ = F.load_wav(out_fn)
    ref = np.zeros((6001, 2))
    ref[:n] = SO.mic([x.astype(np.float64)], [CONTROL[2]], RATE, 0, n)
    assert np.abs(got - ref).max() <= 1.5 / 32768.
