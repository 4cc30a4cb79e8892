"""The polyphase resampler and the windowed RMS on the device (csrc/resample.hip through ops.resample_fir / ops.window_rms /
resample.Resampler and the command lines) against the fp64 restatement of tests/resample_oracle.py, which is written from the
definition, imports nothing of the package and knows nothing of the phase table's layout.

COMPARISON RULE.  With ref = the restatement's fp64 value: every output is within one fp32 spacing of float32(ref), and it IS
float32(ref), bit for bit, wherever ref lies further than 2^-40 |ref| from an fp32 rounding tie.  The share of outputs nearer to a tie
than that is a condition on the INPUT, asserted on the restatement alone: at most 1e-3 per case (for random input about 2^-16 is
expected; the seeds below meet it).

RMS.  Against numpy's fp64 sqrt(mean(x^2)) to 1e-12 relative: both sum exact squares of fp32 values in fp64 in different orders, at
most ~5000 terms of one sign, so the two differ by a few 1e-16 relative at the worst.

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_resample.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_oracle as RO
from util import ensure_lib

pytestmark = pytest.mark.gpu

OP_CASES = 'test_parity or test_one_shot or test_windows or test_streaming or test_refusals or test_window_rms or test_hrir_set'
TIE = 2. ** -40
SMALL = (4, 5.0, 0.8)                 # a filter short enough that both stream ends and the T padding matter at every size below
RATIOS = [(7, 5), (3, 4), (147, 160), (3, 1)]            # rate_in, rate_out: L / M = 5/7, 4/3, 160/147, 1/3
SIZES = [1, 2, 33, 700]
DENSE = np.random.RandomState(77).uniform(-1., 1., (2, 9))
# Output 0 is h[0] x[0] = (L rolloff / q) x[0], a ratio of small integers times an fp32 value: for about one x[0] in a hundred that
# product is short enough to sit EXACTLY on an fp32 rounding tie, and a case of one or two rows then misses the input condition.  Of
# the bases 0 .. 7 tried for SEED + 1000 N_in + C, 600000 is the first for which the restatement alone meets it in every case below.
SEED = 600000
# channels, mix
CHANNEL_CASES = [(1, None), (4, None), (9, None), (9, 'map'), (9, 'dense')]


def _dev():
    from spatialaudiogen_amd import _lib
    ensure_lib()
    if _lib.IS_CPU_TWIN:
        return 'cpu'
    import torch
    assert torch.cuda.is_available()
    return 'cuda'


def _t(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _mix(kind):
    from spatialaudiogen_amd import resample as R
    return None if kind is None else (R.mix_from_map([2, 1, 4, 0], 9) if kind == 'map' else DENSE)


def _x(n, c, seed):
    return np.random.RandomState(seed).uniform(-1., 1., (n, c)).astype(np.float32)


def assert_matches(got, ref, what):
    """The comparison rule of the module docstring; prints its figures before it asserts."""
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    want = ref.astype(np.float32)
    near = RO.tie_distance(ref) < TIE
    share = near.mean() if near.size else 0.
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    differ = int((got != want).sum())
    print('%s: %d outputs, %d near a tie (share %.2g), %d differ from float32(ref), max |got - float32(ref)| %.3g' % (what, ref.size, near.sum(), share, differ, d.max() if d.size else 0.))
    assert share <= 1e-3, (what, 'the input puts too many outputs on a rounding tie')
    assert np.isfinite(got).all()
    assert (d <= np.spacing(np.abs(want)).astype(np.float64)).all(), what
    assert np.array_equal(got[~near], want[~near]), what


def _run(x, rates, quality, mix, n0=0, n=None, x0=0, rows=None, periods=0):
    """ops.resample_fir on the rows x0 .. x0 + rows - 1 of the stream x for the outputs n0 .. n0 + n - 1; periods: the same rows and
    outputs `periods` periods further into a stream (a period is M rows and L outputs)."""
    from spatialaudiogen_amd import ops, resample as R
    dev = _dev()
    L, M, H, taps = R.design(rates[0], rates[1], quality)
    if n is None:
        n = R.output_length(x.shape[0], L, M) - n0
    buf = x[x0:x0 + rows] if rows is not None else x[x0:]
    return ops.resample_fir(_t(buf, dev), x0 + periods * M, _t(taps, dev), L, M, H, n0 + periods * L, n, None if mix is None else _t(mix, dev)).cpu().numpy()


@pytest.mark.parametrize('quality', [SMALL, 'fast'], ids=['small', 'fast'])
@pytest.mark.parametrize('rates', RATIOS, ids=['7to5', '3to4', '147to160', '3to1'])
def test_parity(rates, quality):
    for n_in in SIZES:
        for c, kind in CHANNEL_CASES:
            x, mix = _x(n_in, c, SEED + 1000 * n_in + c), _mix(kind)
            ref = RO.direct(x, rates[0], rates[1], quality, mix)
            L, M, _, _ = RO.filt(rates[0], rates[1], quality)
            assert ref.shape == (-(-n_in * L // M), c if mix is None else mix.shape[0])
            assert_matches(_run(x, rates, quality, mix), ref, '%d -> %d, N_in %d, C %d, mix %s' % (rates[0], rates[1], n_in, c, kind))


def test_one_shot():
    """resample.resample: numpy in, numpy out; a tensor in, a tensor out; one channel as a 1-D array; an empty stream."""
    from spatialaudiogen_amd import resample as R
    dev = _dev()
    x = _x(300, 4, 3)
    ref = RO.direct(x, 44100, 48000, 'fast')
    got = R.resample(x, 44100, 48000, quality='fast')
    assert isinstance(got, np.ndarray)
    assert_matches(got, ref, 'one-shot 44100 -> 48000')
    t = R.resample(_t(x, dev), 44100, 48000, quality='fast')
    assert t.device.type == dev and np.array_equal(t.cpu().numpy(), got)
    mono = R.resample(x[:, 0], 44100, 48000, quality='fast')
    assert mono.shape == (ref.shape[0],) and np.array_equal(mono, got[:, 0])
    assert R.resample(x[:0], 44100, 48000).shape == (0, 4)
    mix = R.mix_fuma_to_ambix(1)
    assert_matches(R.resample(x, 48000, 48000, mix=mix), RO.direct(x, 48000, 48000, 'best', mix), 'equal rates with a mix')


# ---- windows of a stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rates,quality', [((147, 160), 'fast'), ((3, 1), SMALL), ((3, 4), SMALL)], ids=['147to160', '3to1', '3to4'])
def test_windows(rates, quality):
    x = _x(700, 4, 21)
    L, M, H, _ = RO.filt(rates[0], rates[1], quality)
    whole = _run(x, rates, quality, None)
    assert_matches(whole, RO.direct(x, rates[0], rates[1], quality), 'the whole stream')
    n_out = whole.shape[0]
    rs = np.random.RandomState(5)
    # windows whose buffer holds every row their outputs reach: the slice of the whole-stream result, bit for bit
    for _ in range(12):
        n0 = int(rs.randint(0, n_out))
        n = int(rs.randint(1, n_out - n0 + 1))
        lo, hi = max(0, -((H - n0 * M) // L)), min(699, ((n0 + n - 1) * M + H) // L)
        x0 = int(rs.randint(0, lo + 1))
        rows = int(rs.randint(hi + 1 - x0, 700 - x0 + 1))
        got = _run(x, rates, quality, None, n0, n, x0, rows)
        assert np.array_equal(got, whole[n0:n0 + n]), (n0, n, x0, rows)
    # far into a stream, up to the 2^40 the header allows: a whole number of periods further on no phase and no tap changes, so
    # neither do the bits (the positions and n M no longer fit 32 bits)
    for periods in (((1 << 31) + 5) // min(L, M), ((1 << 40) - 2000) // max(L, M)):
        assert np.array_equal(_run(x, rates, quality, None, n_out // 4, n_out // 2, 100, 300, periods), _run(x, rates, quality, None, n_out // 4, n_out // 2, 100, 300))
    # windows whose buffer lacks rows: as if those rows of the stream were zero
    for n0, n, x0, rows in [(0, n_out, 5, 100), (n_out // 3, n_out // 3, 350, 1), (0, 7, 600, 100), (n_out - 3, 3, 0, 10), (10, 50, 40, 0),
                            (n_out + 40, 25, 690, 10)]:
        seen = np.zeros(700, bool)
        seen[x0:x0 + rows] = True
        zeroed = _run(np.where(seen[:, None], x, np.float32(0)), rates, quality, None, n0, n)
        got = _run(x, rates, quality, None, n0, n, x0, rows)
        assert np.array_equal(got, zeroed), (n0, n, x0, rows)
        assert_matches(got, RO.direct(x, rates[0], rates[1], quality, None, n0, n, x0, rows), 'window n0 %d n %d x0 %d rows %d' % (n0, n, x0, rows))


# ---- streaming -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('quality', [SMALL, 'fast'], ids=['small', 'fast'])
@pytest.mark.parametrize('rates', RATIOS, ids=['7to5', '3to4', '147to160', '3to1'])
def test_streaming(rates, quality):
    from spatialaudiogen_amd import resample as R
    dev = _dev()
    for n_in, c, kind in ((700, 9, 'map'), (700, 4, None), (41, 1, None), (2, 4, None)):
        x, mix = _x(n_in, c, 9), _mix(kind)
        whole = _run(x, rates, quality, mix)
        r = R.Resampler(rates[0], rates[1], c, mix, quality)
        assert r.device.type == dev
        for attempt in range(2):                       # the second time after reset(): a new stream, the same rows
            out, i = [], 0
            for piece in (1, 2, 37, n_in):
                if i < n_in:
                    out.append(r.process(_t(x[i:i + piece], dev)))
                    i += piece
            assert r.seen == n_in
            if attempt == 0 and n_in == 700:
                assert out[0].shape[0] <= 1 and sum(o.shape[0] for o in out) < whole.shape[0]      # the look-ahead is held back
                r.reset()
                assert (r.seen, r.position, r.history) == (0, 0, None)
                continue
            out.append(r.flush())
            got = np.concatenate([o.cpu().numpy() for o in out], 0)
            assert got.shape[0] == -(-n_in * r.L // r.M) == R.output_length(n_in, r.L, r.M)
            assert np.array_equal(got, whole), (n_in, c, kind)
            assert (r.seen, r.position, r.history) == (0, 0, None) and r.flush().shape == (0, whole.shape[1])
    with pytest.raises(ValueError):
        r.process(_t(x[:0], dev))
    with pytest.raises(ValueError):
        r.process(_t(np.zeros((3, c + 1), np.float32), dev))


def test_hrir_set_resampled():
    """HrirSet.resampled: 1150 responses through the 64-channel limit in groups, scaled by rate_in / rate_out."""
    import render_oracle as RRO
    from spatialaudiogen_amd.render import HrirSet
    _dev()
    dirs, left, right = RRO.make_hrirs(4, ntaps=24)
    h = HrirSet(dirs, left, right, 44100).resampled(48000, 'fast')
    assert h.rate == 48000 and h.ntaps == -(-24 * 160 // 147) and h.left.shape == (left.shape[0], h.ntaps)
    ref = RO.direct(np.concatenate([left, right], 0).T, 44100, 48000, 'fast')
    got = (np.concatenate([h.left, h.right], 0).T / (44100 / 48000.)).astype(np.float32)
    # (undoing the fp64 scale is exact to well below an fp32 spacing: compared under the one-spacing rule, ties included)
    assert_matches(got, ref, 'HRIRs 44100 -> 48000')
    assert np.abs(h.directions - dirs).max() <= 1e-15


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    dev = _dev()
    l = ensure_lib()
    from spatialaudiogen_amd import resample as R
    L, M, H, taps = R.design(3, 4, SMALL)
    T = taps.shape[1]
    x, tp, mix = _t(_x(20, 4, 1), dev), _t(taps, dev), _t(np.eye(4), dev)
    y = torch.full((30, 4), 777., dtype=torch.float32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    base = dict(x=x, x0=0, n_in=20, c_in=4, taps=tp, L=L, M=M, H=H, T=T, mix=None, c_out=4, n0=0, n=20, y=y)

    def call(**kw):
        a = dict(base, **kw)
        return l.sagen_resample_fir(P(a['x']), a['x0'], a['n_in'], a['c_in'], P(a['taps']), a['L'], a['M'], a['H'], a['T'], P(a['mix']), a['c_out'],
                                    a['n0'], a['n'], P(a['y']), None if dev == 'cpu' else C.c_void_p(torch.cuda.current_stream().cuda_stream))

    OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
    cases = [
        (dict(L=0), SHAPE, 'L, M and T'), (dict(L=-4), SHAPE, 'L, M and T'), (dict(M=0), SHAPE, 'L, M and T'), (dict(T=0), SHAPE, 'L, M and T'),
        (dict(T=T + 1), SHAPE, 'T is not'), (dict(T=T - 1), SHAPE, 'T is not'), (dict(H=H + L), SHAPE, 'T is not'), (dict(H=-1), SHAPE, 'H'),
        (dict(n=-1), SHAPE, ''), (dict(n_in=-1), SHAPE, 'negative'), (dict(x0=-1), SHAPE, 'negative'), (dict(n0=-1), SHAPE, 'negative'),
        (dict(c_in=0), SHAPE, 'c_in'), (dict(c_out=0), SHAPE, 'c_in'), (dict(c_out=2), SHAPE, 'without a mix'),
        (dict(c_in=65, c_out=65), UNSUPPORTED, '64 channels'), (dict(c_out=65, mix=mix), UNSUPPORTED, '64 channels'),
        (dict(L=1, H=2048, T=4097), UNSUPPORTED, '4096'), (dict(L=1 << 20, H=4 << 20, T=9), UNSUPPORTED, '64 MiB'),
        (dict(L=(1 << 20) + 1, H=0, T=1), UNSUPPORTED, '2^20'), (dict(n0=(1 << 40) + 1), UNSUPPORTED, '2^40'),
        (dict(x=None), NULL, 'null'), (dict(taps=None), NULL, 'null'), (dict(y=None), NULL, 'null'),
    ]
    for kw, status, word in cases:
        rc = call(**kw)
        msg = l.sagen_last_error().decode()
        assert rc == status, (kw, rc, msg)
        assert 'sagen_resample_fir' in msg and word in msg, (kw, msg)
        assert bool((y == 777.).all()), kw
    assert call(n=0, L=0, x=None, taps=None, y=None) == OK and bool((y == 777.).all())          # n == 0: nothing is looked at
    assert call(x=None, n_in=0) == OK and bool((y[:20] == 0.).all()) and bool((y[20:] == 777.).all())     # a buffer of no rows: all zeros
    assert call() == OK and not bool((y[:20] == 0.).all()) and bool((y[20:] == 777.).all())


# ---- windowed RMS ----------------------------------------------------------------------------------------------------------------------
def test_window_rms():
    import torch
    from spatialaudiogen_amd import ops
    dev = _dev()
    l = ensure_lib()
    x = _x(10000, 3, 8)
    xd = _t(x, dev)
    # channel, first, hop, length, count: windows at both ends of the buffer included
    for ch, first, hop, length, count in [(0, 0, 7, 100, 5), (1, 9900, 0, 100, 1), (2, 0, 9900, 100, 2), (1, 400, 4800, 4800, 2), (0, 0, 1, 1, 10000),
                                          (2, 3, 65, 63, 9), (0, 9, 64, 64, 150), (1, 0, 1000, 65, 10), (0, 0, 0, 10000, 3)]:
        got = ops.window_rms(xd, ch, first, hop, length, count).cpu().numpy()
        want = np.array([np.sqrt((x[first + i * hop:first + i * hop + length, ch].astype(np.float64) ** 2).mean()) for i in range(count)])
        rel = np.abs(got - want) / want
        print('window_rms ch %d first %d hop %d length %d count %d: max relative difference %.3g' % (ch, first, hop, length, count, rel.max()))
        assert got.dtype == np.float64 and got.shape == (count,)
        assert rel.max() <= 1e-12
    assert ops.window_rms(_t(np.zeros((50, 1), np.float32), dev), 0, 0, 10, 10, 5).cpu().numpy().tolist() == [0.] * 5
    out = torch.full((8,), 777., dtype=torch.float64, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = None if dev == 'cpu' else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = lambda n, c, ch, first, hop, length, count, xx=xd, oo=out: l.sagen_window_rms(P(xx), n, c, ch, first, hop, length, count, P(oo), stream)
    for args, status in [((10000, 3, 0, 9901, 1, 100, 1), -2), ((10000, 3, 0, 0, 4951, 100, 3), -2), ((10000, 3, 0, 0, 1, 10001, 1), -2),
                         ((10000, 3, 3, 0, 1, 10, 1), -2), ((10000, 3, -1, 0, 1, 10, 1), -2), ((10000, 3, 0, -1, 1, 10, 1), -2),
                         ((10000, 3, 0, 0, -1, 10, 2), -2), ((10000, 3, 0, 0, 1, 0, 1), -2), ((10000, 3, 0, 0, 1, 10, -1), -2), ((-1, 3, 0, 0, 1, 10, 1), -2),
                         ((10000, 0, 0, 0, 1, 10, 1), -2), ((10000, 3, 0, (1 << 62), (1 << 62), 10, 8), -2)]:
        assert f(*args) == status, args
        assert 'sagen_window_rms' in l.sagen_last_error().decode()
        assert bool((out == 777.).all()), args
    assert f(10000, 3, 0, 0, 1, 10, 1, xx=None) == -1 and f(10000, 3, 0, 0, 1, 10, 1, oo=None) == -1
    assert f(10000, 3, 9, 0, 1, 0, 0, xx=None, oo=None) == 0 and bool((out == 777.).all())       # count == 0: nothing is looked at
    assert f(10000, 3, 0, 0, 4950, 100, 3) == 0 and bool((out[3:] == 777.).all()) and not bool((out[:3] == 777.).any())


# ---- command lines -----------------------------------------------------------------------------------------------------------------------
def _synthetic(n, c, rate):
    t = np.arange(n)[:, None] / float(rate)
    f = 180. + 97. * np.arange(c)[None, :]
    return 0.3 * np.sin(2 * np.pi * f * t + 0.2 * np.arange(c)[None, :]) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t)) \
        + 0.02 * np.random.RandomState(31).uniform(-1., 1., (n, c))


def test_clip_command_line(tmp_path):
    """3.2 s of 6 channels at 44.1 kHz -> 3 chunks of 48 000 PCM16 samples (the pan remap 2 1 4 0) and 20 lines of audio_pow.lst."""
    from spatialaudiogen_amd import feeder as F, resample as R
    _dev()
    src = str(tmp_path / 'in.wav')
    F.save_wav(src, _synthetic(141120, 6, 44100), 44100)
    x = F.load_wav(src)[0].astype(np.float32)                         # what the file holds: PCM16 / 32768, exact in fp32
    clip = str(tmp_path / 'clip')
    R.main(['clip', src, clip, '--map', '2', '1', '4', '0', '--quality', 'fast', '--block', '50000'])
    assert sorted(os.listdir(clip)) == ['ambix', 'audio_pow.lst'] and sorted(os.listdir(os.path.join(clip, 'ambix'))) == ['%06d.wav' % i for i in range(3)]
    ref = RO.direct(x, 44100, 48000, 'fast', np.eye(6)[[2, 1, 4, 0]]).astype(np.float32)
    assert ref.shape == (153600, 4)
    chunks = []
    for i in range(3):
        got, rate = F.load_wav(os.path.join(clip, 'ambix', '%06d.wav' % i))
        want_fn = str(tmp_path / 'want.wav')
        F.save_wav(want_fn, ref[i * 48000:(i + 1) * 48000], 48000)
        assert rate == 48000 and got.shape == (48000, 4)
        assert np.array_equal(got, F.load_wav(want_fn)[0]), 'chunk %d' % i
        chunks.append(got)
    audio = np.concatenate(chunks, 0)
    lines = open(os.path.join(clip, 'audio_pow.lst')).read().split('\n')
    assert lines[-1] == '' and len(lines) == 21
    for i, line in enumerate(lines[:20]):                             # preprocess.py:149-153 on the reloaded chunks
        t = i / 10. + 0.5
        signal = audio[int(t * 48000):int(t * 48000) + 4800]
        apow = np.sqrt((signal[:, 0] ** 2).mean(axis=0))
        a, b = line.split(' ')
        assert a == '%.12g' % t
        assert abs(float(b) - apow) <= 1e-11 * apow, (i, b, apow)      # twelve digits: half a unit of the last is 5e-12 relative at most
    # the folder reads as a clip folder
    times, powers = F.read_pow_list(os.path.join(clip, 'audio_pow.lst'))
    assert times[:2] == [0.5, 0.6] and len(powers) == 20 and min(powers) > 0
    with pytest.raises(SystemExit):
        R.main(['clip', src, clip, '--map', '2', '1', '4', '0'])                   # holds audio already, no --overwrite
    R.main(['clip', src, clip, '--map', '2', '1', '4', '0', '--quality', 'fast', '--overwrite'])
    assert np.array_equal(F.load_wav(os.path.join(clip, 'ambix', '000002.wav'))[0], chunks[2])      # one block or many: the same bits


def test_convert_command_line(tmp_path):
    from spatialaudiogen_amd import feeder as F, resample as R
    _dev()
    src = str(tmp_path / 'in.wav')
    F.save_wav(src, _synthetic(8820, 4, 44100), 44100)
    x = F.load_wav(src)[0].astype(np.float32)
    out = str(tmp_path / 'out.wav')
    R.main(['convert', src, out, '--rate', '48000', '--float', '--fuma_to_ambix', '--block', '1000'])
    got, rate = F.load_wav(out)
    assert rate == 48000 and got.shape == (9600, 4)
    assert_matches(got.astype(np.float32), RO.direct(x, 44100, 48000, 'best', RO.fuma_to_ambix()), 'convert --float --fuma_to_ambix')
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)             # a float wav holds the fp32 outputs themselves
    with pytest.raises(SystemExit):
        R.main(['convert', src, out, '--rate', '48000'])
    R.main(['convert', src, out, '--rate', '16000', '--quality', 'fast', '--overwrite'])
    pcm, rate = F.load_wav(out)
    ref = RO.direct(x, 44100, 16000, 'fast').astype(np.float32)
    assert rate == 16000 and pcm.shape == ref.shape == (3200, 4)
    assert np.abs(pcm * 32768. - np.rint(np.clip(ref, -1, 1) * 32767.)).max() <= 1.      # PCM16 of an output within one fp32 spacing
    back = F.load_wav(src, 48000, resample='fast')                                     # the opt-in hook of load_wav: fp64 rows at the new rate
    assert back[1] == 48000 and back[0].dtype == np.float64
    assert_matches(back[0].astype(np.float32), RO.direct(x, 44100, 48000, 'fast'), 'load_wav(resample=fast)')


def test_sources_and_render_flags(tmp_path):
    """`sources encode --resample` and `render --resample_hrir` succeed where the unflagged call still exits."""
    import render_oracle as RRO
    from spatialaudiogen_amd import feeder as F, render, sources
    _dev()
    F.save_wav(str(tmp_path / 'm.wav'), _synthetic(4410, 1, 44100), 44100, subtype='FLOAT')
    with open(str(tmp_path / 'pos.txt'), 'w') as f:
        f.write('s0 m.wav 2\n0.3 0.1 1.5\n-0.4 0.2 2.0\n')
    out = str(tmp_path / 'ambix.wav')
    with pytest.raises(SystemExit):
        sources.main(['encode', str(tmp_path / 'pos.txt'), '1', out, '--rate', '24000'])
    assert not os.path.exists(out)
    sources.main(['encode', str(tmp_path / 'pos.txt'), '1', out, '--rate', '24000', '--resample'])
    got, rate = F.load_wav(out)
    assert rate == 24000 and got.shape == (2400, 4) and np.abs(got).max() > 0.5

    dirs, left, right = RRO.make_hrirs(6, ntaps=24)
    RRO.write_cipic_dir(str(tmp_path / 'hrir'), left, right, 44100)
    ambi = str(tmp_path / 'field.wav')
    F.save_wav(ambi, _synthetic(3000, 4, 48000), 48000, subtype='FLOAT')
    stereo = str(tmp_path / 'stereo.wav')
    with pytest.raises(SystemExit, match='44100'):
        render.main([ambi, stereo, '--render', 'hrir', '--hrir_dir', str(tmp_path / 'hrir')])
    assert not os.path.exists(stereo)
    render.main([ambi, stereo, '--render', 'hrir', '--hrir_dir', str(tmp_path / 'hrir'), '--resample_hrir', 'fast'])
    y, rate = F.load_wav(stereo)
    assert rate == 48000 and y.shape == (3000, 2) and np.abs(y).max() > 0
    # the same rendering from the set resampled by hand
    h = render.HrirSet.from_cipic_dir(str(tmp_path / 'hrir')).resampled(48000, 'fast')
    taps, zb = render.build_taps('hrir', 1, 48000, hrir=h)
    r = render.Renderer(taps, zb)
    want = r.process(_t(F.load_wav(ambi)[0].astype(np.float32), r.device)).cpu().numpy()
    assert np.array_equal(y, np.rint(np.clip(want, -1, 1) * 32767.) / 32768.)
