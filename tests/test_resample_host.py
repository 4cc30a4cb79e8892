"""The resampler's definition held to account on the host: the two independent paths of tests/resample_oracle.py (the direct sums and
scipy.signal.resample_poly on the same taps) agree, resample.design() is the table the restatement builds tap by tap, the filter is the
filter it claims to be (sinusoid known answers, DC gain), the channel mixes and the audio_pow.lst formatting, and every opt-in hook
left at its default refuses exactly as before.  Nothing here needs a device.

The sinusoid bounds carry a margin of 2 to 5 over what the restatement measured on the CPU when they were set ('best': passband 4.6e-8
worst, stopband 9.3e-8; 'fast': passband 5.2e-5, stopband 6.1e-5): room for another libm, not for another filter."""
import os

import numpy as np
import pytest

import resample_oracle as RO

RATIOS = [(7, 5), (3, 4), (44100, 48000), (48000, 16000), (24000, 48000)]
QUALITIES = ['best', 'fast']


def _x(n, c, seed):
    return np.random.RandomState(seed).uniform(-1., 1., (n, c)).astype(np.float32)


@pytest.mark.parametrize('quality', QUALITIES)
@pytest.mark.parametrize('rates', RATIOS)
def test_the_two_oracle_paths_agree(rates, quality):
    x = _x(700, 2, 11)
    a, b = RO.direct(x, rates[0], rates[1], quality), RO.poly(x, rates[0], rates[1], quality)
    L, M, _, _ = RO.filt(rates[0], rates[1], quality)
    assert a.shape == b.shape == (-(-700 * L // M), 2)
    d = np.abs(a - b).max()
    print('%d -> %d %s: max |direct - resample_poly| %.3g' % (rates[0], rates[1], quality, d))
    assert d <= 1e-13


@pytest.mark.parametrize('rates,quality,n_in', [((7, 5), 'fast', 33), ((3, 4), (4, 5.0, 0.8), 33), ((44100, 48000), 'fast', 120), ((1, 3), 'best', 7), ((3, 1), 'fast', 50)])
def test_the_whole_array_form_is_the_literal_double_loop_bit_for_bit(rates, quality, n_in):
    x = _x(n_in, 3, 5)
    mix = np.random.RandomState(6).uniform(-1., 1., (2, 3))
    for m in (None, mix):
        a, b = RO.direct_loop(x, rates[0], rates[1], quality, m), RO.direct(x, rates[0], rates[1], quality, m)
        assert a.shape == b.shape and np.array_equal(a, b)
    # a window of outputs seen through a window of rows = the whole-stream sums over the rows seen
    y = RO.direct(np.where((np.arange(n_in) >= 4)[:, None] & (np.arange(n_in) < 20)[:, None], x, 0), rates[0], rates[1], quality)
    assert np.array_equal(RO.direct(x, rates[0], rates[1], quality, n0=2, n=9, x0=4, rows=16), y[2:11])


@pytest.mark.parametrize('quality', QUALITIES + [(4, 5.0, 0.8)])
@pytest.mark.parametrize('rates', RATIOS + [(160, 147), (1, 3)])
def test_design_is_the_restated_table_exactly(rates, quality):
    from spatialaudiogen_amd import resample as R
    L, M, H, taps = R.design(rates[0], rates[1], quality)
    rl, rm, rh, rt = RO.table(rates[0], rates[1], quality)
    assert (L, M, H) == (rl, rm, rh)
    assert taps.dtype == np.float64 and taps.shape == rt.shape == (L, -(-(2 * H + 1) // L))
    assert np.array_equal(taps, rt)
    assert R.output_length(700, L, M) == RO.n_out(700, L, M)


def test_design_refuses_what_is_not_a_ratio_or_a_quality():
    from spatialaudiogen_amd import resample as R
    for bad in [(0, 48000), (44100, -1), (44100.5, 48000)]:
        with pytest.raises(ValueError):
            R.design(bad[0], bad[1])
    for q in ['better', (0, 5., .8), (4, 5.), (4, 5., 1.5)]:
        with pytest.raises(ValueError):
            R.design(3, 4, q)
    assert R.quality_tuple('fast') == (16, 8.6, 0.85) and R.quality_tuple('best') == (64, 14.8, 0.9476)


# ---- the filter is the filter it claims to be -----------------------------------------------------------------------------------------
KAT_RATIOS = [(44100, 48000), (48000, 44100), (48000, 16000), (16000, 48000)]
PASS = {'best': ((0.05, 0.5, 0.8), 2e-7), 'fast': ((0.05, 0.5), 1e-4)}
STOP = {'best': 5e-7, 'fast': 2e-4}


def _tone(rates, quality, rel):
    """(resampled tone, analytic tone at the new rate), both cut to the outputs further than 2 Z max(1, L / M) + 2 from either end."""
    n_in, phase = 6000, 0.3
    f = rel * min(rates) / 2.
    x = np.sin(2 * np.pi * f * np.arange(n_in) / rates[0] + phase)[:, None]
    y = RO.direct(x, rates[0], rates[1], quality)[:, 0]
    L, M, _, _ = RO.filt(rates[0], rates[1], quality)
    edge = int(np.ceil(2 * RO.PRESETS[quality][0] * max(1., L / float(M)) + 2))
    want = np.sin(2 * np.pi * f * np.arange(y.shape[0]) / rates[1] + phase)
    assert y.shape[0] > 2 * edge + 100
    return y[edge + 1:-edge - 1], want[edge + 1:-edge - 1]


@pytest.mark.parametrize('quality', QUALITIES)
@pytest.mark.parametrize('rates', KAT_RATIOS)
def test_passband_tones_come_out_as_the_same_tone_at_the_new_rate(rates, quality):
    tones, bound = PASS[quality]
    for rel in tones:
        y, want = _tone(rates, quality, rel)
        d = np.abs(y - want).max()
        print('%d -> %d %s tone at %.2f nyq: max |y - sin| %.3g (bound %.0e)' % (rates[0], rates[1], quality, rel, d, bound))
        assert d <= bound


@pytest.mark.parametrize('quality', QUALITIES)
@pytest.mark.parametrize('rates', [r for r in KAT_RATIOS if r[1] < r[0]])
def test_stopband_tones_are_removed_when_downsampling(rates, quality):
    for rel in (1.06, 1.15):
        y, _ = _tone(rates, quality, rel)
        d = np.abs(y).max()
        print('%d -> %d %s tone at %.2f nyq: max |y| %.3g (bound %.0e)' % (rates[0], rates[1], quality, rel, d, STOP[quality]))
        assert d <= STOP[quality]


@pytest.mark.parametrize('quality,bound', [('fast', 2e-5), ('best', 1e-8)])
@pytest.mark.parametrize('rates', RATIOS + [(48000, 44100), (16000, 48000)])
def test_dc_gain(rates, quality, bound):
    L, _, _, h = RO.filt(rates[0], rates[1], quality)
    g = h.sum() / L
    print('%d -> %d %s: DC gain - 1 = %.3g' % (rates[0], rates[1], quality, g - 1.))
    assert abs(g - 1.) <= bound


# ---- mixes, formatting ---------------------------------------------------------------------------------------------------------------
def test_mix_from_map_is_the_selection_of_the_pan_remap():
    from spatialaudiogen_amd import resample as R
    m = R.mix_from_map([2, 1, 4, 0], 6)
    assert m.shape == (4, 6) and m.dtype == np.float64 and m.sum() == 4
    x = np.arange(12.).reshape(2, 6)
    assert np.array_equal(x @ m.T, x[:, [2, 1, 4, 0]])
    assert np.array_equal(R.mix_from_map([0, 1, 2, 3], 4), np.eye(4))
    for bad in ([0, 6], [-1], [0.5]):
        with pytest.raises(ValueError):
            R.mix_from_map(bad, 6)


def test_fuma_matrices():
    from spatialaudiogen_amd import resample as R
    a = R.mix_fuma_to_ambix(1)
    assert np.array_equal(a, RO.fuma_to_ambix())
    w, x, y, z = 0.3, -0.5, 0.7, 0.11                       # a B-format sample (W X Y Z): ambiX is (sqrt 2 W, Y, Z, X)
    assert np.allclose(a @ np.array([w, x, y, z]), [np.sqrt(2.) * w, y, z, x], rtol=0, atol=1e-16)
    assert np.allclose(R.mix_ambix_to_fuma(1) @ a, np.eye(4), rtol=0, atol=1e-15)
    assert np.allclose(a @ R.mix_ambix_to_fuma(1), np.eye(4), rtol=0, atol=1e-15)
    for f in (R.mix_fuma_to_ambix, R.mix_ambix_to_fuma):
        with pytest.raises(ValueError):
            f(2)


def test_pow_list_lines_and_windows():
    from spatialaudiogen_amd import resample as R
    assert R.format_pow_line(0.5, 0.0123456789012345) == '0.5 0.0123456789012\n'
    assert R.format_pow_line(1.0, 1e-05) == '1 1e-05\n'
    assert R.format_pow_line(0.1 + 0.5, 0.25) == '0.6 0.25\n'                 # 0.6 exactly as Python 2 printed 0.1 + 0.5
    assert R.format_pow_line(2.3000000000000003, 1. / 3.) == '2.3 0.333333333333\n'
    times, starts = R.pow_windows(3)
    assert len(times) == 20 and times[0] == 0.5 and times[-1] == 19 / 10. + 0.5
    assert starts == [int((i / 10. + 0.5) * 48000) for i in range(20)] and starts[0] == 24000
    assert starts[-1] + 4800 <= 3 * 48000
    assert R.pow_windows(1) == ([], []) and R.pow_windows(0) == ([], [])
    y = np.array([[0.5, 2.], [-1.5, 0.], [1e-5, 0.]])
    assert np.array_equal(R.pcm16_as_stored(y), np.array([[16384., 32767.], [-32767., 0.], [0., 0.]]) / 32768.)


def test_equal_rates_without_a_mix_return_the_input_itself():
    from spatialaudiogen_amd import resample as R
    x = _x(5, 2, 1)
    assert R.resample(x, 48000, 48000) is x


# ---- the hooks, left at their defaults, refuse as before -------------------------------------------------------------------------------
def _wav(path, rate, n=64, c=1):
    from spatialaudiogen_amd.feeder import save_wav
    save_wav(path, 0.25 * np.sin(np.arange(n * c).reshape(n, c) / 7.), rate)
    return path


def test_load_wav_still_refuses_a_rate_mismatch_by_default(tmp_path):
    from spatialaudiogen_amd.feeder import load_wav
    fn = _wav(str(tmp_path / 'a.wav'), 48000, c=2)
    with pytest.raises(ValueError, match='no resampler available offline'):
        load_wav(fn, 44100)
    with pytest.raises(ValueError, match='48000 Hz, expected 44100'):
        load_wav(fn, 44100, resample=None)
    data, rate = load_wav(fn, 48000, resample='best')          # nothing to resample: no device is asked for
    assert rate == 48000 and data.shape == (64, 2) and data.dtype == np.float64
    assert load_wav(fn)[1] == 48000


def _hrirs(rate):
    from spatialaudiogen_amd.render import HrirSet
    rs = np.random.RandomState(2)
    d = rs.normal(size=(6, 3))
    return HrirSet(d, rs.normal(size=(6, 16)), rs.normal(size=(6, 16)), rate)


def test_build_taps_still_refuses_hrirs_at_another_rate_by_default():
    from spatialaudiogen_amd import render
    with pytest.raises(ValueError, match='44100'):
        render.build_taps('hrir', 1, 48000, hrir=_hrirs(44100))
    with pytest.raises(ValueError, match='no resampler available offline'):
        render.build_taps('hrir', 1, 48000, hrir=_hrirs(44100), resample=None)
    taps, zb = render.build_taps('hrir', 1, 48000, hrir=_hrirs(48000), resample='best')       # same rate: nothing to resample
    assert taps.shape == (2, 4, 16) and zb == 15
    h = _hrirs(48000)
    assert h.resampled(48000) is h


def test_the_flags_are_off_by_default_and_bare_means_best():
    from spatialaudiogen_amd import render, sources
    assert render.parse_arguments(['a.wav', 'b.wav']).resample_hrir is None
    assert render.parse_arguments(['a.wav', 'b.wav', '--resample_hrir']).resample_hrir == 'best'
    assert render.parse_arguments(['a.wav', 'b.wav', '--resample_hrir', 'fast']).resample_hrir == 'fast'
    assert sources.parse_arguments(['encode', 'p.txt', '1', 'o.wav']).resample is None
    assert sources.parse_arguments(['encode', 'p.txt', '1', 'o.wav', '--resample']).resample == 'best'
    assert sources.parse_arguments(['binauralize', 'i.wav', 'p.txt', 'o.wav', '--resample', 'fast']).resample == 'fast'
    assert sources.parse_arguments(['encode_and_binauralize', 'i.wav', 'p.txt', '1', 'o.wav']).resample is None
    with pytest.raises(SystemExit):
        render.parse_arguments(['a.wav', 'b.wav', '--resample_hrir', 'better'])


def test_sources_encode_still_exits_on_a_rate_mismatch_without_the_flag(tmp_path):
    from spatialaudiogen_amd import sources
    _wav(str(tmp_path / 'm.wav'), 44100)
    pos = tmp_path / 'pos.txt'
    pos.write_text('s0 m.wav 1\n0.0 0.0 1.0\n')
    args = sources.parse_arguments(['encode', str(pos), '1', str(tmp_path / 'out.wav'), '--rate', '24000'])
    with pytest.raises(SystemExit, match='no resampler available offline'):
        sources.run_encode(args)
    assert not os.path.exists(str(tmp_path / 'out.wav'))


def test_clip_and_convert_refuse_before_any_work(tmp_path):
    from spatialaudiogen_amd import resample as R
    fn = _wav(str(tmp_path / 'a.wav'), 44100, c=4)
    with pytest.raises(SystemExit, match='48000 Hz'):
        R.main(['clip', fn, str(tmp_path / 'clip'), '--rate', '44100'])
    with pytest.raises(SystemExit, match='exists'):
        R.main(['convert', fn, fn, '--rate', '48000'])
    with pytest.raises(SystemExit, match='--block'):
        R.main(['convert', fn, str(tmp_path / 'b.wav'), '--block', '0'])
    with pytest.raises(SystemExit, match='input channels'):
        R.main(['convert', fn, str(tmp_path / 'b.wav'), '--map', '0', '7'])
    with pytest.raises(SystemExit, match='fuma_to_ambix'):
        R.main(['convert', fn, str(tmp_path / 'b.wav'), '--map', '0', '1', '--fuma_to_ambix'])
