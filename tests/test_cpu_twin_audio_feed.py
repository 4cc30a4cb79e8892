"""sagen_assemble_audio of the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: plain loops over csrc/audio_feed_core.h) against
explicit numpy, as bit patterns, in a container without a GPU.  The cases are tests/audio_feed_cases.py; tests/test_gpu_audio_feed.py
runs the same ones through the device library.  feeder.DeviceAudio's cases of that file (equality with WavPieces.assemble over ambix
folders) run here too, against the twin on device='cpu', in the manner of tests/test_feed_host.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import audio_feed_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


@pytest.fixture(scope='module')
def call(twin):
    from spatialaudiogen_amd import _lib
    l = C.CDLL(twin)
    l.sagen_assemble_audio.restype, l.sagen_assemble_audio.argtypes = _lib.SIGNATURES['sagen_assemble_audio']
    l.sagen_last_error.restype = C.c_char_p

    def run(samples, lead, read_from, count, rot, size, want, t_off, t_len, offset=0):
        n, channels = samples.shape
        buf = np.zeros(n * channels + offset, samples.dtype)
        buf[offset:] = samples.reshape(-1)
        lead, read_from, count = np.ascontiguousarray(lead, np.int32), np.ascontiguousarray(read_from, np.int64), np.ascontiguousarray(count, np.int32)
        rot = None if rot is None else np.ascontiguousarray(rot, np.float64)
        n_out = len(lead)
        shapes = {'full': (n_out, size, channels), 'mono': (n_out, size), 'target': (n_out, t_len, channels - 1)}
        out = {w: np.full(shapes[w], np.nan, np.float32) for w in want}
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = l.sagen_assemble_audio(buf[offset:].ctypes.data if n else None, AC.sample_type(samples.dtype), n, channels, ptr(lead), ptr(read_from),
                                    ptr(count), ptr(rot), n_out, size, t_off, t_len, ptr(out.get('full')), ptr(out.get('mono')),
                                    ptr(out.get('target')), None)
        assert rc == 0, l.sagen_last_error()
        return out
    return run


@pytest.mark.parametrize('dtype', AC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('channels', AC.CHANNELS)
@pytest.mark.parametrize('size', AC.SIZES)
def test_every_window_kind_equals_numpy_bit_for_bit(call, size, channels, dtype):
    AC.check_shape(call, size, channels, dtype)


def test_more_items_than_the_grid_takes(call):
    AC.check_grid_strides(call)


def test_a_base_aligned_to_its_element_only(call):
    AC.check_offset_base(call)


def test_no_samples_is_all_padding(call):
    AC.check_no_samples(call)


def test_an_empty_batch_touches_nothing(call):
    s = AC.samples_of(10, 4, np.float32)
    got = call(s, [], [], [], None, 7, ('full', 'mono', 'target'), 0, 7)
    assert all(g.shape[0] == 0 for g in got.values())


def test_the_numpy_oracle_meets_the_cap_against_the_host_rotation(tmp_path):
    """The host feeder rotates with `.dot`, whose BLAS may fuse or reorder: one float64 rounding apart from the fixed order, which
    shows in few float32 values if in any.  The fixed order itself (AC.oracle_rotated, what the op must equal bit for bit) stays
    within 1 ulp of the host at every element and differs in at most 1e-4 of them, for the folder and the angles the device cases use."""
    folder = AC.make_ambix(str(tmp_path / 'ambix'))
    plain, live = AC.plain_windows(folder)
    assert live[AC.TIMES.index(0.0), :100].sum() == 0 and live[1].all() and 0 < live[-1].sum() < AC.SIZE           # a lead, a whole window, a trail
    AC.within_one_ulp(AC.oracle_rotated(plain, live, AC.ROTATIONS), AC.host_windows(folder, AC.ROTATIONS))


def test_device_audio_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_audio_feed import HOST_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_audio_feed.py'), '-m', 'gpu', '-q', '-x', '-k', HOST_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert '5 passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the op cases run above; deploy and evaluate need the device and stay out
