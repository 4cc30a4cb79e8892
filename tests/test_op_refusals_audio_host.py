"""What sagen_assemble_audio refuses, with which code and which message - pinned for BOTH libraries by one fixture, in the manner of
tests/test_op_refusals_feed_host.py (whose buffer, offsets and binding come from tests/test_op_refusals_host.py).

The entry point is written once (csrc/op_entries_audio.h) and compiled into libsagen_hip.so and into the CPU twin.  Every call of the
table below returns before any launch; tests/golden/op_refusals_audio_v1.txt holds what libsagen_hip.so answered.  A 2-byte alignment
rule is broken by the offset 1, a 4-byte rule by 1 and 2, an 8-byte rule by 4.  No GPU is needed: nothing here reaches a kernel.

    python tests/test_op_refusals_audio_host.py        prints the lines of the device library of the tree the file lies in
"""
import ctypes as C
import os
import re
import sys

import pytest

from test_op_refusals_host import P, OFF4, OFF2, OFF1, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'op_refusals_audio_v1.txt')
NAMES = ('samples', 'sample_type', 'n_samples', 'channels', 'lead', 'read_from', 'count', 'rot', 'n_out', 'size', 't_off', 't_len', 'full',
         'mono', 'target', 'stream')
VALID = dict(samples=P, sample_type=2, n_samples=100, channels=4, lead=P, read_from=P, count=P, rot=P, n_out=2, size=37, t_off=5, t_len=8,
             full=P, mono=P, target=P, stream=None)                                     # would launch: never made
POINTERS = ('samples', 'lead', 'read_from', 'count', 'rot', 'full', 'mono', 'target')
UNSUPPORTED = ('channels_17', 'size_16777217', 'rot_channels_3', 'rot_channels_5')
ROWS = [
    ('n_out_-1', dict(n_out=-1)), ('n_samples_-1', dict(n_samples=-1)),
    ('empty_no_items', dict({k: None for k in POINTERS}, n_out=0, size=0, channels=0, sample_type=9, t_len=0)),
    ('size_0', dict(size=0)), ('channels_0', dict(channels=0, rot=None)),
    ('sample_type_-1', dict(sample_type=-1)), ('sample_type_3', dict(sample_type=3)),
    ('channels_17', dict(channels=17, rot=None)), ('size_16777217', dict(size=(1 << 24) + 1)),
    ('null_samples', dict(samples=None)), ('null_lead', dict(lead=None)), ('null_read_from', dict(read_from=None)), ('null_count', dict(count=None)),
    ('null_outputs', dict(full=None, mono=None, target=None)), ('null_outputs_no_samples', dict(samples=None, n_samples=0, full=None, mono=None, target=None)),
    ('rot_channels_3', dict(channels=3)), ('rot_channels_5', dict(channels=5)),
    ('target_channels_1', dict(channels=1, rot=None)),
    ('t_off_-1', dict(t_off=-1)), ('t_len_0', dict(t_len=0)), ('t_len_past_the_end', dict(t_off=30, t_len=8)), ('t_len_int_max', dict(t_off=1, t_len=2 ** 31 - 1)),
    ('samples_off_1_int16', dict(sample_type=0, samples=OFF1)), ('samples_off_2_float32', dict(sample_type=1, samples=OFF2)),
    ('samples_off_4_float64', dict(samples=OFF4)),
    ('lead_off_2', dict(lead=OFF2)), ('count_off_1', dict(count=OFF1)), ('read_from_off_4', dict(read_from=OFF4)),
    ('rot_off_4', dict(rot=OFF4)),
    ('full_off_2', dict(full=OFF2)), ('mono_off_1', dict(mono=OFF1)), ('target_off_2', dict(target=OFF2)),
    ('mono_off_2_alone', dict(full=None, target=None, mono=OFF2, rot=None, t_len=0)),
]


def refusal_lines(lib):
    """'sagen_assemble_audio <case> <rc> <message>' per row: what the golden file holds."""
    lines = []
    for case, over in ROWS:
        args = dict(VALID, **over)
        rc = lib.sagen_assemble_audio(*[args[k] for k in NAMES])
        assert (rc == 0) == case.startswith('empty'), (case, rc, lib.sagen_last_error())
        lines.append(('sagen_assemble_audio %s %d %s' % (case, rc, lib.sagen_last_error().decode() if rc else '')).rstrip())
    return lines


@pytest.fixture(scope='module')
def device_lib():
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope='module')
def twin_lib():
    from spatialaudiogen_amd import build
    return _bind(C.CDLL(build.build_cpu_twin()))


def golden():
    text = open(GOLDEN).read().split('\n')
    assert text[0].startswith('# ')
    return [l for l in text[1:] if l]


def test_the_twin_refuses_as_the_device_library_did(twin_lib):
    assert refusal_lines(twin_lib) == golden()


def test_the_device_library_refuses_as_recorded(device_lib):
    assert refusal_lines(device_lib) == golden()


def test_every_refusal_of_the_entry_point_is_reached():
    """Each fail(...) statement of csrc/op_entries_audio.h is the message of at least one line of the fixture."""
    text = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'op_entries_audio.h')).read()
    formats = re.findall(r'\bfail\([A-Za-z_]+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text)
    assert len(formats) == 14
    messages = [l.split(' ', 3)[3] for l in golden() if len(l.split(' ', 3)) == 4]
    for f in formats:
        fmt = ''.join(re.findall(r'"((?:[^"\\]|\\.)*)"', f))
        pattern = '.*'.join(re.escape(part) for part in re.split(r'%(?:ld|zu|d|g|s)', fmt))
        assert any(re.fullmatch(pattern, m) for m in messages), 'no row of the table reaches: ' + fmt


def test_the_codes_are_the_documented_ones():
    code = {l.split(' ')[1]: int(l.split(' ')[2]) for l in golden()}
    assert len(code) == len(ROWS)
    assert code['empty_no_items'] == 0
    assert {code[k] for k in UNSUPPORTED} == {-3}
    assert {code[k] for k in code if k.startswith('null_')} == {-1}
    assert {code[k] for k in code if not k.startswith(('null_', 'empty')) and k not in UNSUPPORTED} == {-2}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from spatialaudiogen_amd import _lib
    print('\n'.join(refusal_lines(_lib.lib())))
