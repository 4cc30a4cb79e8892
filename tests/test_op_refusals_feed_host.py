"""What sagen_assemble_frames refuses, with which code and which message - pinned for BOTH libraries by one fixture, in the manner of
tests/test_op_refusals_host.py (whose buffer, offsets and binding this file borrows).

The entry point is written once (csrc/op_entries_feed.h, a header of its own next to csrc/op_entries.h because that test pins
op_entries.h against lines recorded earlier) and compiled into libsagen_hip.so and into the CPU twin.  Every call of the table below
returns before any launch; tests/golden/op_refusals_feed_v1.txt holds what libsagen_hip.so answered.  A 4-byte alignment rule is
broken by the offsets 1 and 2, the 8-byte rule by 4.  No GPU is needed: nothing here reaches a kernel.

    python tests/test_op_refusals_feed_host.py        prints the lines of the device library of the tree the file lies in
"""
import ctypes as C
import os
import re
import sys

import pytest

from test_op_refusals_host import P, OFF4, OFF2, OFF1, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'op_refusals_feed_v1.txt')
NAMES = ('frames', 'n_frames', 'h', 'w', 'index', 'shift', 'n_out', 'mode', 'table', 'scale_lo', 'out', 'stream')
VALID = dict(frames=P, n_frames=3, h=4, w=8, index=P, shift=P, n_out=2, mode=2, table=P, scale_lo=P, out=P, stream=None)   # would launch: never made
POINTERS = ('frames', 'index', 'shift', 'table', 'scale_lo', 'out')
ROWS = [
    ('n_out_-1', dict(n_out=-1)), ('n_frames_-1', dict(n_frames=-1)),
    ('empty_no_items', dict({k: None for k in POINTERS}, n_out=0, h=0, w=0, mode=9)),
    ('h_0', dict(h=0)), ('w_0', dict(w=0)), ('h_16385', dict(h=16385)), ('w_16385', dict(w=16385)),
    ('mode_-1', dict(mode=-1)), ('mode_3', dict(mode=3)),
    ('null_frames', dict(frames=None)), ('null_index', dict(index=None)), ('null_shift', dict(shift=None)), ('null_out', dict(out=None)),
    ('null_out_no_frames', dict(frames=None, n_frames=0, out=None)),
    ('null_table_mode_1', dict(mode=1, table=None)), ('null_table_mode_2', dict(table=None)), ('null_scale_lo', dict(scale_lo=None)),
    ('out_off_1', dict(out=OFF1)), ('out_off_2', dict(out=OFF2)), ('out_off_2_mode_1', dict(mode=1, out=OFF2)),
    ('table_off_1', dict(table=OFF1)), ('table_off_2', dict(table=OFF2)),
    ('scale_lo_off_4', dict(scale_lo=OFF4)),
    ('index_off_1', dict(index=OFF1)), ('index_off_2', dict(index=OFF2)), ('shift_off_1', dict(shift=OFF1)), ('shift_off_2', dict(shift=OFF2)),
    ('index_off_2_mode_0', dict(mode=0, index=OFF2, table=None, scale_lo=None)),
]


def refusal_lines(lib):
    """'sagen_assemble_frames <case> <rc> <message>' per row: what the golden file holds."""
    lines = []
    for case, over in ROWS:
        args = dict(VALID, **over)
        rc = lib.sagen_assemble_frames(*[args[k] for k in NAMES])
        assert (rc == 0) == case.startswith('empty'), (case, rc, lib.sagen_last_error())
        lines.append(('sagen_assemble_frames %s %d %s' % (case, rc, lib.sagen_last_error().decode() if rc else '')).rstrip())
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
    """Each fail(...) statement of csrc/op_entries_feed.h is the message of at least one line of the fixture."""
    text = open(os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc', 'op_entries_feed.h')).read()
    formats = re.findall(r'\bfail\([A-Za-z_]+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text)
    assert len(formats) == 10
    messages = [l.split(' ', 3)[3] for l in golden() if len(l.split(' ', 3)) == 4]
    for f in formats:
        fmt = ''.join(re.findall(r'"((?:[^"\\]|\\.)*)"', f))
        pattern = '.*'.join(re.escape(part) for part in re.split(r'%(?:ld|zu|d|g|s)', fmt))
        assert any(re.fullmatch(pattern, m) for m in messages), 'no row of the table reaches: ' + fmt


def test_the_codes_are_the_documented_ones():
    code = {l.split(' ')[1]: int(l.split(' ')[2]) for l in golden()}
    assert code['empty_no_items'] == 0
    assert {code[k] for k in ('h_16385', 'w_16385')} == {-3}
    assert {code[k] for k in code if k.startswith('null_')} == {-1}
    assert {code[k] for k in code if not k.startswith(('null_', 'empty')) and k not in ('h_16385', 'w_16385')} == {-2}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from spatialaudiogen_amd import _lib
    print('\n'.join(refusal_lines(_lib.lib())))
