"""The switch table (csrc/switches.h), without a GPU: it is the only place that reads the environment, INTEGRATION.md 5 lists what it
lists, every row reads its variable the way the sites it replaced did (tests/golden/switches_v1.txt, transcribed from those sites), the
settings a context derives from the rows reach the workspace carving (tests/golden/switch_workspace_v1.txt, recorded from the build
before the table existed) and sagen_set_option answers every name as before."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'spatialaudiogen_amd', 'csrc')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
# options sagen_set_option handles with a rule of their own (model.hip) next to the ones the rows name: (name, a value it accepts)
OWN_RULE_OPTIONS = [('materialize_mask', 1), ('intermediate_group', 0), ('planes_from_stage', 3), ('decoder_planes', 1), ('plane_gather', 1)]


@pytest.fixture(scope='module')
def listing(tmp_path_factory):
    """Output of tests/switches_listing.cpp, built with the host compiler from switches.h alone: one line per row."""
    exe = str(tmp_path_factory.mktemp('switches') / 'switches_listing')
    subprocess.run([os.environ.get('CXX', 'g++'), '-std=c++17', '-Wall', '-Werror', '-I', CSRC, os.path.join(ROOT, 'tests', 'switches_listing.cpp'), '-o', exe],
                   check=True, capture_output=True, text=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout


def rows(listing):
    """[(environment name, option name or None)] in table order."""
    return [(f[0], None if f[1] == '-' else f[1]) for f in (l.split(' ') for l in listing.splitlines())]


def test_only_the_table_reads_the_environment():
    for f in sorted(os.listdir(CSRC)):
        if os.path.isfile(os.path.join(CSRC, f)) and not f.startswith('switches.'):
            assert 'getenv' not in open(os.path.join(CSRC, f)).read(), f


def test_row_semantics_are_those_of_the_sites_they_replace(listing):
    assert listing == open(os.path.join(GOLDEN, 'switches_v1.txt')).read()
    names = [e for e, _ in rows(listing)]
    assert len(names) == 56 and len(set(names)) == 56


def test_integration_md_lists_the_table(listing):
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    sec = text[text.index('\n## 5. '):]
    native = sec[:sec.index('### Python host')]
    envs = {e for e, _ in rows(listing)}
    opts = {o for _, o in rows(listing) if o} | {o for o, _ in OWN_RULE_OPTIONS}
    assert len(opts) == 12
    for e in envs:
        assert re.search(r'`%s\b' % e, native), '%s is not in INTEGRATION.md 5' % e
    for o in opts:
        assert '`"%s"`' % o in native, 'option %s is not in INTEGRATION.md 5' % o
    assert set(re.findall(r'SAGEN_[A-Z0-9_]+', native)) == envs


# one child process: per variable set it, create a context (batch 2, audio + video, 32 tracks), print both workspace sizes, destroy, unset
CHILD = r'''
import ctypes as C, os, sys
sys.path.insert(0, %r)
from spatialaudiogen_amd import _lib
L = _lib.lib()
def sizes(name):
    cfg = _lib.SagenConfig()
    cfg.batch, cfg.encoders, cfg.separation, cfg.num_sep_tracks, cfg.n_loc_units = 2, 3, 1, 32, 2
    cfg.loc_units[0], cfg.loc_units[1] = 512, 512
    cfg.ambi_order, cfg.audio_rate, cfg.video_rate = 1, 48000, 10
    cfg.context, cfg.sample_duration, cfg.fft_window = 1.0, 0.1, 0.025
    h = C.c_void_p()
    rc = L.sagen_create(C.byref(h), C.byref(cfg))
    assert rc == 0, (name, rc, L.sagen_last_error())
    print(name, int(L.sagen_workspace_bytes(h)), int(L.sagen_train_workspace_bytes(h)))
    L.sagen_destroy(h)
names = sys.argv[1:]
for n in names:
    os.environ.pop(n, None)
sizes('base')
for n in names:
    os.environ[n] = '3' if n == 'SAGEN_P3_FROM_STAGE' else '1'
    sizes(n)
    del os.environ[n]
sizes('base_again')
'''


def test_derived_settings_reach_the_carving(listing):
    from spatialaudiogen_amd import build
    build.build(verbose=False)
    names = [e for e, _ in rows(listing)]
    r = subprocess.run([sys.executable, '-c', CHILD % ROOT] + names, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    golden = [l for l in open(os.path.join(GOLDEN, 'switch_workspace_v1.txt')).read().split('\n') if l and not l.startswith('#')]
    assert got == golden
    base = got[0].split(' ')[1:]
    assert got[-1].split(' ')[1:] == base
    moved = sorted(l.split(' ')[0] for l in got[1:-1] if l.split(' ')[1:] != base)
    assert moved == ['SAGEN_FCM', 'SAGEN_FP32_ONLY', 'SAGEN_NO_H2', 'SAGEN_NO_P3', 'SAGEN_P3_FROM_STAGE', 'SAGEN_TRAIN_NO_H2', 'SAGEN_TRAIN_NO_H2D',
                     'SAGEN_TRAIN_NO_H2W']


def _create(lib, **kw):
    from test_abi import _cfg
    h, cfg = C.c_void_p(), _cfg(**kw)
    assert lib.sagen_create(C.byref(h), C.byref(cfg)) == 0, lib.sagen_last_error()
    return h


def test_every_option_name_answers_as_before(listing):
    from spatialaudiogen_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.lib()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    h = _create(lib, batch=2)
    options = [(o, 1) for _, o in rows(listing) if o] + OWN_RULE_OPTIONS
    assert len(options) == 12
    for name, value in options:
        assert lib.sagen_set_option(h, name.encode(), value) == 0, (name, lib.sagen_last_error())
        assert lib.sagen_set_option(h, name.encode(), 0 if name != 'planes_from_stage' else 2) == 0, (name, lib.sagen_last_error())
    SHAPE, UNSUPPORTED = -2, -3
    assert lib.sagen_set_option(h, b'planes_from_stage', 1) == SHAPE
    assert lib.sagen_set_option(h, b'planes_from_stage', 7) == SHAPE
    assert lib.sagen_last_error() == b'planes_from_stage in 2..6'
    assert lib.sagen_set_option(h, b'intermediate_group', 1) == SHAPE            # a one-group context
    assert lib.sagen_last_error() == b'intermediate_group=1 of 1 groups'
    assert lib.sagen_set_option(h, b'no_such_option', 1) == UNSUPPORTED
    assert lib.sagen_last_error() == b'sagen_set_option: unknown option no_such_option'
    lib.sagen_destroy(h)
