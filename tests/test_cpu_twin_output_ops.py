"""The sweep of tests/test_gpu_output_ops.py against the CPU twin (libsagen_cpu.so, csrc_cpu/sagen_cpu.cpp: sagen_render_fir,
sagen_encode_sources and sagen_binauralize_sources as plain loops) - in a container without a GPU, on the pattern of
tests/test_cpu_twin_render.py.  Every case of the file is op-level, so all of them run.  The twin sums in double: it is held to the
elementwise bounds, the integer known answers, the NaN guards and the RMS bar of the sweep, not to the kernels' bits."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_output_op_level_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import output_oracle as OO
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_output_ops.py'), '-m', 'gpu', '-q', '-x', '-s',
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert '%d passed' % (len(OO.render_cases()) + len(OO.source_cases())) in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'twin: not held' in r.stdout and 'skipped' not in r.stdout          # the run did take the twin's branch, and every case ran
