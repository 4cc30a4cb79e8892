"""feeder.DeviceFrames without a GPU: its cases of tests/test_gpu_feed.py - equality with JpgFrames.frames / FlowFrames.frames over a
make_clip(flow=True, secs=1) folder with and without a rotation, ensure() decoding only what is missing, an index outside the resident
range and a flow_prep refused before any launch, a float32 limits file - run against the CPU twin (libsagen_cpu.so decodes the files
and assembles the batches on device='cpu'), in the manner of tests/test_cpu_twin_jpeg.py; and the host logic of `deploy --decode`."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    return build.build_cpu_twin()


def test_device_frames_cases_pass_on_the_cpu_twin(twin):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_feed import HOST_CASES
    env = dict(os.environ, SAGEN_LIB=twin)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_feed.py'), '-m', 'gpu', '-q', '-x', '-k', HOST_CASES,
                        '-p', 'no:cacheprovider'], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert '10 passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]
    assert 'deselected' in r.stdout                     # the deploy-size call and the command lines need the device and stay out


def test_deploy_decode_flag_names_both_decoders():
    """--decode host | device says where the frames are decoded; projection | pseudoinv stay the ambisonic decoder of --render."""
    from spatialaudiogen_amd import deploy
    a = deploy.parse_arguments(['m', 'clip'])
    assert (a.frame_decode, a.decode) == ('host', None)
    a = deploy.parse_arguments(['m', 'clip', '--decode', 'device'])
    assert (a.frame_decode, a.decode) == ('device', None)
    a = deploy.parse_arguments(['m', 'clip', '--decode', 'device', '--render', 'ears', '--render_fn', 'r.wav', '--decode', 'projection'])
    assert (a.frame_decode, a.decode, a.render) == ('device', 'projection', 'ears')
    a = deploy.parse_arguments(['m', 'clip', '--render', 'speakers', '--render_fn', 'r.wav', '--decode', 'pseudoinv'])
    assert (a.frame_decode, a.decode) == ('host', 'pseudoinv')
    with pytest.raises(SystemExit):
        deploy.parse_arguments(['m', 'clip', '--decode', 'gpu'])
    with pytest.raises(ValueError, match='decode'):
        deploy.W2XYZ(params=object(), variables={}, decode='gpu')
