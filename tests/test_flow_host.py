"""Host-side checks of the flow folder tool (spatialaudiogen_amd/flow.py): the pyramid depth rule, parameter validation, the block
bookkeeping and the command line's refusals - and the known answers of the numpy restatement itself (tests/flow_oracle.py), so that
what the device is compared against is pinned without a device."""
import os

import numpy as np
import pytest

import flow_oracle as FO


def test_auto_levels():
    from spatialaudiogen_amd.flow import auto_levels
    assert auto_levels(224, 448) == 5                               # 14 x 28 on the coarsest level
    assert auto_levels(100, 200) == 3                               # 100 = 4 x 25
    assert auto_levels(224, 448, want=8) == 6                       # 7 x 14; 224 = 32 x 7 halves no further
    assert auto_levels(64, 128) == 5 and auto_levels(48, 96) == 4 and auto_levels(16, 32) == 3
    assert auto_levels(7, 9) == 1 and auto_levels(224, 448, want=2) == 2


def test_flow_params_validation():
    from spatialaudiogen_amd.flow import FlowParams
    p = FlowParams()
    assert (p.levels, p.warps, p.iters, p.alpha, p.wrap, p.fuse) == (None, 3, 30, 8., True, 0)
    assert p.levels_for(224, 448) == 5
    for kw in (dict(levels=0), dict(levels=9), dict(warps=0), dict(warps=17), dict(iters=0), dict(iters=1001), dict(alpha=0.),
               dict(alpha=-2.), dict(alpha=float('nan')), dict(alpha=float('inf')), dict(fuse=-1), dict(fuse=9)):
        with pytest.raises(ValueError):
            FlowParams(**kw)
    with pytest.raises(ValueError):
        FlowParams(levels=4).levels_for(36, 64)                     # 36 is not a multiple of 8
    with pytest.raises(ValueError):
        FlowParams(levels=4).levels_for(24, 64)                     # 3 rows on the coarsest level
    with pytest.raises(ValueError):
        FlowParams(levels=1).levels_for(8, 4100)
    assert FlowParams(levels=3, wrap=False).levels_for(40, 72) == 3


def test_params_struct_layout():
    """sagen_flow_params of include/sagen.h: five int32, four bytes of padding, one double."""
    import ctypes as C
    from spatialaudiogen_amd._lib import SagenFlowParams
    assert C.sizeof(SagenFlowParams) == 32 and SagenFlowParams.alpha.offset == 24 and SagenFlowParams.fuse.offset == 16


def test_block_ranges_overlap_by_one_frame():
    from spatialaudiogen_amd.flow import block_ranges
    assert block_ranges(5, 2) == [(0, 2), (1, 4), (3, 5)]
    assert block_ranges(64, 64) == [(0, 64)] and block_ranges(65, 64) == [(0, 64), (63, 65)]
    assert block_ranges(0, 4) == [] and block_ranges(1, 4) == [(0, 1)]
    for n, block in ((17, 4), (130, 64), (7, 1)):
        r = block_ranges(n, block)
        assert all(b - a <= block + 1 for a, b in r) and r[0][0] == 0 and r[-1][1] == n
        assert all(r[i][0] == r[i - 1][1] - 1 for i in range(1, len(r)))             # each block starts on the last frame of the one before
        assert sorted(set(k for a, b in r for k in range(a, b))) == list(range(n))
    with pytest.raises(ValueError):
        block_ranges(5, 0)


def test_command_line_refusals(tmp_path):
    """Every refusal comes before the library or the device is asked for, and before the output folder is touched."""
    from PIL import Image
    from spatialaudiogen_amd import flow as F
    video, out = str(tmp_path / 'video'), str(tmp_path / 'flow')
    with pytest.raises(SystemExit):
        F.main([video, out])                                        # no such folder
    os.makedirs(video)
    with pytest.raises(SystemExit):
        F.main([video, out])                                        # no frame 000000.jpg
    for k in range(2):
        Image.fromarray(np.full((36, 64, 3), 10 * k, np.uint8)).save(os.path.join(video, '%06d.jpg' % k))
    for extra in (['--block', '0'], ['--levels', '4'], ['--levels', '9'], ['--warps', '0'], ['--iters', '2000'], ['--alpha', '0'],
                  ['--format', 'bmp']):
        with pytest.raises(SystemExit):
            F.main([video, out] + extra)
    assert not os.path.exists(out)
    os.makedirs(out)
    open(os.path.join(out, 'notes.txt'), 'w').close()
    with pytest.raises(SystemExit) as e:
        F.main([video, out])
    assert '--overwrite' in str(e.value) and os.listdir(out) == ['notes.txt']
    Image.fromarray(np.zeros((40, 64, 3), np.uint8)).save(os.path.join(video, '000002.jpg'))
    with pytest.raises(SystemExit):
        F.main([video, out, '--overwrite'])                         # frames of two sizes
    assert os.listdir(out) == ['notes.txt']


def test_write_flow_folder_names_an_empty_folder(tmp_path):
    from spatialaudiogen_amd import flow as F
    video = str(tmp_path / 'video')
    os.makedirs(video)
    with pytest.raises(ValueError, match='holds no frame'):
        F.write_flow_folder(video, str(tmp_path / 'flow'))
    assert not os.path.exists(str(tmp_path / 'flow'))


# ---- the restatement's own known answers --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shifted_pair():
    return FO.pattern_frames(64, 128, [(0., 0.), (3.3, 0.)], seed=0)


def test_restatement_recovers_a_known_shift_across_the_seam(shifted_pair):
    flow = FO.optical_flow(shifted_pair, levels=4)[0]
    seam = [0, 1, 126, 127]
    assert np.abs(flow[..., 0] - 3.3).max() <= 0.25 and np.abs(flow[..., 1]).max() <= 0.35
    assert np.abs(flow[:, seam, 0] - 3.3).max() <= 0.25
    clamped = FO.optical_flow(shifted_pair, levels=4, wrap=False)[0]
    assert np.abs(clamped[:, seam, 0] - 3.3).max() > 5.


def test_restatement_identical_frames_and_roll(shifted_pair):
    same = FO.optical_flow(shifted_pair[[0, 0]], levels=4)
    assert same.shape == (1, 64, 128, 2) and not same.any()
    base = FO.optical_flow(shifted_pair, levels=3, iters=5)
    rolled = FO.optical_flow(np.roll(shifted_pair, 4, axis=2), levels=3, iters=5)
    # equal up to rounding only: the warp fetches at the ABSOLUTE coordinate x + u, which rounds differently 4 columns further on
    assert np.abs(rolled - np.roll(base, 4, axis=2)).max() <= 1e-10
    odd = FO.optical_flow(np.roll(shifted_pair, 3, axis=2), levels=3, iters=5)
    assert np.abs(odd - np.roll(base, 3, axis=2)).max() > 1e-3      # the 2 x 2 blocks move: legitimately another flow


def test_restatement_coding_known_answers():
    flow = np.zeros((2, 2, 3, 2), np.float32)
    flow[0, 0, 0] = (3., 0.)            # to the right: atan2 = 0, + pi -> byte 127.5
    flow[0, 0, 1] = (0., 4.)            # down: pi / 2 + pi -> 191.25
    flow[0, 0, 2] = (-5., 0.)           # to the left: pi + pi -> 255
    flow[0, 1, 0] = (0., -2.)           # up: -pi / 2 + pi -> 63.75
    flow[0, 1, 1] = (0.003, 0.)         # below 0.005: angle 0
    pre, limits = FO.encode(flow)
    assert np.allclose(pre[0, :, :, 0], [[127.5, 191.25, 255.], [63.75, 0., 0.]], atol=1e-12)
    assert limits.dtype == np.float32 and np.array_equal(limits, np.array([[0., 5.], [0., 1.]], np.float32))
    assert np.allclose(pre[0, :, :, 2], np.array([[3., 4., 5.], [2., 0.003, 0.]]) / 5. * 255., atol=1e-5)
    assert not pre[..., 1].any() and not pre[1].any()
