"""Frame reprojection on the device (csrc/project.hip through ops.reproject / project.Projector) against the fp64 restatement of
tests/project_oracle.py, which reaches every cube pixel through the reference's own np.rot90 index grids and vrProjector's own
face formulas instead of the product's face table.

PIXEL RULE (the blend rule of tests/test_gpu_overlay.py): got == floor(pre + 0.5) wherever the mean before rounding `pre` is farther
than EDGE = 1e-6 levels from a k + 0.5 edge; elsewhere either neighbour passes.  Coordinates, weights and sums are fp64 on both
sides, so the two differ by rounding of order 1e-10 levels (|value| <= 255, a few dozen operations, sin / cos / atan2 to an ulp or
two of arguments <= pi scaled by <= 16384 pixels); 1e-6 leaves four orders of margin.  Each parity case first asserts ON THE
RESTATEMENT that at most 0.1 % of the values lie within EDGE of an edge and, for cube sources, that no sample's direction comes
within 1e-9 of a cube edge (there either face is right).  Inputs: random bytes, a generic rotation (yaw 0.3, pitch 0.2, roll 0.1).

The op-level cases (OP_CASES) also run against the CPU twin in a container without a GPU (tests/test_cpu_twin_project.py)."""
import os

import numpy as np
import pytest

import project_oracle as PO
from util import ensure_lib

pytestmark = pytest.mark.gpu

EDGE = 1e-6
OP_CASES = ('test_parity or test_identity_returns_the_input or test_yaw_by_whole_pixels_is_a_roll or test_eac_round_trip or '
            'test_split_clip_gives_equal_bytes or test_error_codes_and_untouched_output or test_unwritten_pixels_keep_their_bytes')


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


def _frames(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)


def _rot(k=0):
    from spatialaudiogen_amd import ambisonics
    return ambisonics.rotation_xyz(0.3 + 0.37 * k, 0.2 - 0.11 * k, 0.1 + 0.23 * k)


def _run(frames, src, dst, size, rot=None, S=1):
    from spatialaudiogen_amd import ops
    dev = _dev()
    h, w = frames.shape[1:3]
    r = None if rot is None else _t(np.asarray(rot, np.float64), dev)
    return ops.reproject(_t(frames, dev), src.struct(h, w), size, dst.struct(*size), r, S).cpu().numpy()


def assert_pixel_rule(got, pre, margin, cube_source, what=''):
    live = ~np.isnan(pre)
    assert live.any()
    p, g = pre[live], got[live].astype(np.float64)
    near = np.abs(p - np.floor(p) - 0.5) <= EDGE
    assert near.mean() <= 1e-3, 'input condition: %d of %d values within %g of a rounding edge' % (near.sum(), near.size, EDGE)
    if cube_source:
        assert margin is not None and margin > 1e-9, 'input condition: a sample %g from a cube edge' % margin
    ok = np.where(near, (g == np.floor(p)) | (g == np.floor(p) + 1.), g == np.floor(p + 0.5))
    print('%s: %d values, %d within %g of an edge, %d wrong, worst |got - pre| %.6f' % (what, p.size, near.sum(), EDGE, (~ok).sum(), np.abs(g - p).max()))
    assert ok.all(), '%d of %d values break the rule (worst |got - pre| %.3g)' % ((~ok).sum(), ok.size, np.abs(g - p)[~ok].max())
    assert not got[~live].any()                       # pixels of no rectangle: the fresh destination's zeros


def _proj():
    from spatialaudiogen_amd import project
    return project


# name -> (source, its frame size, restatement's source, destination, its size, restatement's destination, frames, rotations, S)
def _cases():
    P = _proj()
    er, tb = P.equirect(), P.equirect('top_bottom')
    odd = P.Projection('er', rect=(0, 19, 38, 19))                   # the SECOND eye of a 38 x 38 top-bottom frame: y0 = 19
    cube, eac, eacs, view = P.cubemap3x2(), P.eac3x2(), P.eac3x2(stereo=True), P.perspective(90.)
    return {
        'er37x74_er20x40_S3': (er, (37, 74), PO.er(), er, (20, 40), PO.er(), 1, 'one', 3),           # odd row bytes: 222
        'er48x96_er24x48_S2': (er, (48, 96), PO.er(), er, (24, 48), PO.er(), 2, 'one', 2),
        'er31x62_er16x32_S2': (er, (31, 62), PO.er(), er, (16, 32), PO.er(), 1, 'one', 2),
        'er31x62_er16x32_S1': (er, (31, 62), PO.er(), er, (16, 32), PO.er(), 1, 'one', 1),
        'er_upscale_S1': (er, (9, 18), PO.er(), er, (20, 40), PO.er(), 1, 'one', 1),
        'top_bottom_first_eye': (tb, (30, 40), PO.er((0, 0, 40, 15)), er, (12, 24), PO.er(), 1, 'one', 2),
        'top_bottom_odd_y0': (odd, (38, 38), PO.er((0, 19, 38, 19)), er, (12, 24), PO.er(), 1, 'one', 2),
        'cube3x2_er_S1': (cube, (32, 48), PO.cube(), er, (24, 48), PO.er(), 1, 'one', 1),
        'cube3x2_er_S2': (cube, (32, 48), PO.cube(), er, (24, 48), PO.er(), 1, 'one', 2),
        'eac3x2_er_S1': (eac, (32, 48), PO.cube(eac=True), er, (24, 48), PO.er(), 1, 'one', 1),
        'eac3x2_er_S3': (eac, (32, 48), PO.cube(eac=True), er, (24, 48), PO.er(), 1, 'one', 3),
        'eac3x2_er_unrotated_S2': (eac, (32, 48), PO.cube(eac=True), er, (24, 48), PO.er(), 1, None, 2),
        'eac3x2_stereo_er_S2': (eacs, (48, 64), PO.cube(eac=True, stereo=True), er, (24, 48), PO.er(), 1, 'one', 2),
        'er_cube3x2_S2': (er, (48, 96), PO.er(), cube, (32, 48), PO.cube(), 1, 'one', 2),
        'er_eac3x2_S2': (er, (48, 96), PO.er(), eac, (32, 48), PO.cube(eac=True), 1, 'one', 2),
        'er_eac3x2_stereo_S1': (er, (48, 96), PO.er(), eacs, (48, 64), PO.cube(eac=True, stereo=True), 1, 'one', 1),
        'eac_cube_S2': (eac, (32, 48), PO.cube(eac=True), cube, (20, 30), PO.cube(), 1, 'one', 2),
        'er_view_per_frame_S2': (er, (48, 96), PO.er(), view, (30, 40), PO.view(90.), 5, 'each', 2),
        'er_view_one_for_all_S3': (er, (48, 96), PO.er(), view, (30, 40), PO.view(90.), 5, 'one', 3),
        'eac_view_per_frame_S1': (eac, (32, 48), PO.cube(eac=True), view, (30, 40), PO.view(90.), 3, 'each', 1),
        'more_than_one_workgroup': (er, (40, 80), PO.er(), er, (19, 41), PO.er(), 1, 'one', 1),        # 779 pixels: 4 workgroups, a ragged one
    }


CASE_NAMES = ['er37x74_er20x40_S3', 'er48x96_er24x48_S2', 'er31x62_er16x32_S2', 'er31x62_er16x32_S1', 'er_upscale_S1', 'top_bottom_first_eye',
              'top_bottom_odd_y0', 'cube3x2_er_S1', 'cube3x2_er_S2', 'eac3x2_er_S1', 'eac3x2_er_S3', 'eac3x2_er_unrotated_S2', 'eac3x2_stereo_er_S2',
              'er_cube3x2_S2', 'er_eac3x2_S2', 'er_eac3x2_stereo_S1', 'eac_cube_S2', 'er_view_per_frame_S2', 'er_view_one_for_all_S3',
              'eac_view_per_frame_S1', 'more_than_one_workgroup']


@pytest.mark.parametrize('name', CASE_NAMES)
def test_parity(name):
    cases = _cases()
    assert sorted(cases) == sorted(CASE_NAMES)
    src, shape, osrc, dst, size, odst, n, rots, S = cases[name]
    frames = _frames(n, shape[0], shape[1], len(name) + S)
    rot = None if rots is None else (_rot() if rots == 'one' else np.stack([_rot(k) for k in range(n)], 0))
    got = _run(frames, src, dst, size, rot, S)
    assert got.shape == (n,) + tuple(size) + (3,) and got.dtype == np.uint8
    pre, margin = PO.reproject(frames, osrc, odst, size, rot, S)
    if name == 'eac3x2_er_unrotated_S2':
        # an even number of samples per pixel straddles the cube edges az = +-45, +-135 degrees (48 columns put them on pixel borders)
        # instead of sitting on them; the rule below then has to hold at the seams too
        assert margin > 1e-9
    assert_pixel_rule(got, pre, margin, osrc['kind'] != 'er', name)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(37, 74), (24, 48), (5, 7)])
def test_identity_returns_the_input(h, w):
    P = _proj()
    frames = _frames(2, h, w, h)
    assert np.array_equal(_run(frames, P.equirect(), P.equirect(), (h, w), None, 1), frames)


@pytest.mark.parametrize('k', [1, 7, -5, 37])
def test_yaw_by_whole_pixels_is_a_roll(k):
    """Rot = rotation_xyz(2 pi k / W)^T moves every column by k: the feeder's yaw augmentation np.roll(frames, -k, axis=2)."""
    from spatialaudiogen_amd import ambisonics
    P = _proj()
    h, w = 37, 74
    frames = _frames(2, h, w, 100 + k)
    rot = ambisonics.rotation_xyz(2. * np.pi * k / w).T
    assert np.array_equal(_run(frames, P.equirect(), P.equirect(), (h, w), rot, 1), np.roll(frames, -k, axis=2))


def test_eac_round_trip():
    """ER 256 x 512 -> eac3x2 with faces of n = 192 -> ER 256 x 512, S = 1, of the frame painted f(d) = 127.5 (1 + d): every value
    stays within 2 levels of the painting.  The bound, from the sizes: f changes by <= 127.5 levels per radian.
      painting:   the uint8 painting is f + e0, |e0| <= 0.5.
      ER -> EAC:  a face pixel takes four painted values (each f + <= 0.5) bilinearly: interpolation error <= (hx^2 + hy^2) / 8 * 127.5
                  = 0.005 for hx = hy = 2 pi / 512; above the first / below the last row centre the fetch is clamped, i.e. displaced
                  by <= half a row = pi / 512 rad = 0.78 levels; rounding adds <= 0.5.  So a face pixel is f + <= 0.5 + 0.79 + 0.5
                  near a pole and f + <= 0.5 + 0.01 + 0.5 elsewhere.
      EAC -> ER:  face pixels are pi / (2 n) rad apart in the face's own angles (a, b), and |d dir / d a| <= sec a <= sqrt 2 on a face.
                  Interpolation error <= 2 (pi / 384)^2 / 8 * 4 * 127.5 = 0.009; within half a face pixel of a face edge the fetch is
                  clamped (no filtering across faces), i.e. displaced by <= pi / (4 n) rad = 0.0041 * sqrt 2 * 127.5 = 0.74 levels -
                  far from the poles, which sit at face centres; rounding adds <= 0.5.
      total:      |out - painting| <= 0.5 + (0.5 + 0.5) + max(0.79, 0.74 + 0.01) + 0.01 + 0.5 < 3, and both are integers: <= 2.
    A wrong turn or a swapped face in either table moves a pixel by tens of levels."""
    P = _proj()
    painted, _ = PO.direction_painting(256, 512)
    eac = _run(painted[None], P.equirect(), P.eac3x2(), (384, 576), None, 1)
    back = _run(eac, P.eac3x2(), P.equirect(), (256, 512), None, 1)
    err = np.abs(back[0].astype(int) - painted.astype(int))
    print('EAC round trip: worst %d levels, mean %.3f' % (err.max(), err.mean()))
    assert err.max() <= 2


def test_split_clip_gives_equal_bytes():
    """5 frames with 5 rotations at once, and as 2 + 3: Projector keeps nothing between calls."""
    P = _proj()
    dev = _dev()
    frames = _frames(5, 48, 96, 3)
    rot = P.view_trajectory([0., 20., 40., 60., 80.], [5., 4., 3., 2., 1.], 10.)
    assert rot.shape == (5, 3, 3)
    pr = P.Projector(P.equirect(), P.perspective(90.), (30, 40), supersample=2, device=dev)
    whole = pr.process(_t(frames, dev), rot).cpu().numpy()
    a, b = pr.process(_t(frames[:2], dev), rot[:2]).cpu().numpy(), pr.process(_t(frames[2:], dev), rot[2:]).cpu().numpy()
    assert np.array_equal(np.concatenate([a, b], 0), whole)
    assert np.array_equal(whole, _run(frames, P.equirect(), P.perspective(90.), (30, 40), rot, 2))
    assert len({whole[k].tobytes() for k in range(5)}) == 5         # the rotations differ, so do the views
    # auto supersample: ER 48 x 96 -> ER 12 x 24 takes S = 4
    auto = P.Projector(P.equirect(), P.equirect(), (12, 24), device=dev)
    assert np.array_equal(auto.process(_t(frames[:1], dev)).cpu().numpy(), _run(frames[:1], P.equirect(), P.equirect(), (12, 24), None, 4))


def test_unwritten_pixels_keep_their_bytes():
    """A destination rectangle smaller than its frame: ops.reproject(out=...) writes the rectangle and nothing else."""
    import torch
    from spatialaudiogen_amd import ops
    P = _proj()
    dev = _dev()
    frames = _frames(1, 20, 40, 9)
    dst = P.Projection('er', rect=(3, 5, 16, 8))
    out = torch.full((1, 15, 21, 3), 201, dtype=torch.uint8, device=dev)
    ops.reproject(_t(frames, dev), P.equirect().struct(20, 40), (15, 21), dst.struct(15, 21), _t(_rot(), dev), 2, out=out)
    got = out.cpu().numpy()
    pre, _ = PO.reproject(frames, PO.er(), PO.er((3, 5, 16, 8)), (15, 21), _rot(), 2)
    inside = ~np.isnan(pre)
    assert inside.sum() == 16 * 8 * 3 and (got[~inside] == 201).all()
    assert_pixel_rule(np.where(inside, got, 0), pre, None, False, 'rectangle inside the destination')


# ---- error codes ------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_untouched_output():
    import ctypes as C
    import torch
    from spatialaudiogen_amd import _lib, ops
    P = _proj()
    dev = _dev()
    l = _lib.lib()
    n, h, w, H, W = 3, 32, 48, 12, 24
    src = _t(_frames(n, h, w, 1), dev)
    dst = torch.full((n, H, W, 3), 77, dtype=torch.uint8, device=dev)
    rot = _t(np.stack([_rot(k) for k in range(n)], 0), dev)
    stream = ops._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    er_s, eac_s, er_d, view_d = P.equirect().struct(h, w), P.eac3x2().struct(h, w), P.equirect().struct(H, W), P.perspective(90.).struct(H, W)

    def call(s=src, n_=n, sh=h, sw=w, sp=eac_s, d=dst, dh=H, dw=W, dp=er_d, r=rot, n_rot=n, S=2):
        return l.sagen_reproject(ptr(s) if s is not None else None, n_, sh, sw, C.byref(sp) if sp is not None else None,
                                 ptr(d) if d is not None else None, dh, dw, C.byref(dp) if dp is not None else None,
                                 ptr(r) if r is not None else None, n_rot, S, None, 0, stream)

    def changed(**kw):
        base = P.eac3x2().struct(h, w)
        for k, v in kw.items():
            setattr(base.face[2], k, v)
        return base

    assert l.sagen_reproject_scratch_bytes(n, H, W, 2) == 0
    # null arguments
    for kw in (dict(s=None), dict(d=None), dict(sp=None), dict(dp=None), dict(r=None)):
        assert call(**kw) == -1, kw
    # bad shapes
    tall = P.Projection('er', rect=(0, 16, w, 16)).struct(h, w)
    tall.h = 17                                                     # rows 16..32 of a 32-row frame
    wide = P.equirect().struct(H, W)
    wide.x0, wide.y0, wide.w, wide.h = 1, 0, W, H
    bad_view_lo, bad_view_hi = P.perspective(90.).struct(H, W), P.perspective(90.).struct(H, W)
    bad_view_lo.hfov, bad_view_hi.hfov = 0., np.pi
    for kw in (dict(sp=tall), dict(dp=wide), dict(sp=changed(w=15)), dict(sp=changed(x0=40)), dict(sp=changed(y0=-1)),
               dict(sp=changed(orient=8)), dict(n_rot=2), dict(n_rot=n + 1), dict(dp=bad_view_lo), dict(dp=bad_view_hi), dict(n_=-1),
               dict(dh=0), dict(sw=0)):
        assert call(**kw) == -2, (kw, l.sagen_last_error())
    # unsupported
    unknown = P.equirect().struct(h, w)
    unknown.kind = 9
    for kw in (dict(S=0), dict(S=9), dict(sw=16385, sp=er_s), dict(dh=16385), dict(n_=65536, n_rot=1), dict(sp=view_d), dict(sp=unknown)):
        assert call(**kw) == -3, (kw, l.sagen_last_error())
    assert b'supersample' in (l.sagen_last_error() if call(S=9) == -3 else b'')
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((dst == 77).all())                                  # every refused call left the destination alone
    # n == 0: success, nothing looked at
    assert call(n_=0, s=None, d=None, r=None, n_rot=0) == 0 and call(n_=0) == 0
    assert bool((dst == 77).all())
    assert call(dp=view_d) == 0 and call(n_rot=1) == 0 and call(n_rot=0, r=None) == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert not bool((dst == 77).all())
    # the Python layer refuses before the library is asked
    with pytest.raises(TypeError):
        ops.reproject(src.float(), eac_s, (H, W), er_d)
    with pytest.raises(ValueError):
        P.eac3x2().struct(30, 48)                                   # cells of 15 x 16
    with pytest.raises(ValueError):
        P.Projector(P.perspective(90.), P.equirect(), (H, W), device=dev)
    assert ops.reproject(src[:0], eac_s, (H, W), er_d).shape == (0, H, W, 3)


# ---- command line (needs the device) ------------------------------------------------------------------------------------------------
def test_command_line_end_to_end(tmp_path, capsys):
    """EAC jpgs -> the 224 x 448 folder deploy reads (png here, to compare bytes), and a head that turns across the clip."""
    import torch
    assert torch.cuda.is_available()
    ensure_lib()
    from PIL import Image
    from spatialaudiogen_amd import project as P
    from spatialaudiogen_amd.feeder import imread
    in_dir, out_dir, view_dir = str(tmp_path / 'eac'), str(tmp_path / 'er'), str(tmp_path / 'view')
    os.makedirs(in_dir)
    painted, _ = PO.direction_painting(64, 128)
    eac = _run(np.stack([np.roll(painted, 9 * k, axis=1) for k in range(5)], 0), P.equirect(), P.eac3x2(), (64, 96), None, 1)
    for k in range(5):
        Image.fromarray(eac[k]).save(os.path.join(in_dir, '%06d.jpg' % k), quality=95)
    decoded = np.stack([imread(os.path.join(in_dir, '%06d.jpg' % k)) for k in range(5)], 0)
    P.main([in_dir, out_dir, '--from', 'eac', '--to', 'er', '--size', '224', '448', '--format', 'png', '--block', '2'])
    assert 'wrote 5 frames of 224x448 to %s (eac -> er, supersample 1)' % out_dir in capsys.readouterr().out
    got = np.stack([imread(os.path.join(out_dir, '%06d.png' % k)) for k in range(5)], 0)
    assert np.array_equal(got, _run(decoded, P.eac3x2(), P.equirect(), (224, 448), None, 1))
    with pytest.raises(SystemExit):
        P.main([in_dir, out_dir, '--from', 'eac', '--to', 'er', '--size', '224', '448'])
    P.main([in_dir, out_dir, '--from', 'eac', '--to', 'er', '--size', '224', '448', '--overwrite'])
    assert sorted(os.listdir(out_dir)) == ['%06d.jpg' % k for k in range(5)]
    P.main([in_dir, view_dir, '--from', 'eac', '--to', 'view', '--size', '30', '40', '--hfov', '90', '--yaw', '0', '80', '--pitch', '10',
            '--supersample', '2', '--format', 'png'])
    rot = P.view_trajectory(np.linspace(0., 80., 5), 10.)
    got = np.stack([imread(os.path.join(view_dir, '%06d.png' % k)) for k in range(5)], 0)
    assert np.array_equal(got, _run(decoded, P.eac3x2(), P.perspective(90.), (30, 40), rot, 2))
