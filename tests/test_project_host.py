"""Host-side checks of the frame reprojection (spatialaudiogen_amd/project.py): the face tables, the rotation convention shared with
the renderer, the supersampling rule and the command line's refusals.  No device: where pixels are needed they come from the CPU
twin through ctypes (the geometry it runs is the header the device compiles, csrc/project_core.h)."""
import ctypes as C
import os

import numpy as np
import pytest

import project_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables():
    from spatialaudiogen_amd import project as P
    return [('cube3x2', P.cubemap3x2(), (32, 48), 16, False), ('eac3x2', P.eac3x2(), (32, 48), 16, False),
            ('eac3x2_stereo', P.eac3x2(stereo=True), (48, 64), 16, True)]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_face_centres():
    """Top row +y, +x, -y; bottom row -z, -x, +z (utils.py:126-135: left, front, right over bottom, back, top).  In the stereo
    table the eye is the turned left half: the eye's rows are the frame's columns, its columns run up the frame."""
    want = np.array([[0, 1, 0], [1, 0, 0], [0, -1, 0], [0, 0, -1], [-1, 0, 0], [0, 0, 1]], np.float64)
    for name, proj, (h, w), n, stereo in _tables():
        d = proj.directions(h, w)
        # the centre of a cell: the mean of its four middle pixels
        centre = lambda x0, y0: _unit(d[y0 + n // 2 - 1:y0 + n // 2 + 1, x0 + n // 2 - 1:x0 + n // 2 + 1].reshape(4, 3).mean(0))
        if not stereo:
            cells = [(c * n, r * n) for r in range(2) for c in range(3)]
        else:
            cells = [(r * n, h - (c + 1) * n) for r in range(2) for c in range(3)]
        got = np.stack([centre(x0, y0) for x0, y0 in cells], 0)
        assert np.allclose(got, want, atol=1e-12), (name, got)
        if stereo:
            assert np.isnan(d[:, w // 2:]).all() and not np.isnan(d[:, :w // 2]).any()        # the second eye is never read
        else:
            assert not np.isnan(d).any()


def test_direction_is_continuous_across_the_inner_edges_of_each_row():
    """Exactly: on the shared edge the two cells give the same direction for every position along it.  And on the pixel grid:
    neighbours across an inner edge are about one pixel's angle apart, like neighbours inside a face."""
    from spatialaudiogen_amd import project as P
    q = np.linspace(-1., 1., 9)
    for name, proj, (h, w), n, stereo in _tables():
        faces = proj.faces(h, w)
        by_cell = {(x0, y0): (f, o) for f, (x0, y0, _, o) in enumerate(faces)}
        for (x0, y0), (f, o) in by_cell.items():
            nxt = (x0, y0 - n) if stereo else (x0 + n, y0)         # the next cell of the eye's row
            if nxt not in by_cell:
                continue
            a0, r0, d0 = P.face_vectors(f, o)
            a1, r1, d1 = P.face_vectors(*by_cell[nxt])
            for t in q:
                if stereo:                                           # this cell's top edge is the next one's bottom edge
                    e0, e1 = a0 + t * r0 - d0, a1 + t * r1 + d1
                else:                                                # right edge, left edge
                    e0, e1 = a0 + r0 + t * d0, a1 - r1 + t * d1
                assert np.array_equal(e0, e1), (name, FACE(f), t)
        d = _unit(proj.directions(h, w))
        inner = np.arccos(np.clip((d[:, :n - 1] * d[:, 1:n]).sum(-1), -1., 1.))[:n].max()
        if stereo:
            for x in (0, n):
                for y in (n, 2 * n):
                    step = np.arccos(np.clip((d[y - 1, x:x + n] * d[y, x:x + n]).sum(-1), -1., 1.))
                    assert step.max() <= 1.5 * inner, (name, x, y, step.max(), inner)
        else:
            for y in (0, n):
                for x in (n, 2 * n):
                    step = np.arccos(np.clip((d[y:y + n, x - 1] * d[y:y + n, x]).sum(-1), -1., 1.))
                    assert step.max() <= 1.5 * inner, (name, x, y, step.max(), inner)


def FACE(f):
    from spatialaudiogen_amd import project as P
    return P.FACE_NAMES[f]


def test_tables_agree_with_the_rot90_restatement():
    """Every pixel of every table: the product's rectangle-and-orientation tables give the direction that the index grids of
    tests/project_oracle.py (cut and turned with np.rot90 the way utils.py:116-135 does) give through vrProjector's formulas."""
    for name, proj, (h, w), n, stereo in _tables():
        ys, xs, dirs = PO._dst_samples(PO.cube(eac=proj.kind == 'eac', stereo=stereo), h, w, 1)
        mine = proj.directions(h, w)[ys, xs]
        assert np.allclose(mine, dirs[:, 0, :], atol=1e-12), name


# ---- the rotation convention, through the CPU twin ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def twin():
    from spatialaudiogen_amd import build
    l = C.CDLL(build.build_cpu_twin())
    P, I, SZ = C.c_void_p, C.c_int, C.c_size_t
    l.sagen_reproject.argtypes = [P, I, I, I, P, P, I, I, P, P, I, I, P, SZ, P]
    return l


def _twin_reproject(l, frames, src, dst, size, rot, S):
    frames = np.ascontiguousarray(frames)
    n, h, w = frames.shape[:3]
    out = np.zeros((n, size[0], size[1], 3), np.uint8)
    sp, dp = src.struct(h, w), dst.struct(*size)
    rot = None if rot is None else np.ascontiguousarray(rot, np.float64)
    n_rot = 0 if rot is None else (1 if rot.ndim == 2 else rot.shape[0])
    rc = l.sagen_reproject(frames.ctypes.data, n, h, w, C.addressof(sp), out.ctypes.data, size[0], size[1], C.addressof(dp),
                           None if rot is None else rot.ctypes.data, n_rot, S, None, 0, None)
    assert rc == 0
    return out


def test_rot_is_the_heads_rotation(twin):
    """world = Rot . head: a bright source pixel in world direction s shows up in the view at head direction Rot^T s - and
    head_rotation_matrix of the same angles turns the harmonics of s into those of Rot^T s: picture and sound move together."""
    from spatialaudiogen_amd import ambisonics as A, project as P
    r = np.random.RandomState(12)
    H, W, V = 90, 180, 61
    view = P.perspective(60.)
    head_dirs = _unit(view.directions(V, V))
    pixel_angle = np.arccos(np.clip((head_dirs[V // 2, V // 2] * head_dirs[V // 2, V // 2 + 1]).sum(), -1., 1.))
    er_dirs = P.equirect().directions(H, W)
    for _ in range(20):
        yaw, pitch, roll = r.uniform(-np.pi, np.pi), r.uniform(-1.2, 1.2), r.uniform(-1., 1.)
        rot = A.rotation_xyz(yaw, pitch, roll)
        head = _unit(np.array([1., r.uniform(-0.35, 0.35), r.uniform(-0.35, 0.35)]))      # inside the 60-degree view
        s = rot @ head
        # the source pixel closest to s, lit
        iy, ix = np.unravel_index(np.argmax((er_dirs * s).sum(-1)), (H, W))
        frame = np.zeros((1, H, W, 3), np.uint8)
        frame[0, iy, ix] = 255
        s_pix = er_dirs[iy, ix]
        out = _twin_reproject(twin, frame, P.equirect(), view, (V, V), rot, 1)[0, :, :, 0].astype(np.float64)
        assert out.max() > 60
        seen = _unit((head_dirs * out[..., None]).sum((0, 1)))      # the bright spot's centroid, as a head direction
        off = np.arccos(np.clip(seen @ (rot.T @ s_pix), -1., 1.))
        assert off < 1.5 * pixel_angle, (off, pixel_angle)
        m = A.head_rotation_matrix(1, yaw, pitch, roll)
        assert np.allclose(m @ A.sh_order1(*A.to_polar(s)), A.sh_order1(*A.to_polar(rot.T @ s)), atol=1e-9)


def test_view_trajectory_mirrors_head_trajectory():
    from spatialaudiogen_amd import ambisonics as A, project as P, render as R
    yaw, pitch = [0., 30., -100.], [0., 10., 20.]
    rots = P.view_trajectory(yaw, pitch, 5.)
    heard = R.head_trajectory(1, yaw, pitch, 5.)
    assert rots.shape == (3, 3, 3) and heard.shape == (3, 4, 4)
    for k in range(3):
        assert np.allclose(rots[k] @ rots[k].T, np.eye(3), atol=1e-12)
        assert np.allclose(heard[k], A.sh_rotation(1, rots[k].T), atol=1e-12)
    assert np.allclose(P.view_trajectory(90.)[0] @ [1., 0., 0.], [0., 1., 0.], atol=1e-12)      # yaw +90: the head looks left


def test_auto_supersample():
    from spatialaudiogen_amd import project as P
    er = P.equirect()
    assert P.auto_supersample(er, (1920, 3840), er, (224, 448)) == 8
    assert P.auto_supersample(er, (224, 448), er, (224, 448)) == 1
    assert P.auto_supersample(er, (112, 224), er, (224, 448)) == 1
    assert P.auto_supersample(er, (960, 1920), er, (240, 480)) == 4
    # EAC faces of 1080: 2 n / pi = 687.5 pixels per radian against 448 / 2 pi = 71.3 -> 10 -> 8; a 90-degree view of 1280: 640
    assert P.auto_supersample(P.eac3x2(), (2160, 3240), er, (224, 448)) == 8
    assert P.auto_supersample(er, (1080, 1920), P.perspective(90.), (720, 1280)) == 1
    assert P.auto_supersample(P.equirect('top_bottom'), (1792, 1792), er, (224, 448)) == 4


def test_descriptors_refuse_what_a_frame_cannot_hold():
    from spatialaudiogen_amd import project as P
    for bad in (lambda: P.perspective(0.), lambda: P.perspective(180.), lambda: P.equirect('side_by_side'),
                lambda: P.eac3x2().struct(2160, 3840),             # cells of 1080 x 1280
                lambda: P.eac3x2(stereo=True).struct(32, 48), lambda: P.Projection('er', rect=(0, 0, 49, 32)).struct(32, 48)):
        with pytest.raises(ValueError):
            bad()
    s = P.equirect('top_bottom').struct(38, 20)
    assert (s.kind, s.x0, s.y0, s.w, s.h) == (0, 0, 0, 20, 19)
    s = P.eac3x2().struct(32, 48)
    assert [(f.x0, f.y0, f.w, f.h, f.orient) for f in s.face] == [(16, 0, 16, 16, 0), (16, 16, 16, 16, 3), (0, 0, 16, 16, 0), (32, 0, 16, 16, 0),
                                                                  (32, 16, 16, 16, 1), (0, 16, 16, 16, 1)]


# ---- the command line refuses on the host -----------------------------------------------------------------------------------------
def _write_frames(folder, n, h, w):
    from PIL import Image
    os.makedirs(folder)
    for k in range(n):
        Image.fromarray(np.full((h, w, 3), 40 * k, np.uint8)).save(os.path.join(folder, '%06d.jpg' % k))


def test_command_line_refuses_before_any_device_use(tmp_path, monkeypatch):
    from spatialaudiogen_amd import _lib, project as P

    def no_device(*a, **k):
        raise AssertionError('the library was loaded before the refusal')
    monkeypatch.setattr(_lib, 'lib', no_device)
    in_dir, out_dir = str(tmp_path / 'in'), str(tmp_path / 'out')
    _write_frames(in_dir, 2, 32, 48)
    base = [in_dir, out_dir, '--size', '24', '48']
    with pytest.raises(SystemExit):
        P.main(base + ['--from', 'fisheye', '--to', 'er'])                           # an unknown --from
    with pytest.raises(SystemExit) as e:
        P.main(base + ['--from', 'eac', '--to', 'view'])                             # a view without its field of view
    assert '--hfov' in str(e.value)
    with pytest.raises(SystemExit) as e:
        P.main([str(tmp_path / 'nowhere'), out_dir, '--size', '24', '48', '--from', 'eac', '--to', 'er'])
    assert 'not a folder' in str(e.value)
    os.makedirs(out_dir)
    open(os.path.join(out_dir, '000000.jpg'), 'wb').close()
    with pytest.raises(SystemExit) as e:
        P.main(base + ['--from', 'eac', '--to', 'er'])                               # frames are there already
    assert '--overwrite' in str(e.value) and os.listdir(out_dir) == ['000000.jpg']
    for extra, word in ((['--from', 'eac_stereo', '--to', 'er'], '3 n x 4 n'), (['--from', 'eac', '--to', 'cube', '--overwrite'], '2 n x 3 n'),
                        (['--from', 'eac', '--to', 'er', '--supersample', '9', '--overwrite'], '1..8'),
                        (['--from', 'eac', '--to', 'er', '--hfov', '90', '--overwrite'], '--hfov')):
        with pytest.raises(SystemExit) as e:
            P.main(base + extra)
        assert word in str(e.value), (extra, str(e.value))
    assert os.listdir(out_dir) == ['000000.jpg']                                     # no refusal removed anything
    empty = str(tmp_path / 'empty')
    os.makedirs(empty)
    with pytest.raises(SystemExit):
        P.main([empty, out_dir, '--size', '24', '48', '--from', 'eac', '--to', 'er', '--overwrite'])
