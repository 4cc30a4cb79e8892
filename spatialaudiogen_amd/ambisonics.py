"""Ambisonic geometry on the host: the speaker mesh and the real spherical-harmonic matrix the power-map kernels project onto
(reference: pyutils/ambisonics/distance.py:9-13 mesh, common.py:151-178 harmonics, decoder.py:9-28 'projection' decoding), and - for
the renderings of render.py - the harmonics of orders 1 and 2 at arbitrary directions, sound-field rotations and decode matrices.
ACN channel order (W,Y,Z,X, ...) with SN3D normalisation, as everywhere in the path."""
import numpy as np


def spherical_mesh(angular_res):
    """(phi, nu) grids in radians: azimuth from +180 down to -180 (exclusive) in steps of `angular_res` degrees along the
    columns, elevation from -90 to +90 along the rows (distance.py:9-13)."""
    phi = np.flip(np.arange(-180., 180., angular_res)) / 180. * np.pi
    nu = np.arange(-90., 90.1, angular_res) / 180. * np.pi
    return np.meshgrid(phi, nu)


def sh_order1(phi, nu):
    """Order-1 real harmonics, ACN/SN3D: [1, cos(nu) sin(phi), sin(nu), cos(nu) cos(phi)] (common.py:151-157)."""
    phi, nu = np.asarray(phi, np.float64), np.asarray(nu, np.float64)
    return np.stack([np.ones_like(phi), np.cos(nu) * np.sin(phi), np.sin(nu), np.cos(nu) * np.cos(phi)], -1)


def sh_matrix(angular_res):
    """[P, 4] projection matrix of the mesh, row-major over (elevation row, azimuth column)."""
    phi, nu = spherical_mesh(angular_res)
    return sh_order1(phi.reshape(-1), nu.reshape(-1))


def mesh_shape(angular_res):
    phi, _ = spherical_mesh(angular_res)
    return phi.shape


def angular_distance(angular_res):
    """[P, P] fp64 great-circle distance between the mesh's directions, the ground distance of the EMD metric (distance.py:101-110);
    same row-major node order as sh_matrix.  The reference's arccos(clip(u_i . u_j, -1, 1)) turns the rounding of a dot product
    of 1 into 1.5e-8 rad on the diagonal and between the coincident pole nodes, which pyemd's cost quantisation (max C / 1e6) then
    rounds back to 0; atan2(|u_i x u_j|, u_i . u_j) gives those exactly 0 (to 1e-16) and equals the arccos form everywhere else."""
    phi, nu = spherical_mesh(angular_res)
    phi, nu = phi.reshape(-1), nu.reshape(-1)
    u = np.stack([np.cos(nu) * np.cos(phi), np.cos(nu) * np.sin(phi), np.sin(nu)], -1)
    cross = np.linalg.norm(np.cross(u[:, None, :], u[None, :, :]), axis=-1)
    return np.arctan2(cross, u @ u.T)


# ---- orders 1 and 2 at arbitrary directions, rotations, decoders (fp64; the host side of render.py) --------------------------------
def num_channels(order):
    if order not in (1, 2):
        raise ValueError('ambisonic order %r is not supported (1 or 2)' % (order,))
    return (order + 1) ** 2


def sh_matrix_at(phi, nu, order=1):
    """[..., (order + 1)^2] real harmonics at azimuth phi / elevation nu (radians), ACN / SN3D, in closed form - the values of
    common.py:151-157 ((-1)^m N_nm P_n^|m|(sin nu) cos / sin(|m| phi), whose sign cancels the Condon-Shortley phase):
    [1, cos nu sin phi, sin nu, cos nu cos phi, (sqrt3/2) cos^2 nu sin 2phi, (sqrt3/2) sin 2nu sin phi, (3 sin^2 nu - 1) / 2,
    (sqrt3/2) sin 2nu cos phi, (sqrt3/2) cos^2 nu cos 2phi]."""
    C = num_channels(order)
    phi, nu = np.broadcast_arrays(np.asarray(phi, np.float64), np.asarray(nu, np.float64))
    cn, sn = np.cos(nu), np.sin(nu)
    rows = [np.ones_like(phi), cn * np.sin(phi), sn, cn * np.cos(phi)]
    if order == 2:
        h = np.sqrt(3.) / 2.
        s2n = np.sin(2 * nu)
        rows += [h * cn * cn * np.sin(2 * phi), h * s2n * np.sin(phi), (3. * sn * sn - 1.) / 2., h * s2n * np.cos(phi),
                 h * cn * cn * np.cos(2 * phi)]
    return np.stack(rows[:C], -1)


def to_polar(xyz):
    """Cartesian [..., 3] (x front, y left, z up) -> (phi, nu) as Position.calc_polar does (position.py:34-37)."""
    xyz = np.asarray(xyz, np.float64)
    return np.arctan2(xyz[..., 1], xyz[..., 0]), np.arctan2(xyz[..., 2], np.hypot(xyz[..., 0], xyz[..., 1]))


def to_cartesian(phi, nu, r=1.):
    """position.py:29-32."""
    phi, nu = np.asarray(phi, np.float64), np.asarray(nu, np.float64)
    return np.stack([r * np.cos(phi) * np.cos(nu), r * np.sin(phi) * np.cos(nu), r * np.sin(nu) * np.ones_like(phi)], -1)


def rotation_xyz(yaw, pitch=0., roll=0.):
    """The 3x3 matrix Rot = Rz(yaw) . Ry(pitch) . Rx(roll), right-handed, x front, y left, z up (radians):

        Rz(a) = [[cos a, -sin a, 0],      Ry(b) = [[ cos b, 0, sin b],      Rx(g) = [[1, 0,      0     ],
                 [sin a,  cos a, 0],               [ 0,     1, 0    ],               [0, cos g, -sin g],
                 [0,      0,     1]]               [-sin b, 0, cos b]]               [0, sin g,  cos g]]
    """
    ca, sa, cb, sb, cg, sg = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[ca, -sa, 0.], [sa, ca, 0.], [0., 0., 1.]])
    ry = np.array([[cb, 0., sb], [0., 1., 0.], [-sb, 0., cb]])
    rx = np.array([[1., 0., 0.], [0., cg, -sg], [0., sg, cg]])
    return rz @ ry @ rx


def _fit_directions(count=64):
    """Fixed, well-spread unit vectors (a Fibonacci spiral): the sample the rotation matrices are fitted on."""
    i = np.arange(count) + 0.5
    z = 1. - 2. * i / count
    az = np.pi * (1. + np.sqrt(5.)) * i
    rho = np.sqrt(1. - z * z)
    return np.stack([rho * np.cos(az), rho * np.sin(az), z], -1)


def sh_rotation(order, rot):
    """The C x C matrix M with Y(rot . d) = M . Y(d) for every direction d, for a 3x3 rotation `rot` (Y = sh_matrix_at).  M is block
    diagonal per order; each block is obtained by solving Y(d_i) . M^T = Y(rot . d_i) in the least-squares sense over 64 fixed
    directions (exact up to rounding: the rotated harmonics of an order span that order)."""
    C = num_channels(order)
    d = _fit_directions()
    y0 = sh_matrix_at(*to_polar(d), order=order)
    y1 = sh_matrix_at(*to_polar(d @ np.asarray(rot, np.float64).T), order=order)
    m = np.zeros((C, C))
    lo = 0
    for n in range(order + 1):                       # one block per order: nothing leaks between orders, W stays exactly W
        hi = (n + 1) ** 2
        m[lo:hi, lo:hi] = np.linalg.lstsq(y0[:, lo:hi], y1[:, lo:hi], rcond=None)[0].T
        lo = hi
    return m


def rotation_matrix(order, yaw, pitch=0., roll=0.):
    """The C x C matrix M of the SOUND-FIELD rotation Rot = rotation_xyz(yaw, pitch, roll) = Rz(yaw) . Ry(pitch) . Rx(roll) (radians),
    defined by Y(Rot . d) = M . Y(d) for every direction d: a source at azimuth phi moves to phi + yaw.  Order 1 with
    pitch = roll = 0 equals feeder.rotation_matrix_z(yaw) (the reference's augmentation, feeder.py:92-101).  A listener who turns
    their head by an angle hears the field rotated by the inverse (head_rotation_matrix)."""
    return sh_rotation(order, rotation_xyz(yaw, pitch, roll))


def head_rotation_matrix(order, yaw, pitch=0., roll=0.):
    """What a listener hears whose head is turned by Rot = rotation_xyz(yaw, pitch, roll): the field rotated by Rot^-1 = Rot^T."""
    return sh_rotation(order, rotation_xyz(yaw, pitch, roll).T)


def decode_matrix(positions, order=1, method='projection'):
    """D [S, C] with speaker feeds = ambi . D^T (AmbiDecoder, decoder.py:16-28): 'projection' D = Y, 'pseudoinv' D = pinv(Y)^T, Y the
    harmonics at the speakers.  positions: cartesian [S, 3] (any radius)."""
    y = sh_matrix_at(*to_polar(np.asarray(positions, np.float64).reshape(-1, 3)), order=order)
    if method == 'projection':
        return y
    if method == 'pseudoinv':
        return np.linalg.pinv(y).T
    raise ValueError('unknown decoding method %r (projection or pseudoinv)' % (method,))


def ring_positions(order, radius=1.):
    """The reference's loudspeaker ring (binauralizer.py:137-138): S = 2 C speakers at phi_s = (2 s / S - 1) pi, nu = 0."""
    S = 2 * num_channels(order)
    phi = (2. * np.arange(S) / float(S) - 1.) * np.pi
    return to_cartesian(phi, np.zeros(S), radius)
