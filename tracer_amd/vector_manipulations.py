"""
Host-side helpers with the names of the reference's ray_trace_utils/vector_manipulations.py that
scene construction needs (AABB :92-102; get_angle, get_angles, get_plane_normals, axes_and_angles_between :5-54, :84-90).  The
per-ray minimal rotation `rotate_z_to_normal` (:56-74), a top CPU hotspot of the reference, lives on the device
(trc_rotate_z_to_normal); the host form here serves the host samplers (sampling.py).
"""
import numpy as N


def AABB(vecs):
    """Axis-aligned bounding box of the columns of a (3,n) array: (min point, max point)."""
    return N.amin(vecs, axis=1), N.amax(vecs, axis=1)


def get_angle(v1, v2, signed=False):
    """the angle between two 3-vectors (of any length); signed: negative where their scalar product is"""
    v1, v2 = N.asarray(v1, dtype=float), N.asarray(v2, dtype=float)
    proj = N.dot(v1.T, v2)
    angs = N.arccos(proj / (N.sqrt(N.sum(v1 ** 2)) * N.sqrt(N.sum(v2 ** 2))))
    if signed:
        angs = (1. if proj == 0. else N.sign(proj)) * angs
    return angs


def get_angles(v1, v2, signed=False):
    """the angles between the columns of v1 (3, n) and those of v2 (3, n), or the one vector v2 (3,): UNIT vectors, as in the
    reference, whose arc cosine takes the scalar products as they are"""
    v1, v2 = N.asarray(v1, dtype=float), N.asarray(v2, dtype=float)
    if v2.ndim <= 1 and v1.ndim <= 1:
        return get_angle(v1, v2, signed)
    proj = N.sum(v1 * (v2[:, None] if v2.ndim <= 1 else v2), axis=0)
    angs = N.arccos(proj)
    if signed:
        sign = N.sign(proj)
        sign[sign == 0] = 1.
        angs = sign * angs
    return angs


def get_plane_normals(v1, v2):
    """unit normals of the planes of the rows of v1 (n, 3) and v2 (n, 3) or (3,), as columns (3, n); the x axis where the two are
    parallel.  Two single vectors give one (3,) normal."""
    plane = N.cross(N.asarray(v1, dtype=float), N.asarray(v2, dtype=float)).T
    with N.errstate(divide='ignore', invalid='ignore'):
        plane = plane / N.sqrt(N.sum(plane ** 2, axis=0))
    if plane.ndim == 1:
        return N.array([1., 0., 0.]) if N.isnan(plane[0]) else plane
    plane[:, N.isnan(plane[0])] = N.array([[1., 0., 0.]]).T
    return plane


def axes_and_angles_between(vecs, normal):
    """(axes, angles) of the rotations that take each of vecs (3, n) or (3,) to normal (3, n) or (3,) within the plane of the two:
    the plane's normal and the angle between them"""
    vecs, normal = N.asarray(vecs, dtype=float), N.asarray(normal, dtype=float)
    axes = get_plane_normals(vecs.T, normal.T)
    if vecs.ndim > 1:
        return axes, get_angles(vecs, normal, signed=False)
    return axes, get_angle(vecs, normal, signed=False)


def rotate_z_to_normal(vecs, normals):
    """
    Rotate the columns of vecs (3, n), given about +z, so that `normals` (3, n) or (3,), unit vectors, become their +z, each by the
    minimal rotation in the plane of z and its normal (reference :56-74; the device form is trc_rotate_z_to_normal).
    Host helper for direction samplers, one small rotation matrix per column as in the reference.
    """
    from .spatial_geometry import general_axis_rotation
    vecs = N.asarray(vecs, dtype=float)
    zs = N.zeros(vecs.shape)
    zs[2] = 1.
    axes, angles = axes_and_angles_between(zs, N.asarray(normals, dtype=float))
    out = N.empty_like(vecs)
    for i in range(vecs.shape[1]):
        out[:, i] = vecs[:, i] if angles[i] == 0. else N.dot(general_axis_rotation(axes[:, i], angles[i]), vecs[:, i])
    return out
