"""
The scene, the maps and the host reference of the flux-map chart tests (test_gpu_fluxmap_charts.py on the device,
test_fluxmap_charts_host.py for what can be said without one): flux maps binned in the coordinates of the receiver's shape --
cylinder (z, phi), polar (r, phi), sphere (theta, phi) -- beside the plain (x, y) of fluxmap_scene.py.

The scene is a small receiver assembly over a round floor, turned by a general rotation and moved off the origin:

  0  floor     RoundPlateGM 2.6           LambertianReceiver(1.)            ends every ray (terminal); POLAR with x and y exchanged
                                                                            (RoundPlateGM's arctan2(x, y)), full azimuth; the map that
                                                                            is made large for the bins-on-global-atomics regime
  1  wall      RectPlateGM 3 x 4          LambertianReceiver(0.4)           diffuse class; the plain XY map: the chart maps behind it
                                                                            sit at offsets in the tally buffer and its LDS copy
  2  cylinder  FiniteCylinder 1.2 / 1.4   Lambertian_IAMDetector(0.5, 0.2)  general class; CYLINDER, full azimuth
  3  sphere    SphericalGM 0.5            ReflectiveReceiver(0.3)           mirror class; SPHERE, full azimuth
  4  dish      ParabolicDishGM 1.6, f 1   LambertianReceiver(0.4)           diffuse class; POLAR out to r = 0.55 of 0.8: clipped
  5  frustum   ConicalFrustum             ReflectiveDetector(0.1)           mirror class; CYLINDER on edges of the caller's (the
                                                                            reference has no get_fluxmap for cones)

Every surface carries a map and captures its hits.  The reference of every check is numpy.histogram2d of those hits, projected on
the host with the same round(inv(frame), 9) and the NumPy formulas of the charts (chart_uv).
"""
import numpy as N

import fluxmap_scene as fs

FLOOR, WALL, CYLINDER, SPHERE, DISH, FRUSTUM = range(6)
CLIPPED = (DISH,)
SEAM = (FLOOR, CYLINDER, SPHERE)          # full-azimuth maps: their first and last phi bins must both be populated
CLASS_OF = {FLOOR: 'terminal', WALL: 'diffuse', CYLINDER: 'general', SPHERE: 'mirror', DISH: 'diffuse', FRUSTUM: 'mirror'}
EDGE_EPS = 1e-12                          # no hit may lie within this share of a map's span from one of its edges

# Bins of the floor's map per storage regime of the streaming engine (trc_stream_form_shade, trc_stream.inc: a shading kernel keeps the
# bins in LDS while they and its tables fit 78 KiB (k_s_shade) / 150 KiB (the lean kernels)).  The other five maps hold
# 14 * 19 + 7 * 12 + 6 * 12 + 5 * 8 + 6 * 9 = 516 bins.
#   lds      13 x 16:   (208 + 516) * 8   =   5 792 bytes: every kernel keeps the bins in LDS
#   global  200 x 100:  (20000 + 516) * 8 = 164 128 bytes > 150 KiB: every kernel adds to the bins in global memory
FLOOR_BINS = {'lds': (13, 16), 'global': (200, 100)}
OTHER_BINS = 14 * 19 + 7 * 12 + 6 * 12 + 5 * 8 + 6 * 9
CHARTS = ('xy', 'cylinder', 'polar', 'sphere')


def maps(regime):
    """{surface: (chart, swap_xy, u edges, v edges)}"""
    nu, nv = FLOOR_BINS[regime]
    two_pi = 2. * N.pi
    return {FLOOR: ('polar', True, fs.nonuniform(0., 2.6, nu), N.linspace(0., two_pi, nv + 1)),
            WALL: ('xy', False, N.linspace(-1.5, 1.5, 15), N.linspace(-2., 2., 20)),
            CYLINDER: ('cylinder', False, N.linspace(-0.7, 0.7, 8), N.linspace(0., two_pi, 13)),
            SPHERE: ('sphere', False, N.linspace(0., N.pi, 7), N.linspace(0., two_pi, 13)),
            DISH: ('polar', False, N.linspace(0., 0.55, 6), fs.nonuniform(0., two_pi, 8)),
            FRUSTUM: ('cylinder', False, N.linspace(0., 0.6, 7), N.linspace(0., two_pi, 10))}


def receivers():
    """(assembly, objects, T)"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM, RoundPlateGM
    from tracer_amd.cylinder import FiniteCylinder
    from tracer_amd.sphere_surface import SphericalGM
    from tracer_amd.paraboloid import ParabolicDishGM
    from tracer_amd.cone import ConicalFrustum
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
    T = N.dot(translate(-5.2, 3.7, 4.4), N.dot(rotx(-0.5), N.dot(roty(0.7), rotz(-0.9))))
    half = N.pi / 2.
    parts = [(RoundPlateGM(2.6), opt.LambertianReceiver(1.), N.eye(4)),
             (RectPlateGM(3., 4.), opt.LambertianReceiver(0.4), N.dot(translate(-2., 0., 1.5), roty(half))),
             (FiniteCylinder(1.2, 1.4), opt.Lambertian_IAMDetector(0.5, 0.2), N.dot(translate(-0.6, 0.5, 1.1), rotz(0.4))),
             (SphericalGM(0.5), opt.ReflectiveReceiver(0.3), N.dot(translate(1.0, -0.9, 0.8), rotx(0.3))),
             (ParabolicDishGM(1.6, 1.), opt.LambertianReceiver(0.4), N.dot(translate(0.9, 1.1, 0.2), roty(0.2))),
             (ConicalFrustum(0., 0.5, 0.6, 0.9), opt.ReflectiveDetector(0.1), N.dot(translate(-0.8, -1.3, 0.1), rotz(-0.7)))]
    objs = [AssembledObject(surfs=[Surface(gm, o)], transform=N.dot(T, tr)) for gm, o, tr in parts]
    return Assembly(objects=objs), objs, T


def source(n, T, seed, ray_offset=0, spectrum=None):
    """the disc source of fluxmap_scene.py over this assembly"""
    return fs.source(n, T, seed, ray_offset=ray_offset, spectrum=spectrum)


def projection(frame, swap_xy=False):
    """rows of the global -> local matrix as the library takes them: round(inv(frame), 9), rows 0 and 1 exchanged for swap_xy"""
    p = fs.projection(frame)
    return p[[1, 0, 2, 3]] if swap_xy else p


def chart_uv(chart, proj, points):
    """(u, v) of global points (3, n) in `chart`: the formulas of the reference's get_fluxmap bodies in NumPy, products and sums in
    the order the kernels take them (no fused multiply-add there either)"""
    x, y, z = N.asarray(points, dtype=float)
    xl = ((proj[0, 0] * x + proj[0, 1] * y) + proj[0, 2] * z) + proj[0, 3]
    yl = ((proj[1, 0] * x + proj[1, 1] * y) + proj[1, 2] * z) + proj[1, 3]
    if chart == 'xy':
        return xl, yl
    zl = ((proj[2, 0] * x + proj[2, 1] * y) + proj[2, 2] * z) + proj[2, 3]
    phi = N.arctan2(yl, xl)
    phi[phi < 0.] += 2. * N.pi
    if chart == 'cylinder':
        return zl, phi
    if chart == 'polar':
        return N.sqrt(xl * xl + yl * yl), phi
    assert chart == 'sphere'
    with N.errstate(invalid='ignore', divide='ignore'):
        return N.arccos(zl / N.sqrt((xl * xl + yl * yl) + zl * zl)), phi


def near_edge(c, edges):
    """coordinates within EDGE_EPS of the map's span from one of its edges"""
    edges, c = N.asarray(edges), N.asarray(c)
    i = N.searchsorted(edges, c)
    lo, hi = edges[N.clip(i - 1, 0, len(edges) - 1)], edges[N.clip(i, 0, len(edges) - 1)]
    return N.minimum(N.abs(c - lo), N.abs(c - hi)) <= EDGE_EPS * (edges[-1] - edges[0])


def host_maps(hits, frames, maps_):
    """{surface: (histogram2d of its hits, energy of its hits outside the map, hits outside, hits, hits near an edge)} from a hit
    list dict(surf, e_abs, points)"""
    out = {}
    for s, (chart, swap, ue, ve) in maps_.items():
        k = N.nonzero(N.asarray(hits['surf']) == s)[0]
        u, v = chart_uv(chart, projection(frames[s], swap), N.asarray(hits['points'])[:, k])
        w = N.asarray(hits['e_abs'])[k]
        H = N.histogram2d(u, v, bins=[ue, ve], weights=w)[0]
        outside = ~((u >= ue[0]) & (u <= ue[-1]) & (v >= ve[0]) & (v <= ve[-1]))
        out[s] = (H, w[outside].sum(), int(outside.sum()), len(k), int((near_edge(u, ue) | near_edge(v, ve)).sum()))
    return out


def check_inputs(ref, maps_, min_filled=0.10):
    """the conditions on the inputs every test states: they are properties of the host histograms alone"""
    for s, (H, e_out, n_out, n_hits, n_near) in ref.items():
        assert n_near == 0, ('INPUT CONDITION, not the map: %d hits of surface %d lie within %g of the span of an edge; their bin '
                             'depends on the last bit of atan2 / acos -- choose another seed' % (n_near, s, EDGE_EPS))
        assert H.sum() > 0., s
        assert (H > 0).mean() >= min_filled, (s, (H > 0).mean())
        if s in CLIPPED:
            assert 0.01 * n_hits <= n_out <= 0.90 * n_hits, (s, n_out, n_hits)
        if s in SEAM:
            assert H[:, 0].sum() > 0. and H[:, -1].sum() > 0., (s, 'seam bins')


# -- hits exactly on edges ------------------------------------------------------------------------------------------------------
# Rays fired straight down on a 64 x 64 plate in the plane z = 0 of an identity frame land at (x, y, 0) exactly.  The map's
# projection is handed over explicitly (DeviceScene.set_fluxmap(proj=...)) so that the plate's plane serves every chart:
#   cylinder   xl = 1, yl = y, zl = x:   u = x itself, phi = atan2(y, 1)
#   polar      xl = x, yl = y:           r from 3-4-5 triples scaled by powers of two, or |x| on the axis (sqrt(x * x) = |x| exactly)
#   sphere     xl = x, yl = 0, zl = y:   theta = 0 at the pole x = 0, y > 0; phi = 0 or pi
# Only points whose bin does not depend on the library's atan2 / acos: u exact, phi = 0 exactly at yl = 0, xl > 0, phi = 2 pi exactly
# after the wrap of a tiny negative angle (-2^-60 + 2 pi rounds to 2 pi), theta = acos(1) = 0; every other angle far inside a bin.
EDGE_PROJ = {'cylinder': N.array([[0., 0., 0., 1.], [0., 1., 0., 0.], [1., 0., 0., 0.], [0., 0., 0., 1.]]),
             'polar': N.eye(4),
             'sphere': N.array([[1., 0., 0., 0.], [0., 0., 0., 0.], [0., 1., 0., 0.], [0., 0., 0., 1.]])}
TWO_PI = 2. * N.pi
EDGE_EDGES = {'cylinder': (N.array([-2., -1., -0.5, 0.5, 1., 4.]), N.array([0., 0.5, 2., 4., TWO_PI])),
              'polar': (N.array([0.5, 1., 2.5, 5., 10.]), N.array([0., 0.5, 2., 4., TWO_PI])),
              'sphere': (N.array([0., 0.5, 1., 2.]), N.array([0., 1., 4., TWO_PI]))}
TINY = -2. ** -60


def edge_cases(chart):
    """(x, y, energy, expected map, energy outside): the bin of every landing point written out by hand from numpy's rule -- edge i
    opens bin i, the last edge closes the last bin, anything else is outside (None) -- and ray k carries 2^-k, so that every sum is
    exact and every ray can be told from the others."""
    up, dn = (lambda a: N.nextafter(a, N.inf)), (lambda a: N.nextafter(a, -N.inf))
    if chart == 'cylinder':
        # u = x on edges -2 -1 -0.5 0.5 1 4; phi = atan2(y, 1): y = 0 -> 0 (bin 0), 1 -> pi/4 (bin 1), -1 -> 7 pi/4 (bin 3),
        # TINY -> 2 pi, the closed last edge (bin 3)
        table = [
            (-1., 0., 1, 0), (dn(-1.), 0., 0, 0), (up(-1.), 0., 1, 0),
            (-0.5, 1., 2, 1), (dn(-0.5), 1., 1, 1), (up(-0.5), 1., 2, 1),
            (0.5, -1., 3, 3), (dn(0.5), -1., 2, 3), (up(0.5), -1., 3, 3),
            (1., TINY, 4, 3), (dn(1.), TINY, 3, 3), (up(1.), TINY, 4, 3),
            (-2., 0., 0, 0), (dn(-2.), 0., None, None), (up(-2.), 0., 0, 0),
            (4., 0., 4, 0), (dn(4.), 0., 4, 0), (up(4.), 0., None, None),
            (-2., TINY, 0, 3), (4., TINY, 4, 3), (up(4.), TINY, None, None), (dn(-2.), TINY, None, None),
            (0.25, 1., 2, 1), (3., -1., 4, 3), (6., 0., None, None), (-7., 1., None, None)]
    elif chart == 'polar':
        # r on edges 0.5 1 2.5 5 10; phi: atan2(4, 3) = 0.927 (bin 1), atan2(4, -3) = 2.214 (bin 2), atan2(-4, -3) + 2 pi = 4.069
        # (bin 3), atan2(-4, 3) + 2 pi = 5.356 (bin 3), on the axis y = 0, x > 0: 0 (bin 0), y = TINY: 2 pi (bin 3; r = x still:
        # x * x + 2^-120 rounds to x * x)
        table = [
            (3., 4., 3, 1), (1.5, 2., 2, 1), (6., 8., 3, 1), (0.75, 1., 1, 1), (0.375, 0.5, 0, 1), (0.1875, 0.25, None, None),
            (-3., 4., 3, 2), (-1.5, -2., 2, 3), (6., -8., 3, 3), (-12., 16., None, None),
            (1., 0., 1, 0), (dn(1.), 0., 0, 0), (up(1.), 0., 1, 0),
            (2.5, 0., 2, 0), (dn(2.5), 0., 1, 0), (up(2.5), 0., 2, 0),
            (5., 0., 3, 0), (dn(5.), 0., 2, 0), (up(5.), 0., 3, 0),
            (0.5, 0., 0, 0), (dn(0.5), 0., None, None), (up(0.5), 0., 0, 0),
            (10., 0., 3, 0), (dn(10.), 0., 3, 0), (up(10.), 0., None, None),
            (1., TINY, 1, 3), (dn(1.), TINY, 0, 3), (10., TINY, 3, 3), (up(10.), TINY, None, None), (0.5, TINY, 0, 3),
            (3., 0., 2, 0), (0.25, 0., None, None), (20., 0., None, None)]
    else:
        assert chart == 'sphere'
        # theta on edges 0 0.5 1 2: the pole (x = 0, y > 0) 0, the first edge (bin 0); (3, 4) acos(0.8) = 0.644 (bin 1); (4, 3)
        # acos(0.6) = 0.927 (bin 1); the equator y = 0: pi/2 (bin 2); (3, -4) acos(-0.8) = 2.498 and the other pole, pi: outside.
        # phi: x > 0 -> 0 (bin 0); x < 0 -> pi (bin 1); on the axis x = 0: atan2(0, 0) = 0 (bin 0)
        table = [
            (0., 2., 0, 0), (0., 0.5, 0, 0), (0., 16., 0, 0),
            (3., 4., 1, 0), (-3., 4., 1, 1), (4., 3., 1, 0), (-1.5, 2., 1, 1),
            (1., 0., 2, 0), (-8., 0., 2, 1),
            (3., -4., None, None), (-6., -8., None, None), (0., -2., None, None)]
    x = N.array([t[0] for t in table])
    y = N.array([t[1] for t in table])
    e = 2. ** -N.arange(1, len(table) + 1)
    ue, ve = EDGE_EDGES[chart]
    want = N.zeros((len(ue) - 1, len(ve) - 1))
    outside = 0.
    for (_, _, iu, iv), ek in zip(table, e):
        if iu is None:
            outside += ek
        else:
            want[iu, iv] += ek
    return x, y, e, want, outside
