"""
The scene, the flux maps and the host reference of the flux-map tests (test_gpu_fluxmap.py on the device, test_fluxmap_host.py for
what can be said about the inputs without one).

The scene is a box cavity open at the top with a cylinder and a tilted mirror inside, turned by a general rotation and moved off
the origin so that no frame is axis aligned:

  0  floor        RectPlateGM 4 x 4      LambertianReceiver(1.)            ends every ray (TRC_SURF_TERMINAL: k_s_absorb)
  1  wall +x      RectPlateGM 3 x 4      ReflectiveReceiver(0.3)           mirror class, absorbs 30 % of every hit
  2  wall -x      RectPlateGM 3 x 4      LambertianReceiver(0.4)           diffuse class
  3  wall +y      RectPlateGM 4 x 3      RefractiveHomogenous(1., 1.5)     general class; absorbs nothing, so no map: what it refracts leaves
  4  wall -y      RectPlateGM 4 x 3      ReflectiveDetector(0.1)           mirror class, full capture
  5  cylinder     FiniteCylinder 1.2/1.4 Lambertian_IAMDetector(0.5, 0.2)  general class and curved: its hits are not coplanar with its map
  6  mirror       RectPlateGM 1.2 x 0.9  RealReflective(0.2, 3e-3)         no map; the surface the update_frames test turns

Surfaces 0, 1, 2, 4 and 5 carry a flux map each and capture their hits (Receiver: lean capture, Detector: everything).  The
reference of every check is numpy.histogram2d of those hits, projected on the host with the same round(inv(frame), 9).
"""
import numpy as N

MAPPED = (0, 1, 2, 4, 5)
CLIPPED = (1, 5)          # maps that cover only a part of what their surface sees
FLOOR = 0
MOVING = 6

# Bins of the floor's map per storage regime of the streaming engine (trc_stream_form_shade / trc_stream_form_absorb in trc_stream.inc); the
# other four maps hold 204 + 266 + 336 + 48 = 854 bins in every regime.  The tables every shading kernel stages besides the bins --
# tallies (3 S + 2) * 8 = 184, surface records S * stride * 8, optics 8 * S * 8 = 448, edges, map descriptors and flags -- come to
# less than 8 KiB for these seven surfaces (records of at most 31 doubles: 1.7 KiB; the edges of the five maps: 4.9 KiB with the
# floor's 300 x 200, 2.8 KiB with 120 x 110).
#   small    31 x 23:   (713 + 854) * 8   =  12 536 bytes: + 8 KiB  < 78 KiB  -> every kernel keeps the bins in LDS, k_s_absorb runs
#   middle  120 x 110:  (13200 + 854) * 8 = 112 432 bytes: > 78 KiB alone, + 8 KiB < 150 KiB -> k_s_shade on global atomics, the lean
#                                                          kernels in LDS, k_s_absorb switched off (fm_ok)
#   large   300 x 200:  (60000 + 854) * 8 = 486 832 bytes: > 150 KiB -> every kernel on global atomics
FLOOR_BINS = {'small': (31, 23), 'middle': (120, 110), 'large': (300, 200)}
OTHER_BINS = 204 + 266 + 336 + 48


def nonuniform(lo, hi, n):
    """n bins on [lo, hi] whose widths vary by a factor of 5.5 (narrow in the middle)"""
    t = N.linspace(-1., 1., n + 1)
    return lo + (hi - lo) * 0.5 * (1. + 0.4 * t + 0.6 * t ** 3)


def map_edges(regime):
    """{surface: (u edges, v edges)}: nu != nv everywhere; the floor's edges are not uniform; the maps of the mirror wall and of the
    cylinder cover only the middle of what is hit"""
    nu, nv = FLOOR_BINS[regime]
    return {0: (nonuniform(-2., 2., nu), nonuniform(-2., 2., nv)),
            1: (N.linspace(-0.8, 0.8, 18), N.linspace(-1.1, 1.1, 13)),          # 17 x 12 of a wall of +-1.5 x +-2
            2: (N.linspace(-1.5, 1.5, 15), N.linspace(-2., 2., 20)),            # 14 x 19
            4: (N.linspace(-2., 2., 22), N.linspace(-1.5, 1.5, 17)),            # 21 x 16
            5: (N.linspace(-0.65, 0.45, 9), N.linspace(-0.65, 0.65, 7))}        # 8 x 6 over the circle of radius 0.6: cut at x = 0.45


def cavity(mirror_turn=0.):
    """(assembly, objects); mirror_turn: the tilted mirror turned further about its own x axis"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.cylinder import FiniteCylinder
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
    T = N.dot(translate(7.3, -4.1, 2.9), N.dot(rotx(0.7), N.dot(roty(-0.4), rotz(1.1))))
    half = N.pi / 2.
    parts = [(RectPlateGM(4., 4.), opt.LambertianReceiver(1.), N.eye(4)),
             (RectPlateGM(3., 4.), opt.ReflectiveReceiver(0.3), N.dot(translate(2., 0., 1.5), roty(half))),
             (RectPlateGM(3., 4.), opt.LambertianReceiver(0.4), N.dot(translate(-2., 0., 1.5), roty(half))),
             (RectPlateGM(4., 3.), opt.RefractiveHomogenous(1., 1.5), N.dot(translate(0., 2., 1.5), rotx(half))),
             (RectPlateGM(4., 3.), opt.ReflectiveDetector(0.1), N.dot(translate(0., -2., 1.5), rotx(half))),
             (FiniteCylinder(1.2, 1.4), opt.Lambertian_IAMDetector(0.5, 0.2), translate(-0.6, 0.5, 1.1)),
             (RectPlateGM(1.2, 0.9), opt.RealReflective(0.2, 3e-3), mirror_pose(mirror_turn))]
    objs = [AssembledObject(surfs=[Surface(gm, o)], transform=N.dot(T, tr)) for gm, o, tr in parts]
    return Assembly(objects=objs), objs, T


def plates(general=False):
    """
    (assembly, T): the cavity's box alone, five surfaces -- an ODD count, two maps of different bin counts (PLATES_EDGES) and a
    non-empty optics table: the scene in which every rounding of the shading kernels' LDS image shows (the surface -> map table of
    five words ends off 8 bytes, and the optics table and the bins lie behind it).

      0  floor     LambertianReceiver(1.)       ends every ray; map of 3 x 4
      1  wall +x   Lambertian_directional_axisymmetric_piecewise: a diffuse wall driven by a table of absorptance over angle
      2  wall -x   ReflectiveReceiver(0.3)      mirror class; map of 5 x 2
      3  wall +y   LambertianSpecular(0.3, 0.5) diffuse class
      4  wall -y   Reflective(0.2), or with `general` Reflective_IAM(0.2, 0.2): the general class, which brings k_s_shade in
    """
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
    T = N.dot(translate(-2.3, 6.1, 1.7), N.dot(rotx(-0.6), N.dot(roty(0.5), rotz(0.8))))
    half = N.pi / 2.
    th = N.linspace(0., half, 7)
    parts = [(RectPlateGM(4., 4.), opt.LambertianReceiver(1.), N.eye(4)),
             (RectPlateGM(3., 4.), opt.Lambertian_directional_axisymmetric_piecewise(th, 0.2 + 0.4 * N.cos(th)), N.dot(translate(2., 0., 1.5), roty(half))),
             (RectPlateGM(3., 4.), opt.ReflectiveReceiver(0.3), N.dot(translate(-2., 0., 1.5), roty(half))),
             (RectPlateGM(4., 3.), opt.LambertianSpecular(0.3, 0.5), N.dot(translate(0., 2., 1.5), rotx(half))),
             (RectPlateGM(4., 3.), opt.Reflective_IAM(0.2, 0.2) if general else opt.Reflective(0.2), N.dot(translate(0., -2., 1.5), rotx(half)))]
    objs = [AssembledObject(surfs=[Surface(gm, o)], transform=N.dot(T, tr)) for gm, o, tr in parts]
    return Assembly(objects=objs), T


PLATES_EDGES = {0: (nonuniform(-2., 2., 3), N.linspace(-2., 2., 5)),          # 3 x 4
                2: (N.linspace(-1.5, 1.5, 6), N.linspace(-2., 2., 3))}        # 5 x 2


def mirror_pose(turn):
    from tracer_amd.spatial_geometry import translate, rotx, roty
    return N.dot(translate(0.9, -0.8, 1.2), N.dot(rotx(0.5 + turn), roty(-0.6)))


def source(n, T, seed, ray_offset=0, spectrum=None):
    """a pillbox disc source above the open top, aimed obliquely into the cavity (cone 0.3 rad: within the footprint map's reach)"""
    from tracer_amd import sources
    d = N.r_[0.32, 0.22, -1.]
    d = d / N.linalg.norm(d)
    c = N.r_[0., 0., 1.2] - 6. * d
    return sources.disk_bundle(n, N.c_[N.dot(T[:3, :3], c) + T[:3, 3]], N.dot(T[:3, :3], d), 1.9, 0.3, flux=1000., seed=seed,
                               ray_offset=ray_offset, spectrum=spectrum)


def projection(frame):
    """rows of the global -> local matrix as DeviceScene.set_fluxmap hands them to the library"""
    return N.round(N.linalg.inv(frame), decimals=9)


def project(proj, points):
    """local u, v of global points (3, n), summed in the order the kernels sum (no fused multiply-add there either)"""
    x, y, z = points
    u = ((proj[0, 0] * x + proj[0, 1] * y) + proj[0, 2] * z) + proj[0, 3]
    v = ((proj[1, 0] * x + proj[1, 1] * y) + proj[1, 2] * z) + proj[1, 3]
    return u, v


def host_maps(hits, frames, edges):
    """{surface: (histogram2d of its hits, energy of its hits outside the map, hits outside, hits)} from a hit list
    dict(surf, e_abs, points)"""
    out = {}
    for s, (ue, ve) in edges.items():
        k = N.nonzero(N.asarray(hits['surf']) == s)[0]
        u, v = project(projection(frames[s]), N.asarray(hits['points'])[:, k])
        w = N.asarray(hits['e_abs'])[k]
        H = N.histogram2d(u, v, bins=[ue, ve], weights=w)[0]
        outside = ~((u >= ue[0]) & (u <= ue[-1]) & (v >= ve[0]) & (v <= ve[-1]))
        out[s] = (H, w[outside].sum(), int(outside.sum()), len(k))
    return out


def hits_of_levels(levels, keep=None):
    """the hit list of a recorded trace (the levels of the ordered engine's tree or of oracle.engine, one ray out per hit): a ray
    of level k + 1 starts where its parent of level k landed, on `surf`, and what the parent lost there was absorbed.  Levels
    that carry directions (oracle.engine's) give the incident energy and direction of every hit as well: what a full capture holds.
    keep: level -> mask of its rays that stand for a hit (default: all of them)."""
    surf, e_abs, pts, e_in, dirs = [], [], [], [], []
    with_dirs = all('directions' in L for L in levels[:-1])       # (the ordered engine's level 0 is given as energies alone: no directions then)
    for prev, L in zip(levels[:-1], levels[1:]):
        m = N.ones(len(L['parents']), dtype=bool) if keep is None else keep(L)
        par = N.asarray(L['parents'])[m]
        assert len(N.unique(par)) == len(par)           # (no optics of this scene sends two rays on)
        surf.append(N.asarray(L['surf'])[m])
        e_in.append(N.asarray(prev['energy'])[par])
        e_abs.append(e_in[-1] - N.asarray(L['energy'])[m])
        pts.append(N.asarray(L['vertices'])[:, m])
        if with_dirs:
            dirs.append(N.asarray(prev['directions'])[:, par])
    out = dict(surf=N.concatenate(surf), e_abs=N.concatenate(e_abs), points=N.hstack(pts), e_in=N.concatenate(e_in))
    if with_dirs:
        out['directions'] = N.hstack(dirs)
    return out


def check_inputs(ref, edges, min_filled=0.10):
    """the conditions on the inputs every test states: they are properties of the host histograms alone"""
    for s, (H, e_out, n_out, n_hits) in ref.items():
        assert H.sum() > 0., s
        assert (H > 0).mean() >= min_filled, (s, (H > 0).mean())
        if s in CLIPPED:
            assert 0.01 * n_hits <= n_out <= 0.90 * n_hits, (s, n_out, n_hits)


# -- hits exactly on edges ------------------------------------------------------------------------------------------------------
EDGE_U = N.array([-2., -1., -0.5, 0.5, 1., 4.])         # 5 bins; every edge a power of two, so is every landing point's projection
EDGE_V = N.array([-4., -2., 1., 2.])                    # 3 bins


def edge_cases():
    """(x, y, energy, expected map, energy outside): rays fired straight down on a 16 x 16 plate in the plane z = 0 of an identity
    frame land at (x, y) exactly, and the projection returns x and y themselves.  The bin of every landing point is written out
    here by hand from numpy's rule -- edge i opens bin i, the last edge closes the last bin, anything else is outside (None) --
    and ray k carries 2^-k, so that every sum is exact and every ray can be told from the others."""
    up, dn = (lambda a: N.nextafter(a, N.inf)), (lambda a: N.nextafter(a, -N.inf))
    table = [
        # interior edges, and one ulp either side of them
        (-1., 0., 1, 1), (dn(-1.), 0., 0, 1), (up(-1.), 0., 1, 1),
        (-0.5, 0., 2, 1), (dn(-0.5), 0., 1, 1), (up(-0.5), 0., 2, 1),
        (0.5, 0., 3, 1), (dn(0.5), 0., 2, 1), (up(0.5), 0., 3, 1),
        (1., 0., 4, 1), (dn(1.), 0., 3, 1), (up(1.), 0., 4, 1),
        (0., -2., 2, 1), (0., dn(-2.), 2, 0), (0., up(-2.), 2, 1),
        (0., 1., 2, 2), (0., dn(1.), 2, 1), (0., up(1.), 2, 2),
        # first and last edges: the first opens bin 0, the last closes the last bin; one ulp beyond is outside
        (-2., 0., 0, 1), (dn(-2.), 0., None, None), (up(-2.), 0., 0, 1),
        (4., 0., 4, 1), (dn(4.), 0., 4, 1), (up(4.), 0., None, None),
        (0., -4., 2, 0), (0., dn(-4.), None, None), (0., up(-4.), 2, 0),
        (0., 2., 2, 2), (0., dn(2.), 2, 2), (0., up(2.), None, None),
        # corners of bins: inner ones, the four corners of the map, and corners missed by one ulp in one coordinate
        (-1., -2., 1, 1), (0.5, 1., 3, 2), (1., -2., 4, 1), (-0.5, 1., 2, 2),
        (-2., -4., 0, 0), (4., 2., 4, 2), (-2., 2., 0, 2), (4., -4., 4, 0),
        (up(4.), 2., None, None), (4., up(2.), None, None), (dn(-2.), -4., None, None), (-2., dn(-4.), None, None),
        (dn(4.), dn(2.), 4, 2), (up(-2.), up(-4.), 0, 0), (dn(0.5), dn(1.), 2, 1),
        # well inside and well outside
        (0.25, -3., 2, 0), (3., 1.5, 4, 2), (6., 0., None, None), (0., -7., None, None)]
    x = N.array([t[0] for t in table])
    y = N.array([t[1] for t in table])
    e = 2. ** -N.arange(1, len(table) + 1)
    want = N.zeros((len(EDGE_U) - 1, len(EDGE_V) - 1))
    outside = 0.
    for (_, _, iu, iv), ek in zip(table, e):
        if iu is None:
            outside += ek
        else:
            want[iu, iv] += ek
    return x, y, e, want, outside
