"""
Scenes and calls that trace every geometry kind of the per-ray core through every engine, and their host reference
(test_geometry_cases_host.py for what can be said without a device, test_gpu_geometry_kinds.py on one).

The core knows 30 kinds (oracle/kinds.py, trc_gm_nparams in csrc/trc_core.h).  test_gpu_parity.py holds each of them to the
fixtures one surface at a time, through k_gm_intersect / k_gm_normals.  Inside an engine a kind also has to be right in its box
(trc_surface_local_box), in the single-precision searches built from that box, in a record whose stride the widest kind of the scene
sets, in tables staged to LDS, in the FLAT instances that take the normal from the frame, and in the lean shading kernels that take
the normal of a curved surface.  The scenes here put every kind there:

  gallery        every bounded maker of MAKERS twice, general rotations, centres uniform in +-4
  gallery-full   the gallery over a plane of filler plates: records, boxes and shading tables beyond LDS
  flats          the ten bounded flat makers three times, packed in +-2, above a floor and in front of a wall: all_flat
  open           every maker once, the seven unbounded kinds included, inside an absorbing sphere of radius 25
  alone/<kind>   the kind twice inside the same sphere: the kind is the widest of its scene, so the stride is its own

Two situations are ill-conditioned in the reference itself and the scenes avoid them: a ray that leaves a hexagonal dish (its root
rule `t > 0` accepts or rejects the self-intersection root by its last bit), so every hex dish ends every ray; and a ray that leaves
an unbounded quadric far from the origin (the self-intersection root then sits next to the `t >= 1e-6` threshold), so the unbounded
kinds stand inside the sphere, which ends every ray within 25 of the origin.

Optics: Reflective(0.3), Lambertian(0.5), RealReflective(0.2, 2e-3) in turn over the surfaces -- the mirror and the diffuse lean
class on every family of normals.  Every scene has one flux map on a surface that ends every ray (lean capture) and one surface
captured in full (ReflectiveDetector).  A call names the kernel instances it is there for as the library names them
(search_cases.library_decide); every call over one scene and one set of rays shares one oracle trace.
"""
import collections
import functools

import numpy as N

import fluxmap_scene as fs
import mega_cases as M
import search_cases as S
import shade_cases as sc

N_RAYS, REPS, SEED, E_MIN_SHARE = sc.N_RAYS, sc.REPS, sc.SEED, sc.E_MIN_SHARE
ALONE_RAYS, ALONE_REPS = 1024 + 37, 4
REC_HDR = sc.REC_HDR

# trc_gm_nparams (csrc/trc_core.h) restated for all 30 kinds, by _cabi.GM_* name; test_geometry_cases_host.py compares it with the library
NPARAMS = {
    'GM_FLAT_INF': 0, 'GM_RECT': 2, 'GM_RECT_EXTRUDED': 6, 'GM_RECT_PERFORATED': 2, 'GM_ROUND': 2, 'GM_ROUND_CUT': 3, 'GM_TRIANGLE': 6,
    'GM_PARABOLOID': 2, 'GM_PARAB_DISH': 3, 'GM_PARAB_HEX': 3, 'GM_PARAB_RECT': 4, 'GM_PARAB_RECT_OFFAXIS': 16, 'GM_PARAB_CYL': 1,
    'GM_PARAB_TROUGH': 3, 'GM_SPHERE': 1, 'GM_HEMISPHERE': 1, 'GM_SPHERE_RECT': 3, 'GM_CYL_INF': 1, 'GM_CYL_FINITE': 4, 'GM_CYL_RECTCUT': 4,
    'GM_CONE_INF': 2, 'GM_CONE_FINITE': 3, 'GM_FRUSTUM': 4, 'GM_FRUSTUM_RECTCUT': 6, 'GM_QUADRATIC': 6, 'GM_QUADRATIC_RECT': 8,
    'GM_ELLIPSOID': 3, 'GM_ELLIPSOID_CUT': 9, 'GM_SPHERE_CUT': 15, 'GM_POLYGON': 6,
}
# the kinds trc_surface_local_box (csrc/trc_bounds.h) gives no box: they go on the `unbounded` list of every search
UNBOUNDED = ('GM_FLAT_INF', 'GM_PARABOLOID', 'GM_PARAB_RECT_OFFAXIS', 'GM_PARAB_CYL', 'GM_CYL_INF', 'GM_CONE_INF', 'GM_QUADRATIC')
FLAT_KINDS = sc.FLAT_KINDS
HEX = 'GM_PARAB_HEX'
ENCLOSURE = 25.                 # radius of the absorbing sphere around `open` and `alone/<kind>`


def _rot(axis, angle):
    from tracer_amd.spatial_geometry import general_axis_rotation
    return general_axis_rotation(N.asarray(axis, dtype=float) / N.linalg.norm(axis), angle)


_L = N.array([[-1., -1., 0.2, 0.2, 0.6, 1.2, 1.2], [-0.8, 1., 1., 0.1, 0.3, 0.1, -0.8]])
_PENTAGON = N.array([[N.cos(-2. * N.pi * k / 5. + 0.3) for k in range(5)], [0.8 * N.sin(-2. * N.pi * k / 5. + 0.3) for k in range(5)]])
_OFF_AXIS = N.array([N.sin(0.2) * N.cos(0.4), N.sin(0.2) * N.sin(0.4), N.cos(0.2)])


def _cut(kind):
    """the bounding volume of a CutSphereGM maker, built when the maker is called"""
    from tracer_amd import boundary_shape as bs
    if kind == 'plane':
        return bs.BoundaryPlane(location=N.r_[0.1, 0., 0.4], rotation=_rot([1., 0.3, 0.], 0.5))
    if kind == 'cap':
        return bs.BoundaryPlane(location=N.r_[0., 0., 1.2])
    return bs.BoundarySphere(radius=4., location=N.r_[0., 0., -4 * N.sqrt(3) / 2.])


# name: (kind, module, class, arguments, keyword arguments, reach).  The arguments are those of the geometry fixtures
# (tests/golden/make_golden.py: gm_cases); reach: no point of the surface is farther from the frame's origin (bounded kinds)
MAKERS = collections.OrderedDict([
    ('flat', ('GM_FLAT_INF', 'flat_surface', 'FlatGeometryManager', (), {}, None)),
    ('rect', ('GM_RECT', 'flat_surface', 'RectPlateGM', (1.5, 0.8), {}, 0.9)),
    ('rect_extruded', ('GM_RECT_EXTRUDED', 'flat_surface', 'ExtrudedRectPlateGM', (2., 1.6, N.c_[[0.2, -0.1]], 0.5, 0.4), {}, 1.3)),
    ('rect_perforated', ('GM_RECT_PERFORATED', 'flat_surface', 'PerforatedRectPlateGM',
                         (2., 2., N.array([[0.3, 0.3], [-0.4, 0.1], [0., -0.5]]), N.array([0.2, 0.15, 0.25])), {}, 1.45)),
    ('round', ('GM_ROUND', 'flat_surface', 'RoundPlateGM', (1.,), {}, 1.05)),
    ('annulus', ('GM_ROUND', 'flat_surface', 'RoundPlateGM', (1., 0.4), {}, 1.05)),
    ('round_cut', ('GM_ROUND_CUT', 'flat_surface', 'StraightCutRoundPlateGM', (1., 0.3), {}, 1.05)),
    ('triangle', ('GM_TRIANGLE', 'triangular_face', 'TriangularFace', (N.array([[1.2, 0.], [0.1, 0.9], [0., 0.]]),), {}, 1.25)),
    ('paraboloid', ('GM_PARABOLOID', 'paraboloid', 'Paraboloid', (1.3, 0.9), {}, None)),
    ('parab_dish', ('GM_PARAB_DISH', 'paraboloid', 'ParabolicDishGM', (2., 1.5), {}, 1.05)),
    ('parab_hex', ('GM_PARAB_HEX', 'paraboloid', 'HexagonalParabolicDishGM', (2., 1.5), {}, 1.5)),
    ('parab_rect', ('GM_PARAB_RECT', 'paraboloid', 'RectangularParabolicDishGM', (1.6, 1.2, 2.), {}, 1.05)),
    ('parab_rect_offaxis', ('GM_PARAB_RECT_OFFAXIS', 'paraboloid', 'RectangularParabolicDishGM', (1.0, 0.8, 3.), {'off_axis_normal': _OFF_AXIS}, None)),
    ('parab_cyl', ('GM_PARAB_CYL', 'paraboloid', 'ParabolicCylinder', (1.2,), {}, None)),
    ('parab_trough', ('GM_PARAB_TROUGH', 'paraboloid', 'ParabolicTroughGM', (2., 1., 3.), {}, 1.9)),
    ('sphere', ('GM_SPHERE', 'sphere_surface', 'SphericalGM', (1.1,), {}, 1.15)),
    ('hemisphere', ('GM_HEMISPHERE', 'sphere_surface', 'HemisphereGM', (1.1,), {}, 1.15)),
    ('sphere_rect', ('GM_SPHERE_RECT', 'sphere_surface', 'SphericalRectFacet', (2., 1.2, 0.9), {}, 2.05)),
    ('cyl_inf', ('GM_CYL_INF', 'cylinder', 'InfiniteCylinder', (1.4,), {}, None)),
    ('cyl_finite', ('GM_CYL_FINITE', 'cylinder', 'FiniteCylinder', (1.4, 2.), {}, 1.25)),
    ('cyl_finite_arc', ('GM_CYL_FINITE', 'cylinder', 'FiniteCylinder', (1.4, 2.), {'ang_range': [0.5, 4.0]}, 1.25)),
    ('cyl_rectcut', ('GM_CYL_RECTCUT', 'cylinder', 'RectCutCylinder', (1.4, 2., 1.2, 1.1), {}, 1.25)),
    ('cone_inf', ('GM_CONE_INF', 'cone', 'InfiniteCone', (0.7,), {'a': 0.3}, None)),
    ('cone_finite', ('GM_CONE_FINITE', 'cone', 'FiniteCone', (0.8, 1.5), {}, 1.75)),
    ('frustum', ('GM_FRUSTUM', 'cone', 'ConicalFrustum', (0.2, 0.5, 1.4, 1.1), {}, 1.85)),
    ('frustum_rectcut', ('GM_FRUSTUM_RECTCUT', 'cone', 'RectCutConicalFrustum', (0.2, 0.5, 1.4, 1.1, 1.2, 1.3), {}, 1.85)),
    ('quadratic', ('GM_QUADRATIC', 'quadratic_surface', 'FlatQuadricSurfaceGM', (0.05, 0.08, 0.01, 0.02, -0.03, 0.1), {}, None)),
    ('quadratic_rect', ('GM_QUADRATIC_RECT', 'quadratic_surface', 'RectFlatQuadricSurfaceGM', (2., 1.5, 0.05, 0.08, 0.01, 0.02, -0.03, 0.1), {}, 1.35)),
    ('ellipsoid', ('GM_ELLIPSOID', 'ellipsoid', 'Ellipsoid', (1.2, 0.8, 1.5), {}, 1.55)),
    ('ellipsoid_cut', ('GM_ELLIPSOID_CUT', 'ellipsoid', 'EllipsoidGM', (1.2, 0.8, 1.5), {'xlim': [-0.5, 1.0], 'ylim': None, 'zlim': [-1., 0.7]}, 1.55)),
    ('ellipsoid_alllims', ('GM_ELLIPSOID_CUT', 'ellipsoid', 'EllipsoidGM', (1.2, 0.8, 1.5),
                           {'xlim': [-0.5, 1.0], 'ylim': [-0.3, 0.3], 'zlim': [-1., 0.7]}, 1.55)),
    ('polygon_L', ('GM_POLYGON', 'polygon', 'FlatSimplePolygonGM', (_L,), {}, 1.5)),
    ('polygon_pentagon', ('GM_POLYGON', 'polygon', 'FlatSimplePolygonGM', (_PENTAGON,), {}, 1.05)),
    ('polygon_perforated', ('GM_POLYGON', 'polygon', 'PerforatedPolygonGM',
                            (_L, N.array([[-0.5, 0.4], [0.7, -0.4], [-0.3, -0.5]]), N.array([0.3, 0.2, 0.15])), {}, 1.5)),
    ('sphere_cut_plane', ('GM_SPHERE_CUT', 'sphere_surface', 'CutSphereGM', (1.3,), {'bounding_volume': lambda: _cut('plane')}, 1.35)),
    ('sphere_cut_plane_lens_cap', ('GM_SPHERE_CUT', 'sphere_surface', 'CutSphereGM', (2.,), {'bounding_volume': lambda: _cut('cap')}, 2.05)),
    ('sphere_cut_sphere', ('GM_SPHERE_CUT', 'sphere_surface', 'CutSphereGM', (2.,), {'bounding_volume': lambda: _cut('sphere')}, 2.05)),
])
BOUNDED = [m for m, v in MAKERS.items() if v[5] is not None]
FLATS = [m for m in BOUNDED if MAKERS[m][0] in FLAT_KINDS]
# the maker that stands for a kind where it is alone: the first of MAKERS with that kind
FIRST_OF_KIND = collections.OrderedDict()
for _m, _v in MAKERS.items():
    FIRST_OF_KIND.setdefault(_v[0], _m)
assert sorted(FIRST_OF_KIND) == sorted(NPARAMS) and len(BOUNDED) == 30 and len(FLATS) == 10


def make(maker):
    """the geometry manager of a maker"""
    import importlib
    kind, mod, cls, args, kw, reach = MAKERS[maker]
    kw = dict((k, v() if callable(v) else v) for k, v in kw.items())
    return getattr(importlib.import_module('tracer_amd.' + mod), cls)(*args, **kw)


def optics_of(i, maker, full=False):
    """the optics of the i-th surface of a scene: the cycle; a hex dish ends every ray; full: the surface captured in full, a mirror (of
    two hex dishes alone: one of them)"""
    from tracer_amd import optics_callables as opt
    if MAKERS[maker][0] == HEX:
        return opt.LambertianDetector(1.) if full else opt.LambertianReceiver(1.)
    if full:
        return opt.ReflectiveDetector(0.3)
    return (opt.Reflective(0.3), opt.Lambertian(0.5), opt.RealReflective(0.2, 2e-3))[i % 3]


# -- the scenes -------------------------------------------------------------------------------------------------------------------
# name: (makers in table order, half width of the cube their centres are drawn in, seed of the poses, the maker whose first surface is
# captured in full, extras: 'sphere' | 'floor+wall' | 'fillers').  A scene that fails a condition of test_geometry_cases_host.py gets
# another seed here
POSE_SEED = 7
SCENES = collections.OrderedDict([
    ('gallery', (BOUNDED * 2, 4., POSE_SEED, 'sphere_cut_plane_lens_cap', None)),
    ('gallery-full', (BOUNDED * 2, 4., POSE_SEED, 'sphere_cut_plane_lens_cap', 'fillers')),
    ('flats', (FLATS * 3, 2., POSE_SEED, 'rect_perforated', 'floor+wall')),
    ('open', (list(MAKERS), 4., POSE_SEED, 'sphere_cut_plane_lens_cap', 'sphere')),
])
for _k, _m in FIRST_OF_KIND.items():
    SCENES['alone/' + _k[3:]] = ([_m, _m], 0.9, POSE_SEED, _m, 'sphere')
ALONE = [n for n in SCENES if n.startswith('alone/')]
FILL_Z, FILL_PITCH = -7.5, 0.62          # the fillers' plane, under where the given rays start; their pitch
FLOOR_Z, WALL_X = -2.9, -3.1             # flats: the floor and the wall behind the plates


def fill_count(own, stride):
    """the fewest fillers that put the records alone beyond 40 KiB, the tables of k_s_bounce (records, oriented boxes, boxes, flags)
    and of k_s_fresh beyond 150 KiB, and the lean shading kernels' tables beyond 120 KiB -- from the restated sums, each without the
    parts that only add (search_cases.fill_for)"""
    n = own
    while not (n * stride * 8 > S.LIMIT_RECS and
               S.lds_need(S.fresh_lds_parts(n, stride, S.FP_CELLS // 4, 0, 0, True, 0)) > S.LIMIT_LDS and
               S.lds_need(S.bounce_lds_parts(n, stride, 0, True, False, 0, 0, 0, 0)) > S.LIMIT_LDS and
               (3 * n + 2) * 8 + n * stride * 8 + 8 * n * 8 + 2 * n * 4 > sc.LIMIT_LEAN):
        n += 1
    return n - own


class Scene(object):
    """a scene built: compiled table, frames, makers and kinds per surface, the mapped surface (it ends every ray), the surface
    captured in full; the attributes test_gpu_shade_instances._check reads of a case come from here through Call"""
    W, spec = 0, False

    def __init__(self, name):
        from tracer_amd.scene import compile_scene
        from tracer_amd.flat_surface import RectPlateGM
        from tracer_amd.sphere_surface import SphericalGM
        from tracer_amd import optics_callables as opt
        from tracer_amd.spatial_geometry import generate_transform, translate, rotx, roty, rotz
        self.name = name
        makers, spread, seed, full, extras = SCENES[name]
        self.alone = name.startswith('alone/')
        self.n_rays, self.reps = (ALONE_RAYS, ALONE_REPS) if self.alone else (N_RAYS, REPS)
        rng = N.random.RandomState(seed)
        self.makers = list(makers)
        self.reach = [MAKERS[m][5] for m in makers]
        full_at = makers.index(full)
        parts = []
        for i, m in enumerate(makers):
            axis = rng.normal(size=3)
            loc = rng.uniform(-spread, spread, 3)
            if self.alone:          # the two copies side by side
                loc = N.r_[(-1.2, 1.2)[i], 0., 0.] + 0.3 * loc
            tr = generate_transform(axis / N.linalg.norm(axis), rng.uniform(0.4, 2. * N.pi - 0.4), loc[:, None])
            parts.append((make(m), optics_of(i, m, full=(i == full_at)), tr))
        self.full_surf = full_at
        turn = N.dot(rotx(-0.5), N.dot(roty(0.8), rotz(-0.9)))
        self.n_fill = 0
        if extras == 'sphere':
            parts.append((SphericalGM(ENCLOSURE), opt.LambertianReceiver(1.), N.dot(translate(0.3, -0.2, 0.4), turn)))
            self.makers.append('enclosure'); self.reach.append(ENCLOSURE + 0.01)
            self.map_surf = len(parts) - 1
            self.edges = {self.map_surf: (fs.nonuniform(-21., 23., 13), N.linspace(-24., 19., 10))}
        elif extras == 'floor+wall':
            # a floor and a wall of big plates, tilted a little, and the mapped plate that ends every ray among the others
            parts.append((RectPlateGM(11., 11.), opt.Lambertian(0.5), N.dot(translate(0., 0., FLOOR_Z), N.dot(rotx(0.07), roty(-0.05)))))
            parts.append((RectPlateGM(11., 8.), opt.Reflective(0.3), N.dot(translate(WALL_X, 0., 0.5), N.dot(roty(N.pi / 2. - 0.06), rotz(0.04)))))
            parts.append((RectPlateGM(2.4, 2.4), opt.LambertianReceiver(1.), N.dot(translate(1.1, -0.6, -1.4), N.dot(rotx(0.3), roty(-0.25)))))
            self.makers += ['floor', 'wall', 'receiver']; self.reach += [7.8, 6.9, 1.7]
            self.map_surf = len(parts) - 1
            self.edges = {self.map_surf: (fs.nonuniform(-0.9, 1.2, 13), N.linspace(-1.2, 0.8, 10))}
        else:
            self.map_surf = makers.index('parab_hex')
            self.edges = {self.map_surf: (fs.nonuniform(-0.8, 0.9, 13), N.linspace(-0.9, 0.7, 10))}
        if extras == 'fillers':
            own = len(parts)
            stride = (REC_HDR + max(NPARAMS[MAKERS[m][0]] for m in makers)) | 1
            self.n_fill = fill_count(own, stride)
            side = int(N.ceil(N.sqrt(self.n_fill)))
            fill = []
            for k in range(self.n_fill):        # in front of the gallery in the table: its surfaces sit at offsets of hundreds of records
                x, y = (k % side - (side - 1) / 2.) * FILL_PITCH, (k // side - (side - 1) / 2.) * FILL_PITCH
                tr = N.dot(translate(x, y, FILL_Z), N.dot(rotx(0.09 + 0.05 * N.cos(1.3 * k)), N.dot(roty(0.07 + 0.05 * N.sin(0.7 * k)), rotz(0.3))))
                fill.append((RectPlateGM(0.9 * FILL_PITCH, 0.9 * FILL_PITCH), opt.Reflective(0.2) if k % 2 else opt.Lambertian(0.5), tr))
            parts = fill + parts
            self.makers = ['filler'] * self.n_fill + self.makers
            self.reach = [0.65 * FILL_PITCH] * self.n_fill + self.reach
            self.map_surf += self.n_fill
            self.full_surf += self.n_fill
            self.edges = dict((k + self.n_fill, v) for k, v in self.edges.items())
        self._parts = parts
        self.cs = compile_scene(self._assembly())
        n = self.cs.n_surf
        assert n == len(parts) == len(self.makers)
        gm = sc._names('GM_')
        self.kinds = [gm[self.cs.descs[i].gm_kind] for i in range(n)]
        for i, m in enumerate(self.makers):
            assert m not in MAKERS or self.kinds[i] == MAKERS[m][0], (m, self.kinds[i])
        self.frames = [N.array(s._temp_frame) for s in self.cs.surfaces]
        self.captured = [i for i in range(n) if self.cs.capture[i]]
        self.terminal = [i for i in range(n) if sc.ends_every_ray(self.cs.descs[i])]
        assert self.map_surf in self.terminal and self.map_surf in self.captured
        assert self.full_surf in self.captured and self.full_surf != self.map_surf
        self.stride = (REC_HDR + max(NPARAMS[k] for k in self.kinds)) | 1
        self.flat = all(k in FLAT_KINDS for k in self.kinds)
        self.unbounded = [i for i in range(n) if self.kinds[i] in UNBOUNDED]

    def _assembly(self, boxes=False):
        """the assembly; boxes: every bounded object brings a cube around its surface, for a Kd-tree built over them"""
        from tracer_amd.assembly import Assembly
        from tracer_amd.object import AssembledObject
        from tracer_amd.surface import Surface
        from tracer_amd.boundary_shape import BoundaryBox
        objs = []
        for (gm, o, tr), r in zip(self._parts, self.reach):
            obj = AssembledObject(surfs=[Surface(gm, o)], transform=tr)
            if boxes and r is not None:
                obj.add_boundary(BoundaryBox([[-r, -r, -r], [r, r, r]]))
            objs.append(obj)
        return Assembly(objects=objs)

    # -- the rays ---------------------------------------------------------------------------------------------------------------
    def source(self, src):
        """the pending bundle of a disc source 25 up the line (0.3, -0.2, -1) from the origin, radius 9: a pillbox of 20 mrad ('disk') or a
        Buie sunshape of CSR 0.05 ('buie')"""
        from tracer_amd import sources
        d = N.r_[0.3, -0.2, -1.]
        d = d / N.linalg.norm(d)
        centre = N.c_[-25. * d]
        if src == 'disk':
            return sources.disk_bundle(self.n_rays, centre, d, 9., 0.02, flux=1000., seed=SEED)
        assert src == 'buie'
        return sources.buie_sunshape(self.n_rays, centre, d, 9., 0.05, flux=1000., seed=SEED)

    def desc(self, src):
        return self.source(src)._src_desc

    def min_energy(self, src):
        return E_MIN_SHARE * (1. if src == 'given' else self.desc(src).energy)

    @functools.lru_cache(maxsize=None)
    def rays(self, src):
        """(vertices, directions, energy, ray ids): 'given': seeded rays of energy 1 that start uniform in +-6 with isotropic directions
        (alone/<kind>: aimed at points uniform in +-1.8 around the two copies, so that a thousand rays hit them); otherwise the
        source's rays, made by the oracle"""
        if src != 'given':
            from oracle import engine, sources
            return sources.generate(engine.source_from_desc(self.desc(src)), self.n_rays, SEED, 0)
        n = self.n_rays
        rng = N.random.RandomState(SEED + 11)
        v = rng.uniform(-6., 6., (3, n))
        d = rng.normal(size=(3, n))
        if self.alone:
            d = rng.uniform(-1.8, 1.8, (3, n)) - v
        d /= N.sqrt((d ** 2).sum(axis=0))
        return N.ascontiguousarray(v), N.ascontiguousarray(d), N.ones(n), N.arange(n, dtype=N.uint64)

    # -- the trees ----------------------------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def kdtree(self):
        """the reference's build over the cubes of the bounded objects; the unbounded ones are always relevant"""
        from tracer_amd.accel_tree import KdTree
        return KdTree(self._assembly(boxes=True), 8 + 1.3 * N.log(self.cs.n_surf), min_leaf=1)

    @functools.lru_cache(maxsize=None)
    def deep_tree(self, D):
        """a valid tree of depth D (mega_cases.nested): D planes across the box of the bounded surfaces, on the three axes in turn, every
        leaf listing every bounded surface, the unbounded ones always relevant"""
        bounded = [i for i in range(self.cs.n_surf) if i not in self.unbounded]
        c = N.array([self.frames[i][:3, 3] for i in bounded])
        r = N.sqrt(3.) * N.array([self.reach[i] for i in bounded])[:, None]
        lo, hi = (c - r).min(axis=0), (c + r).max(axis=0)
        n = 2 * D + 1
        flag, child, sp = N.full(n, 3, dtype=N.int32), N.zeros(n, dtype=N.int32), N.zeros(n)
        leaf_off, leaf_cnt = N.zeros(n, dtype=N.int32), N.zeros(n, dtype=N.int32)
        for k in range(D):
            a = k % 3
            flag[2 * k], child[2 * k] = a, 2 * k + 1
            sp[2 * k] = lo[a] + (hi[a] - lo[a]) * (k // 3 + 1.) / (D // 3 + 2.)
        leaves = [i for i in range(n) if flag[i] == 3]
        for j, node in enumerate(leaves):
            leaf_off[node], leaf_cnt[node] = j * len(bounded), len(bounded)
        return M.HandTree(dict(flag=flag, split=sp, child=child, leaf_off=leaf_off, leaf_cnt=leaf_cnt,
                               leaf_surfs=N.tile(N.array(bounded, dtype=N.int32), len(leaves)),
                               always_relevant=N.array(self.unbounded, dtype=N.int32), bounds=N.r_[lo, hi]))

    def tree(self, kd):
        """None, 'built' or ('deep', D)"""
        return None if kd is None else self.kdtree() if kd == 'built' else self.deep_tree(kd[1])

    @functools.lru_cache(maxsize=None)
    def facts(self, src, kd=None, force32=False):
        """search_cases.scene_facts of the scene with its flux map, the source (None: no source) and a tree: nobody changes it"""
        t = self.tree(kd)
        return S.scene_facts(self.cs, t.flat() if t is not None else None, self.desc(src) if src else None, self.edges, force32=force32)


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(name)


# -- the calls --------------------------------------------------------------------------------------------------------------------
DEEP = ('deep', M.ORD_STACK_DEPTH - 1)     # one level more than the ordered engine's LDS stack takes
_Call = collections.namedtuple('Call', 'name scene src given stream accel kd env scene_env targets')


class Call(_Call):
    """scene: of SCENES; src: 'disk' | 'buie' | 'given'; given: the rays go in as a bundle; stream: the streaming form, or the megakernel;
    accel, kd: trace_fast's accel, a tree set on the scene (None | 'built' | ('deep', D)); env: knobs around the trace; scene_env: knobs
    around the scene's creation; targets: the instances the call is there for, as the library names them.  The attributes below are
    what test_gpu_shade_instances._check reads of a case."""
    cs = property(lambda self: scene(self.scene).cs)
    edges = property(lambda self: scene(self.scene).edges)
    map_surf = property(lambda self: scene(self.scene).map_surf)
    full_surf = property(lambda self: scene(self.scene).full_surf)
    captured = property(lambda self: scene(self.scene).captured)
    min_energy = property(lambda self: scene(self.scene).min_energy(self.src))
    reps = property(lambda self: scene(self.scene).reps)
    W, spec = 0, False

    def bundle(self, given):
        from tracer_amd.ray_bundle import RayBundle
        if not given:
            return scene(self.scene).source(self.src)
        v, d, e, rid = scene(self.scene).rays(self.src)
        return RayBundle(vertices=v.copy(), directions=d.copy(), energy=e.copy())


def _call(name, scn, src, targets, stream=True, accel=True, kd=None, env=None, scene_env=None):
    return Call(name, scn, src, src == 'given', stream, accel, kd, tuple(sorted((env or {}).items())), tuple(sorted((scene_env or {}).items())),
                tuple(targets))


def _shade(cls, flatn, lds):
    return 'k_s_shade_c<%d, %s, %s, false, false>' % (cls, S._t(flatn), S._t(lds))


MEGA = 'k_trace_coop<512, false, false, false>'


def _calls():
    out = []
    F32, NOCOOP = dict(TRC_GRID_FORCE32=1), dict(TRC_STREAM_COOP=0)
    b, coop = S._bounce, S._coop
    for scn, flat in (('gallery', False), ('flats', True)):
        lean = [_shade(0, flat, True), _shade(1, flat, True)]
        # the footprint route: the cull, the listed fresh rays (a Buie source: the cull on the mask over the rays' uniforms, the two-phase
        # form, what its map leaves out through the general path), continued rays on the grid
        out += [_call(scn + '/disk', scn, 'disk', ['k_s_cull<0>', 'k_s_fresh<0, %s, true>' % S._t(flat), b(1, True, False, flat, False)] + lean),
                _call(scn + '/buie', scn, 'buie', ['k_s_ucull<2>', 'k_s_fresh2<2, %s, true>' % S._t(flat), 'k_s_gen_src<2>',
                                                   b(1, True, False, flat, False)]),
                # given rays: the general path of fresh rays; every box (accel = False); the large grid, forced at the scene's creation, by
                # waves that share their rays' tests and lane by lane
                _call(scn + '/given', scn, 'given', ['k_s_gen<true, -1>', 'k_s_walk<256, true>', 'k_s_exact', b(1, True, False, flat, False)] + lean),
                _call(scn + '/given/boxes', scn, 'given', ['k_s_walk<256, false>', b(0, True, False, flat, False)], accel=False),
                _call(scn + '/given/grid32', scn, 'given', [coop(True, flat, False), coop(False, flat, False)], scene_env=F32),
                _call(scn + '/given/grid32/lanes', scn, 'given', [b(2, False, True, False, False), b(2, False, False, flat, False)], env=NOCOOP,
                      scene_env=F32),
                _call(scn + '/given/mega', scn, 'given', [MEGA], stream=False)]
    # the gallery's tables in global memory: over the fillers, and there with the pre-assigned chunks of the active list switched off
    full_lean = [_shade(0, False, False), _shade(1, False, False)]
    out += [_call('gallery-full/disk', 'gallery-full', 'disk', ['k_s_cull<0>', 'k_s_fresh<0, false, false>', b(1, False, False, False, False)] + full_lean),
            _call('gallery-full/given', 'gallery-full', 'given', ['k_s_exact', b(1, False, False, False, False)] + full_lean),
            _call('gallery-full/given/static', 'gallery-full', 'given', full_lean, env=dict(TRC_STREAM_STATIC=0)),
            _call('gallery/given/mega/kd', 'gallery', 'given', [MEGA], stream=False, kd='built')]
    # the unbounded list beside the grid and beside the boxes
    out += [_call('open/given', 'open', 'given', ['k_s_gen<true, -1>', 'k_s_walk<256, true>', 'k_s_exact', b(1, True, False, False, False),
                                                  _shade(0, False, True), _shade(1, False, True)]),
            _call('open/given/boxes', 'open', 'given', ['k_s_walk<256, false>', b(0, True, False, False, False)], accel=False),
            _call('open/given/mega', 'open', 'given', [MEGA], stream=False),
            _call('open/given/mega/boxes', 'open', 'given', [MEGA], stream=False, accel=False)]
    # every kind as the widest of its scene
    for scn in ALONE:
        out += [_call(scn + '/given', scn, 'given', [], stream=True), _call(scn + '/given/mega', scn, 'given', [MEGA], stream=False)]
    assert len(set(c.name for c in out)) == len(out)
    return out


CALLS = _calls()
CALL = dict((c.name, c) for c in CALLS)
# the ordered engine: (scene, tree, accel, the instance of k_ord_bounce).  trc_ordered_choose takes the conservative single-precision
# search with and without the built tree; its generic search is left to trees deeper than its LDS stack
ORDERED = [(scn, kd, accel, 'k_ord_bounce<%d, false, false>' % mode) for scn in ('gallery', 'flats', 'open')
           for kd, accel, mode in (('built', True, 1), ('built', False, 1), (DEEP, True, 0))]
# what the calls must select between them (test_geometry_cases_host.py)
MUST_SELECT = ['k_s_cull<0>', 'k_s_ucull<2>', 'k_s_fresh<0, true, true>', 'k_s_fresh<0, false, true>', 'k_s_fresh<0, false, false>', 'k_s_fresh2<2, true, true>',
               'k_s_fresh2<2, false, true>'] + \
              [S._bounce(g, l, False, f, False) for g, l in ((0, True), (1, True), (2, False)) for f in (True, False)] + \
              [S._bounce(1, False, False, False, False)] + [S._coop(fr, f, False) for fr in (True, False) for f in (True, False)] + \
              [_shade(c, f, True) for c in (0, 1) for f in (True, False)] + [_shade(c, False, False) for c in (0, 1)] + \
              ['k_ord_bounce<0, false, false>', 'k_ord_bounce<1, false, false>', MEGA]


def facts(call):
    """the fact block of a call (search_cases.facts): the scene, its tree and the footprint map as the library gathers them, the call and
    the knobs as the test makes it"""
    s = scene(call.scene)
    env, senv = dict(call.env), dict(call.scene_env)
    src = None if call.given else call.src
    f = dict(s.facts(src, call.kd, bool(int(senv.get('TRC_GRID_FORCE32', 0)))))
    f.update(n=s.n_rays, flags=(S.TRACE_STREAM if call.stream else S.TRACE_MEGAKERNEL) | (S.TRACE_ACCEL if call.accel else 0),
             src_kind=S.SRC_KIND[call.src] if src else -1, term_ok=int(s.min_energy(call.src) >= 0.))
    f.update(k_search=int(env.get('TRC_STREAM_SEARCH', 2)), k_fresh=int(int(env.get('TRC_STREAM_FRESH', 1)) != 0),
             k_bounce=int(int(env.get('TRC_STREAM_BOUNCE', 1)) != 0), k_first=int(int(env.get('TRC_STREAM_FIRST', 0)) != 0),
             k_coop=int(int(env.get('TRC_STREAM_COOP', 1)) != 0), k_absorb=int(env.get('TRC_STREAM_ABSORB', -1)),
             k_umask=int(int(env.get('TRC_STREAM_UMASK', 1)) != 0))
    return f


def launched(call):
    """(the header's decisions for the call's facts, {kernel by the library's name: launches, or None where the count depends on how
    the active lists turn out}): the megakernel once; of the streaming form the search stages as search_cases.launches counts them from
    the restated forms and the reference's live rays -- with k_s_ucull in the place of k_s_cull where the header stages it (a first
    call with a Buie source) -- the shading kernels and k_s_absorb"""
    f = facts(call)
    d = S.library_decide([f])[0]
    if not call.stream:
        return d, {d['mega']: 1}
    s = scene(call.scene)
    out = S.launches(S.forms(f), reference(call.scene, call.src)['levels'], s.n_rays, s.reps)
    if d['cull_u'][0]:
        out[d['cull_u'][0]] = out.pop(d['cull'][0])
    out.update((x[0], None) for x in d['shk'])
    if d['absorb'][0]:
        out[d['absorb'][0]] = None
    return d, out


def ordered_facts(scn, kd, accel):
    s = scene(scn)
    f = dict(s.facts(None, kd))
    f.update(n=s.n_rays, flags=S.TRACE_ACCEL if accel else 0, src_kind=-1, term_ok=1)
    return f


# -- the references -----------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(scn, src):
    """The oracle's trace of (scene, rays), computed once and shared by every call over them (nobody changes it): a descriptor source
    and the same rays given are one reference, and a tree, accel and the knobs change no ray."""
    from oracle import engine
    key = (scn, src)
    if key not in _REF:
        s = scene(scn)
        v, d, e, rid = s.rays(src)
        with N.errstate(all='ignore'):
            o = engine.trace_bundle(s.cs, v, d, e, s.reps, s.min_energy(src), SEED, offset=0)
        o['hit_list'] = sc.hit_list(o['levels'], s)
        o['maps'] = fs.host_maps(o['hit_list'], s.frames, s.edges)
        _REF[key] = o
    return _REF[key]


def levels(scn, src):
    """(vertices, directions, the surface the oracle's next level records or -1) of the live rays of every level of the reference that
    is traced on (test_mega_cases_host._levels)"""
    s, lv = scene(scn), reference(scn, src)['levels']
    out = []
    for k, L in enumerate(lv[:-1] if len(lv) > s.reps else lv):
        n = L['n_live']
        if n == 0:
            continue
        hit = N.full(n, -1)
        if k + 1 < len(lv):
            hit[lv[k + 1]['parents']] = lv[k + 1]['surf']
        out.append((N.ascontiguousarray(L['vertices'][:, :n]), N.ascontiguousarray(L['directions'][:, :n]), hit))
    return out
