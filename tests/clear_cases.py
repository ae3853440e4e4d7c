"""
The scenes of the tests of the clear cones (csrc/trc_bounds.h: trc_clear_build; k_s_bounce on the LDS-sized grid), shared by
tests/test_clear_cones_host.py, tests/test_gpu_clear_cones.py and tools/clear_cones.py.  Every scene is a set of heliostats (one flat
plate each) that track the sun onto a receiver standing far enough above them for the grid to set it apart -- the grid sets a surface
apart only in scenes of more than four bounded surfaces, so the small scenes carry four plates that stand clear of everything beside
the plates they are about, two on either side, so that the receiver alone is set apart (no single plate holds a face of the
field's box).
"""
import os
import struct
import ctypes as C

import numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZENITH = 35.05 * N.pi / 180.
TOWER = 40.
BYSTANDERS = [[25., 28., 0.], [25., 44., 0.], [-25., 28., 0.], [-25., 44., 0.]]


def _plant(pos, extra_objects=(), azimuth=N.pi, zenith=ZENITH, size=6.1, receiver=True, aim_height=TOWER, sigma=1e-3):
    """(plant, field, source arguments): heliostats at `pos` aimed at (0, 0, aim_height), the receiver there.  The sun stands behind
    the tower (azimuth pi): the plates are tilted by 40 degrees, and a neighbour of their height does not stretch the field's box"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.models.heliostat_field import HeliostatField, solar_vector
    from tracer_amd.models.one_sided_mirror import one_sided_receiver
    from tracer_amd.spatial_geometry import rotx, translate
    pos = N.asarray(pos, dtype=float)
    field = HeliostatField(pos, size, size, absorptivity=0.04, sigma=sigma, bi_var=True, MCRT_option='fast')
    field.track_sun(azimuth, zenith, aim_points=N.tile(N.array([0., 0., aim_height]), (pos.shape[0], 1)))
    objs = list(extra_objects)
    if receiver:
        rec = one_sided_receiver(11., 11.)
        rec.set_transform(N.dot(translate(0., 0., aim_height), rotx(-N.pi / 2.)))
        objs = [rec] + objs
    plant = Assembly(objects=objs, subassemblies=[field])
    sun = solar_vector(azimuth, zenith)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    centre = N.r_[(lo[:2] + hi[:2]) / 2., 0.]
    radius = 1.10 * N.sqrt(N.sum(((hi[:2] - lo[:2]) / 2.) ** 2)) + size
    src = dict(center=N.vstack(300. * sun + centre), direction=-sun, radius=radius, CSR=0.01, flux=1000., pre_process_CSR=False)
    return plant, field, src


def shadowing():
    """three plates in a column towards the tower, 4.2 m apart: each stands in the lower part of the beam of the one behind it"""
    return _plant([[0., 30., 0.], [0., 34.2, 0.], [0., 38.4, 0.]] + BYSTANDERS)


def side_by_side():
    """two plates side by side, 6.3 m between their centres: their axial ranges overlap, neither is in the other's beam"""
    return _plant([[-3.15, 36., 0.], [3.15, 36., 0.]] + BYSTANDERS)


def quadric_neighbours():
    """a plate whose neighbours towards the tower are a sphere and a cylinder: their oriented boxes are boxes of quadrics"""
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.sphere_surface import SphericalGM
    from tracer_amd.cylinder import FiniteCylinder
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate
    ball = AssembledObject(surfs=[Surface(SphericalGM(0.9), opt.Reflective(0.5))], transform=translate(1.5, 35., 0.9))
    mast = AssembledObject(surfs=[Surface(FiniteCylinder(1.0, 3.6), opt.Reflective(0.5))], transform=translate(-2., 35., 0.))
    return _plant([[0., 40., 0.], [9., 40., 0.], [-9., 40., 0.]] + BYSTANDERS, extra_objects=[ball, mast])


def random_slab(n=200, seed=3):
    """n tilted plates of 2 m scattered in a slab 120 x 80 x 6 m, aimed at a far target"""
    rng = N.random.RandomState(seed)
    pos = N.c_[rng.uniform(-60., 60., n), rng.uniform(40., 120., n), rng.uniform(0., 6., n)]
    return _plant(pos, size=2., aim_height=90.)


def no_apart():
    """six plates and no receiver: nothing is set apart from the grid, and nothing gets a cone"""
    return _plant([[-7., 30., 0.], [0., 30., 0.], [7., 30., 0.], [-7., 37., 0.], [0., 37., 0.], [7., 37., 0.]], receiver=False)


def nsttf(n_heliostats=None):
    from tracer_amd import scenes
    plant, field, rec, src = scenes.nsttf_field(n_heliostats=n_heliostats)
    return plant, field, src


SCENES = [('nsttf', nsttf), ('shadowing', shadowing), ('side_by_side', side_by_side), ('quadric_neighbours', quadric_neighbours),
          ('random_slab', random_slab), ('no_apart', no_apart)]


def compiled(make):
    from tracer_amd.scene import compile_scene
    plant, field, src = make()
    return compile_scene(plant), src


def source_desc(src, n=10, seed=1):
    from tracer_amd import scenes
    return scenes.nsttf_source(n, src, seed=seed).source_args()[0]


def load_check():
    """the host check's library (make clearcheck), with its argument types"""
    import subprocess
    subprocess.check_call(['make', '-s', '-C', ROOT, 'clearcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'clearcheck', 'libtrc_clear_check.so'))
    p = C.POINTER(C.c_double)
    lib.cc_sound.restype = C.c_int
    lib.cc_sound.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_uint64, C.c_double, p]
    lib.cc_walk_share.restype = C.c_int
    lib.cc_walk_share.argtypes = [C.c_int, C.c_void_p, p, C.c_void_p, C.c_long, C.c_uint64, C.c_int, C.POINTER(C.c_int), p, p]
    lib.cc_build_time.restype = C.c_double
    lib.cc_build_time.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    return lib


def sound(lib, cs, T, n_rays, seed=1, kscale=1.):
    out = N.zeros(12)
    rc = lib.cc_sound(cs.n_surf, C.addressof(cs.descs), T, n_rays, seed, kscale, out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


def walk_share(lib, cs, src, n, Ts, seed=2024):
    desc = source_desc(src)
    extra = N.ascontiguousarray(cs.extra if len(cs.extra) else N.zeros(1), dtype=float)
    ts = (C.c_int * len(Ts))(*Ts)
    out, tail = N.zeros(4 * len(Ts)), N.zeros(4)
    p = C.POINTER(C.c_double)
    rc = lib.cc_walk_share(cs.n_surf, C.addressof(cs.descs), extra.ctypes.data_as(p), C.addressof(desc), int(n), seed, len(Ts), ts,
                           out.ctypes.data_as(p), tail.ctypes.data_as(p))
    return rc, out.reshape(len(Ts), 4), tail


def write_cases(path, cases, T, n_rays):
    """the scenes in the form tests/clearcheck/clear_check reads as a program of its own"""
    with open(path, 'wb') as f:
        for cs in cases:
            f.write(struct.pack('<iiq', cs.n_surf, T, n_rays))
            f.write(bytes(C.string_at(C.addressof(cs.descs), C.sizeof(cs.descs))))
