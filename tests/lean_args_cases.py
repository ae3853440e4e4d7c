"""
The scenes and calls of test_gpu_lean_args.py: the smallest shapes that reach the instances of the streaming kernels that read their
arguments again in every turn of their loops (k_s_bounce for continued rays, k_s_fresh2: kernel_args_again,
csrc/trc_device.h), and their neighbours that do not.  Each is traced twice: by the streaming form as a script gets it, and by
the megakernel (stream=False: k_trace_coop), which shares no kernel with the streaming form -- only the per-ray core.

A small heliostat field: mirrors on the ground tilted to send the sun to an aim point, a plate that absorbs everything up on a
"tower" at that point.

  field3        3 mirrors + the plate, Buie disc         k_s_cull, k_s_fresh2, surface by surface (4 surfaces: k_s_bounce<3>),
                                                         k_s_shade_c<mirror>
  field6        6 mirrors + the plate, Buie disc         ... the grid in LDS with the plate set apart from it: k_s_bounce<1, LDS>, the
                                                         terminal hits finished inside
  pillbox       field6 under a pillbox disc              k_s_fresh
  absorb        field6, TRC_STREAM_ABSORB=1              the terminal list behind k_s_bounce, finished by k_s_absorb
  diffuse       1 mirror + 1 diffuse plate + the plate   two classes: k_s_partition, k_s_shade_c<diffuse>
  dish          field6 with a paraboloid among them      the instances that carry the quadric code (FLAT = false)
  given         field6, the Buie rays as host arrays     k_s_bounce<.., FRESH>

Run as a program -- `lean_args_cases.py stream|mega case ...` -- it traces the cases named and prints one JSON line: that is how the
test hands a call an environment of its own, in a fresh process (the knobs of the library are environment variables).
"""
import json
import os
import sys

import numpy as N

N_RAYS = 20000
REPS = 4
SEED = 4711
SUN = N.r_[0.12, -0.2, -1.] / N.linalg.norm([0.12, -0.2, -1.])
AIM = N.r_[0., 9., 30.]
PLATE = 5.                                         # side of the absorbing plate
MAP_EDGES = (N.linspace(-2.5, 2.5, 14), N.linspace(-2.5, 2.5, 12))      # its flux map: the whole plate, 13 x 11 bins

CASES = {          # name: (mirrors, source, extra surfaces, environment of the streaming call, rays given as host arrays)
    'field3': (3, 'buie', None, {}, False),
    'field6': (6, 'buie', None, {}, False),
    'pillbox': (6, 'pillbox', None, {}, False),
    'absorb': (6, 'buie', None, dict(TRC_STREAM_ABSORB=1), False),
    'diffuse': (1, 'buie', 'diffuse', {}, False),
    'dish': (6, 'buie', 'dish', {}, False),
    'given': (6, 'buie', None, {}, True),
}


def _pose(normal, at):
    """a frame whose z axis is `normal`, at point `at`"""
    from tracer_amd.spatial_geometry import rotation_to_z
    tr = N.eye(4)
    tr[:3, :3] = rotation_to_z(N.asarray(normal, dtype=float))
    tr[:3, 3] = at
    return tr


def scene(mirrors, extra):
    """(assembly, index of the absorbing plate)"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.paraboloid import ParabolicDishGM
    from tracer_amd import optics_callables as opt
    objs = []
    spots = [N.r_[3.2 * (k % 3 - 1), -3.4 * (k // 3), 0.3 * k] for k in range(mirrors)]
    for p in spots:
        out = (AIM - p) / N.linalg.norm(AIM - p)
        n = (out - SUN) / N.linalg.norm(out - SUN)                # the mirror law: sun in, aim point out
        objs.append(AssembledObject(surfs=[Surface(RectPlateGM(2.2, 1.7), opt.RealReflective(0.06, 2e-3))], transform=_pose(n, p)))
    if extra == 'diffuse':          # a second class: a diffuse plate beside the mirror, facing the sun
        objs.append(AssembledObject(surfs=[Surface(RectPlateGM(2.4, 2.), opt.LambertianReceiver(0.35))], transform=_pose(-SUN, N.r_[3.4, 0.4, 0.2])))
    if extra == 'dish':             # a curved surface: a small dish looking at the sun
        objs.append(AssembledObject(surfs=[Surface(ParabolicDishGM(2., 1.5), opt.RealReflective(0.1, 2e-3))], transform=_pose(-SUN, N.r_[-6.6, -1.5, 0.1])))
    towards = (N.r_[0., -1.7, 0.] - AIM) / N.linalg.norm(N.r_[0., -1.7, 0.] - AIM)
    objs.append(AssembledObject(surfs=[Surface(RectPlateGM(PLATE, PLATE), opt.LambertianReceiver(1.))], transform=_pose(towards, AIM)))
    return Assembly(objects=objs), len(objs) - 1


def source(kind):
    from tracer_amd import sources
    centre = N.c_[N.r_[0., -1.7, 0.] - 60. * SUN]
    if kind == 'buie':
        return sources.buie_sunshape(N_RAYS, centre, SUN, 8.5, 0.03, flux=1000., seed=SEED)
    return sources.disk_bundle(N_RAYS, centre, SUN, 8.5, 4.65e-3, flux=1000., seed=SEED)


def bundle(kind, given):
    """the pending bundle of the source, or the same rays made on the host"""
    b = source(kind)
    if not given:
        return b
    from oracle import engine, sources
    from tracer_amd.ray_bundle import RayBundle
    desc, n, seed, off = b.source_args()
    v, d, e, rid = sources.generate(engine.source_from_desc(desc), n, seed, off)
    return RayBundle(vertices=v.copy(), directions=d.copy(), energy=e.copy())


def trace(name, stream):
    """the tallies, statistics, flux map and captured hits of a case, as plain lists (in the environment as it is); stream: the
    streaming form, else the megakernel"""
    from tracer_amd import _cabi
    from tracer_amd.scene import DeviceScene, compile_scene
    mirrors, kind, extra, knobs, given = CASES[name]
    asm, plate = scene(mirrors, extra)
    cs = compile_scene(asm)
    dev = DeviceScene(cs, _cabi.get_context(0))
    dev.set_fluxmap(plate, *MAP_EDGES)
    dev.set_hit_capacity(4 * N_RAYS)
    st, _ = dev.trace_fast(bundle(kind, given), REPS, 1e-10, SEED, accel=True, stream=stream)
    a, r, h = dev.get_tallies()
    hits = dev.get_hits()
    fm = dev.get_fluxmap(plate)
    dev.close()
    o = N.lexsort((hits['points'][2], hits['points'][1], hits['points'][0], hits['surf']))
    return dict(plate=plate, a=a.tolist(), r=r.tolist(), h=N.asarray(h).tolist(), segments=int(st.segments), hits=int(st.hits),
                dropped=int(st.hits_dropped), fm=fm.tolist(), hit_surf=N.asarray(hits['surf'])[o].tolist(),
                hit_e=N.asarray(hits['e_abs'])[o].tolist(), hit_points=N.asarray(hits['points'])[:, o].tolist())


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(dict((name, trace(name, sys.argv[1] == 'stream')) for name in sys.argv[2:])))
