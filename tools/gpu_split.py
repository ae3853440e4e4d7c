"""Ray-splitting refraction, fast engine (streaming form, k_s_shade_x<.., SPLIT>) against the ordered engine, tree=False: the lens of the
engine fixture (tests/golden/make_golden.py scene_lens: a paraboloidal cap over a round plate, both RefractiveHomogenous(1, 1.5,
single_ray=False)) over a detector that captures every hit.  Three alternating runs of a given bundle; kernel time and call time.
usage: gpu_split.py [rays, default 2e6] [runs, default 3]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as N
from tracer_amd import optics_callables as opt
from tracer_amd.assembly import Assembly
from tracer_amd.object import AssembledObject
from tracer_amd.surface import Surface
from tracer_amd.flat_surface import RectPlateGM, RoundPlateGM
from tracer_amd.paraboloid import ParabolicDishGM
from tracer_amd.spatial_geometry import translate, rotx
from tracer_amd.ray_bundle import RayBundle
from tracer_amd.tracer_engine import TracerEngine

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2000000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
REPS, MIN_ENERGY = 8, 1e-6 / n          # (a ray is followed down to a millionth of what it started with)


def lens_scene():
    h = (2. / (2. * N.sqrt(1.5))) ** 2
    front = Surface(ParabolicDishGM(4., 1.5), opt.RefractiveHomogenous(1., 1.5, single_ray=False), location=N.r_[0., 0., h], rotation=rotx(N.pi)[:3, :3])
    back = Surface(RoundPlateGM(2.), opt.RefractiveHomogenous(1., 1.5, single_ray=False))
    lens = AssembledObject(surfs=[front, back], transform=translate(0., 0., 1.))
    detector = AssembledObject(surfs=[Surface(RectPlateGM(6., 6.), opt.LambertianDetector(1.))], transform=translate(0., 0., -4.))
    return Assembly(objects=[lens, detector])


rng = N.random.RandomState(8)
v = N.vstack((rng.uniform(-1.6, 1.6, n), rng.uniform(-1.6, 1.6, n), N.full(n, 3.)))
d = N.vstack((rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), -N.ones(n)))
d /= N.sqrt(N.sum(d ** 2, axis=0))
engines = dict((name, TracerEngine(lens_scene())) for name in ('fast', 'ordered'))
kernel = dict(fast=[], ordered=[])
tallies = {}
for r in range(runs):
    for name in ('fast', 'ordered'):
        eng = engines[name]
        b = RayBundle(vertices=v, directions=d, energy=N.ones(n) / n)
        eng.reset_tallies()
        t0 = time.time()
        eng.ray_tracer(b, reps=REPS, min_energy=MIN_ENERGY, tree=False, seed=33 + r, engine=name)
        wall = time.time() - t0
        t0 = time.time()
        got = eng._asm.get_surfaces()[2].get_optics_manager().get_all_hits()
        read = time.time() - t0
        eng._asm.reset_all_optics()
        kernel[name].append(eng.stats['kernel_ms'])
        tallies[name] = eng.get_tallies()
        print('lens over a detector, %d rays, %s engine, run %d: call %.1f ms, kernels %.2f ms, %d segments, %d hits, %d rays left (%.0f M segments/s by kernel time); '
              'reading the detector\'s %d hits %.1f ms' % (n, name, r, wall * 1e3, eng.stats['kernel_ms'], eng.stats['segments'], eng.stats['hits'],
                                                           eng.stats['rays_left'], eng.stats['segments'] / eng.stats['kernel_ms'] / 1e3, len(got[0]), read * 1e3), flush=True)
(af, rf, hf), (ao, ro, ho) = tallies['fast'], tallies['ordered']
print('hits per surface: fast %s, ordered %s; absorbed agrees to %.3g' % (list(hf), list(ho), N.abs(af - ao).max()))
print('kernel time: slowest fast run %.2f ms, fastest ordered run %.2f ms: %s' % (max(kernel['fast']), min(kernel['ordered']),
      "engine='auto' may take the fast route" if max(kernel['fast']) < min(kernel['ordered']) else "engine='auto' stays with the ordered engine"))
