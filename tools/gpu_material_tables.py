"""Tabulated materials evaluated on the device: the glass slab of tests/test_gpu_media.py (two refracting
plates of RefractiveAbsorbant between a constant and a dispersive 6-point table, one ray per hit, over a black floor), tree=False,
three alternating runs per arm:
  (a) a given bundle, device=False -- the materials' m(lambda) evaluated by their Python objects for every ray and sent as
      trc_rays.mat (k_s_shade_x<LDS>);
  (b) the same bundle, device=True -- wavelengths only, the tables on the device (k_s_shade_x<LDS, false, false, MAT>);
  (c) a pending source with a tabulated spectrum, device=True -- nothing made on the host.
Per call: wall time, kernel time (HIP events around the call's kernels, stats['kernel_ms']), bounces.  (a) and (b) trace the same rays
through the same kernels but for the instance of k_s_shade_x, launched once per bounce: the difference of their kernel times per
bounce is what MAT costs or saves per launch.  The launches' own times: run this under `rocprofv3 --kernel-trace --stats --`.
usage: gpu_material_tables.py [rays, default 2e6] [runs, default 3]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as N
from tracer_amd import optics_callables as opt
from tracer_amd.assembly import Assembly
from tracer_amd.object import AssembledObject
from tracer_amd.surface import Surface
from tracer_amd.flat_surface import RectPlateGM
from tracer_amd.spatial_geometry import translate
from tracer_amd.ray_bundle import RayBundle
from tracer_amd.sources import rect_bundle
from tracer_amd.source_spectrum import SourceSpectrum
from tracer_amd.tracer_engine import TracerEngine

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2000000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
REPS, MIN_ENERGY = 7, 1e-9
TL = N.linspace(0.3e-6, 2.5e-6, 6)


def slab_scene(device):
    air = opt.TabulatedMaterial(TL, N.ones(6), N.zeros(6), device=device)
    glass = opt.TabulatedMaterial(TL, [1.55, 1.53, 1.51, 1.50, 1.49, 1.47], [3e-8, 2e-8, 1e-8, 5e-8, 2e-7, 6e-7], device=device)
    plate = lambda z: AssembledObject(surfs=[Surface(RectPlateGM(40., 40.), opt.RefractiveAbsorbant(air, glass, single_ray=True, attenuation_coefficient_1=1.))],
                                      transform=translate(0., 0., z))
    floor = AssembledObject(surfs=[Surface(RectPlateGM(60., 60.), opt.LambertianReceiver(1.))], transform=translate(0., 0., -1.))
    return Assembly(objects=[plate(0.5), plate(0.), floor]), air


rng = N.random.RandomState(11)
v = N.vstack((rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), N.full(n, 3.)))
d = N.vstack((rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), -N.ones(n)))
d /= N.sqrt(N.sum(d ** 2, axis=0))
wl = rng.uniform(0.4e-6, 2.4e-6, n)
spectrum = SourceSpectrum.uniform(0.4e-6, 2.4e-6)

arms = [('a: given bundle, rows from the host', False, False), ('b: given bundle, tables on the device', True, False),
        ('c: pending spectral source, tables on the device', True, True)]
engines, air_of = {}, {}
for name, device, pending in arms:
    asm, air_of[name] = slab_scene(device)
    engines[name] = TracerEngine(asm)
wall, kernel, bounces = dict((a[0], []) for a in arms), dict((a[0], []) for a in arms), {}
for r in range(runs + 1):           # (the first round warms up: workspace allocation, the scene's upload)
    for name, device, pending in arms:
        eng = engines[name]
        eng.reset_tallies()
        t0 = time.time()
        if pending:
            b = rect_bundle(n, N.array([0., 0., 3.]), N.array([0., 0., -1.]), 2., 2., 0.6, flux=1., seed=100 + r, spectrum=spectrum)
        else:
            b = RayBundle(vertices=v, directions=d, energy=N.ones(n) / n, ref_index=air_of[name].m(wl), wavelengths=wl)
        eng.ray_tracer(b, reps=REPS, min_energy=MIN_ENERGY, tree=False, seed=21)
        w = time.time() - t0
        eng._asm.reset_all_optics()
        assert eng.stats['engine'] == 'fast' and eng.stats['form'] == 'stream', eng.stats
        assert not pending or b.is_pending()
        if r > 0:
            wall[name].append(w * 1e3)
            kernel[name].append(eng.stats['kernel_ms'])
        bounces[name] = eng.stats['bounces']
        print('%-50s run %d%s: call %8.2f ms, kernels %7.3f ms, %d segments, %d bounces, %d launches' % (
            name, r, ' (warm-up)' if r == 0 else '', w * 1e3, eng.stats['kernel_ms'], eng.stats['segments'], eng.stats['bounces'], eng.stats['launches']), flush=True)
print('glass slab, %d rays, reps %d: per call (bundle made, traced; median of %d, [min, max])' % (n, REPS, runs))
for name, device, pending in arms:
    print('  %-50s call %8.2f [%8.2f, %8.2f] ms   kernels %7.3f [%7.3f, %7.3f] ms' % (
        name, N.median(wall[name]), min(wall[name]), max(wall[name]), N.median(kernel[name]), min(kernel[name]), max(kernel[name])))
a, b = arms[0][0], arms[1][0]
diff = N.median(kernel[b]) - N.median(kernel[a])
spread = max(max(kernel[a]) - min(kernel[a]), max(kernel[b]) - min(kernel[b]))
print('k_s_shade_x, MAT against rows: %+.4f ms of kernel time per call, %+.4f ms per launch (%d launches); run-to-run spread of an arm %.4f ms'
      % (diff, diff / max(bounces[a], 1), bounces[a], spread))
