"""A polychromatic source on the box of tools/gpu_poly.py (a polychromatic wall that keeps every hit's spectra, a mirror, a diffuse
wall), fast engine, tree=False: (a) the rays as a given bundle with host-made (W, n) columns `wavelengths` and `spectra` -- the only
way in before SourceSpectrum.polychromatic -- against (b) the pending source that carries its spectrum (k_s_shade_p: nothing of
size W x n is made or uploaded).  The same rays on the same Philox streams both ways; alternating runs; per run the kernel time and
the time of the call, for (a) also what making its two columns on the host took.
usage: gpu_poly_source.py [rays, default 2e6] [W, default 16] [runs of each, default 3]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as N
from tracer_amd import optics_callables as opt, sources
from tracer_amd.assembly import Assembly
from tracer_amd.object import AssembledObject
from tracer_amd.surface import Surface
from tracer_amd.flat_surface import RectPlateGM
from tracer_amd.spatial_geometry import translate, rotx
from tracer_amd.ray_bundle import RayBundle
from tracer_amd.source_spectrum import SourceSpectrum, planck
from tracer_amd.tracer_engine import TracerEngine

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2000000
W = int(sys.argv[2]) if len(sys.argv) > 2 else 16
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
REPS, SEED = 6, 33


def poly_scene():
    ths = N.linspace(0., N.pi / 2., 7)
    wls = N.linspace(0.25e-6, 2.6e-6, 5)
    grid = 0.2 + 0.7 * N.outer(N.cos(ths) ** 0.5, 1. / (1. + (wls * 1e6 - 1.) ** 2))
    wall = opt.Lambertian_directional_axisymmetric_piecewise_PolychromaticAbsorberPolychromatic(ths, grid, wls)      # (absorbed energy and absorbed spectrum per hit)
    floor = AssembledObject(surfs=[Surface(RectPlateGM(4., 4.), wall)], transform=translate(0., 0., 0.))
    roof = AssembledObject(surfs=[Surface(RectPlateGM(4., 4.), opt.Reflective(0.1))], transform=N.dot(translate(0., 0., 1.5), rotx(N.pi)))
    side = AssembledObject(surfs=[Surface(RectPlateGM(4., 1.5), opt.Lambertian(0.3))], transform=N.dot(translate(0., 2., 0.75), rotx(N.pi / 2.)))
    return Assembly(objects=[floor, roof, side])


grid = N.linspace(0.3e-6, 2.5e-6, W)
spectrum = SourceSpectrum.polychromatic(grid, planck(grid, 5777.))          # the sun as a black body, W samples
source = lambda spec: sources.rect_bundle(n, N.c_[[0., 0., 1.]], N.r_[0., 0., -1.], 2., 2., 0.4, flux=1000., seed=SEED, ray_offset=0, spectrum=spec)
plain = source(None)
v, d, e = plain.get_vertices(), plain.get_directions(), plain.get_energy()      # (the rays themselves: made once, not timed)
wl, val, _ = spectrum.table()

engines = {'a': TracerEngine(poly_scene()), 'b': TracerEngine(poly_scene())}
tallies = {}
for r in range(runs + 1):           # (run 0 of each warms up: workspaces, the hit buffer)
    for route in ('a', 'b'):
        eng = engines[route]
        eng.reset_tallies()
        made = 0.
        if route == 'a':
            t0 = time.time()
            swl = N.ascontiguousarray(N.broadcast_to(wl[:, None], (W, n)))
            spec = e * val[:, None]
            made = time.time() - t0
            b = RayBundle(vertices=v, directions=d, energy=e, spectra=spec, wavelengths=swl)
        else:
            b = source(spectrum)
        t0 = time.time()
        eng.ray_tracer(b, reps=REPS, min_energy=1e-9, tree=False, seed=SEED)
        call = time.time() - t0
        assert eng.stats['engine'] == 'fast' and eng.stats['form'] == 'stream' and (route == 'a' or b.is_pending())
        tallies[route] = eng.get_tallies()
        eng._asm.reset_all_optics()
        print('%s, %d rays x %d samples, run %d%s: kernels %.2f ms, call %.1f ms%s, %d segments' %
              ('(a) given bundle, host columns' if route == 'a' else '(b) pending carried source   ', n, W, r, ' (warm-up)' if r == 0 else '',
               eng.stats['kernel_ms'], call * 1e3, ', making the two columns %.1f ms' % (made * 1e3) if route == 'a' else '', eng.stats['segments']), flush=True)
(aa, ar, ah), (ba, br, bh) = tallies['a'], tallies['b']
print('same rays both ways: hits per surface equal %s, absorbed energy within %.2g (relative)' % (N.array_equal(ah, bh), N.abs(aa - ba).max() / aa.max()))
