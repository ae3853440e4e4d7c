"""
The spectra of the captured hits of the polychromatic box (tools/gpu_poly_source.py: a polychromatic wall for a floor, a mirror, a
diffuse wall), reduced two ways on the hits of the same call -- a 50 x 50 spectral flux map of the floor, and the absorbed spectrum
of every surface:
  device  TracerEngine.histogram_spectra and surface_spectra: the hits binned where they lie (k_hist_hits_x), the sums come back
  host    DeviceScene.get_hits() -- 8 + 3 W float64 columns per hit packed on the device and copied to page-locked host arrays -- then
          NumPy: the bin of every hit once (searchsorted), numpy.bincount per sample; a sum per surface
A warm-up and five repetitions, one ray_tracer(tree=False, feed=False) call each; the two ways alternate in order from one
repetition to the next.  Prints per repetition the wall times, the time of the kernel alone between two device events, and the bytes
it reads -- per slice the surface of every reserved entry and the chart's three columns of every hit, per sample the wavelength, the
arrived and the left spectrum of every hit -- against the 8 TB/s of the memory; then medians and spread (min .. max).  One JSON
object on the last line.
    python tools/gpu_hit_spectra.py [--rays N] [--samples W] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0
REPS, SEED, FLOOR = 6, 33, 0
LDS_WORDS = 8192


def poly_scene():
    from tracer_amd import optics_callables as opt
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.spatial_geometry import translate, rotx
    ths = N.linspace(0., N.pi / 2., 7)
    wls = N.linspace(0.25e-6, 2.6e-6, 5)
    grid = 0.2 + 0.7 * N.outer(N.cos(ths) ** 0.5, 1. / (1. + (wls * 1e6 - 1.) ** 2))
    wall = opt.Lambertian_directional_axisymmetric_piecewise_PolychromaticAbsorberPolychromatic(ths, grid, wls)
    floor = AssembledObject(surfs=[Surface(RectPlateGM(4., 4.), wall)], transform=translate(0., 0., 0.))
    roof = AssembledObject(surfs=[Surface(RectPlateGM(4., 4.), opt.Reflective(0.1))], transform=N.dot(translate(0., 0., 1.5), rotx(N.pi)))
    side = AssembledObject(surfs=[Surface(RectPlateGM(4., 1.5), opt.Lambertian(0.3))], transform=N.dot(translate(0., 2., 0.75), rotx(N.pi / 2.)))
    return Assembly(objects=[floor, roof, side])


def slices(nu, nv, W, counts):
    """the slices k_hist_hits_x passes over the entries in (trc_hit_hist_x_plan_for, trc_hithist.h)"""
    nb = nu * nv
    fixed = (nu + 1) + (nv + 1) + (nb if counts else 0) + 2
    ks = min(max((LDS_WORDS - fixed) // (nb + 1), 0) or LDS_WORDS - 2, W)
    return -(-W // ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=float, default=2e6)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from tracer_amd import _cabi, sources
    from tracer_amd.source_spectrum import SourceSpectrum, planck
    from tracer_amd.tracer_engine import TracerEngine
    ctx = _cabi.get_context(0)
    n, W = int(args.rays), args.samples
    wl = N.linspace(0.3e-6, 2.5e-6, W)
    spectrum = SourceSpectrum.polychromatic(wl, planck(wl, 5777.))
    eng = TracerEngine(poly_scene())
    ue = ve = N.linspace(-2., 2., 51)
    runs, worst = [], {'map': 0., 'surfaces': 0.}
    for rep in range(args.reps + 1):
        b = sources.rect_bundle(n, N.c_[[0., 0., 1.]], N.r_[0., 0., -1.], 2., 2., 0.4, flux=1000., seed=SEED, ray_offset=rep * n, spectrum=spectrum)
        t0 = time.time()
        eng.ray_tracer(b, reps=REPS, min_energy=1e-9, tree=False, seed=SEED, feed=False)
        ctx.synchronize()
        dev = eng._dev
        entries = dev.hits_reserved()[0]
        run = {'trace_ms': (time.time() - t0) * 1e3, 'entries': int(entries)}

        def device():
            t = time.time()
            M = eng.histogram_spectra(FLOOR, ue, ve)
            run['map_ms'] = (time.time() - t) * 1e3
            run['map_kernel_ms'] = dev.histogram_hits_ms()
            t = time.time()
            S = eng.surface_spectra()
            run['surfaces_ms'] = (time.time() - t) * 1e3
            run['surfaces_kernel_ms'] = dev.histogram_hits_ms()
            return M, S

        def host():
            t = time.time()
            hits = dev.get_hits()
            run['read_ms'] = (time.time() - t) * 1e3
            arrived, left, swl = hits['spectra']
            assert N.array_equal(swl[:, 0], wl)
            absorbed = arrived - left
            surf = hits['surf']
            S = N.stack([N.bincount(surf, weights=absorbed[j], minlength=dev.n_surf) for j in range(W)], axis=-1)
            run['host_surfaces_ms'] = (time.time() - t) * 1e3
            t1 = time.time()
            k = N.nonzero(surf == FLOOR)[0]
            x, y = hits['points'][0][k], hits['points'][1][k]           # (the floor's frame is the global one)
            iu = N.minimum(N.searchsorted(ue, x, side='right') - 1, 49)
            iv = N.minimum(N.searchsorted(ve, y, side='right') - 1, 49)
            inside = (x >= ue[0]) & (x <= ue[-1]) & (y >= ve[0]) & (y <= ve[-1])
            flat = (iu * 50 + iv)[inside]
            M = N.stack([N.bincount(flat, weights=absorbed[j][k][inside], minlength=2500) for j in range(W)], axis=-1).reshape(50, 50, W)
            run['host_map_ms'] = run['read_ms'] + (time.time() - t1) * 1e3
            run['hits'], run['floor_hits'] = int(len(surf)), int(len(k))
            return M, S
        (Md, Sd), (Mh, Sh) = (device(), host()) if rep % 2 else (host(), device())[::-1]
        dev.lib.trc_scene_clear_hits(dev.handle)
        worst['map'] = max(worst['map'], float(N.abs(Md.sum - Mh).max() / Mh.max()))
        worst['surfaces'] = max(worst['surfaces'], float(N.abs(Sd.sum - Sh).max() / Sh.max()))
        # (both passes hold the hits to the grid: three columns per sample)
        run['map_bytes'] = slices(50, 50, W, False) * (4 * run['entries'] + 24 * run['floor_hits']) + 24 * W * run['floor_hits']
        run['surfaces_bytes'] = slices(dev.n_surf, 1, W, True) * 4 * run['entries'] + 24 * W * run['hits']
        for what in ('map', 'surfaces'):
            ms = run[what + '_kernel_ms']
            run[what + '_tb_per_s'] = run[what + '_bytes'] / (ms * 1e-3) / 1e12 if ms > 0 else 0.
        if rep == 0:
            continue            # (warm-up: workspaces, the hit buffer, page-locked blocks)
        run['first'] = 'device' if rep % 2 else 'host'
        runs.append(run)
        print('rep %d (%s first): trace %.1f ms, %d hits (%d on the floor) in %d entries, %d samples\n'
              '   50 x 50 map: device %.3f ms (kernel %.3f ms, %.0f MB, %.2f TB/s = %.0f %% of %.0f); get_hits + NumPy %.1f ms\n'
              '   per surface: device %.3f ms (kernel %.3f ms, %.0f MB, %.2f TB/s = %.0f %% of %.0f); get_hits + NumPy %.1f ms; get_hits alone %.1f ms'
              % (rep, run['first'], run['trace_ms'], run['hits'], run['floor_hits'], entries, W,
                 run['map_ms'], run['map_kernel_ms'], run['map_bytes'] / 1e6, run['map_tb_per_s'], 100. * run['map_tb_per_s'] / PEAK_TBS, PEAK_TBS, run['host_map_ms'],
                 run['surfaces_ms'], run['surfaces_kernel_ms'], run['surfaces_bytes'] / 1e6, run['surfaces_tb_per_s'],
                 100. * run['surfaces_tb_per_s'] / PEAK_TBS, PEAK_TBS, run['host_surfaces_ms'], run['read_ms']), flush=True)
    med = {}
    for k in ('map_ms', 'map_kernel_ms', 'map_tb_per_s', 'host_map_ms', 'surfaces_ms', 'surfaces_kernel_ms', 'surfaces_tb_per_s', 'host_surfaces_ms',
              'read_ms', 'trace_ms'):
        v = N.array([r[k] for r in runs])
        med[k] = {'median': float(N.median(v)), 'min': float(v.min()), 'max': float(v.max())}
        print('%-18s median %.3f (%.3f .. %.3f)' % (k, med[k]['median'], med[k]['min'], med[k]['max']))
    print('device against the host route, largest difference of the largest bin: map %.3g, per surface %.3g' % (worst['map'], worst['surfaces']))
    out = {'rays': n, 'samples': W, 'reps': args.reps, 'device': ctx.device_name(), 'map_slices': slices(50, 50, W, False), 'runs': runs,
           'medians': med, 'device_vs_host': worst}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
