"""
The flux map of a cylindrical receiver three ways, alternating, a warm-up round and three runs each:
  chart   the (z, azimuth) map binned on the device (set_fluxmap(.., chart='cylinder')), no hit captured
  xy      the same scene with an (x, y) map of equal bin count: chart - xy is the cost of the chart arithmetic
  host    the route without the chart: every hit of the receiver captured, the hit list read, FiniteCylinder.get_fluxmap on the host
The scene is an external cylindrical receiver (diameter 2, height 3, absorptivity 0.9, diffuse) over a diffuse ground plate that
sends part of what misses the receiver back up, lit by a disc source from the side and above.
Prints per run the kernel time of the call (HIP events) and the wall time until the map is in host memory; the chart map is checked
against the host route's once.  One JSON object on the last line.
    python tools/gpu_fluxmap_charts.py [--rays N] [--bins B] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tower(capture):
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.cylinder import FiniteCylinder
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate, rotx, rotz
    T = N.dot(translate(3., -2., 10.), N.dot(rotx(0.3), rotz(0.5)))
    wall = opt.LambertianReceiver(0.9) if capture else opt.Lambertian(0.9)
    objs = [AssembledObject(surfs=[Surface(FiniteCylinder(2., 3.), wall)], transform=N.dot(T, translate(0., 0., 1.5))),
            AssembledObject(surfs=[Surface(RectPlateGM(12., 12.), opt.Lambertian(0.5))], transform=T)]
    return Assembly(objects=objs), T


def source(n, T, seed):
    from tracer_amd import sources
    d = N.r_[1., 0.3, -0.7]
    d = d / N.linalg.norm(d)
    c = N.r_[0., 0., 1.5] - 8. * d
    return sources.disk_bundle(n, N.c_[N.dot(T[:3, :3], c) + T[:3, 3]], N.dot(T[:3, :3], d), 2.2, 0.05, flux=1000., seed=seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=10000000)
    ap.add_argument('--bins', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from tracer_amd import _cabi
    from tracer_amd.scene import DeviceScene, compile_scene
    ctx = _cabi.get_context(0)
    n, B = args.rays, args.bins
    asm, T = tower(False)
    asm_c, _ = tower(True)
    cs, cs_c = compile_scene(asm), compile_scene(asm_c)
    gm = asm.get_surfaces()[0].get_geometry_manager()
    chart, swap, zs, angs, areas = gm.fluxmap_grid(B)
    dev = {'chart': DeviceScene(cs, ctx), 'xy': DeviceScene(cs, ctx), 'host': DeviceScene(cs_c, ctx)}
    dev['chart'].set_fluxmap(0, zs, angs, chart=chart)
    dev['xy'].set_fluxmap(0, N.linspace(-1., 1., B + 1), N.linspace(-1., 1., B + 1))
    dev['host'].set_hit_capacity(2 * n + 65536)
    surf_c = cs_c.surfaces[0]
    runs = dict((k, []) for k in dev)
    flux = {}
    for rep in range(4):
        for name in ('chart', 'xy', 'host'):
            d = dev[name]
            d.reset_tallies()
            if name == 'host':
                d.lib.trc_scene_clear_hits(d.handle)
            b = source(n, T, 9)
            t0 = time.time()
            st, _ = d.trace_fast(b, 20, 1e-10, 9)
            if name == 'host':
                hits = d.get_hits()
                t1 = time.time()
                k = N.asarray(hits['surf']) == 0
                flux[name] = gm.get_fluxmap(N.asarray(hits['e_abs'])[k], surf_c.global_to_local(N.asarray(hits['points'])[:, k]), B)
                n_hits = int(k.sum())
            else:
                m = d.get_fluxmap(0)
                t1 = time.time()
                flux[name] = N.hstack(m / areas)
                n_hits = int(d.get_tallies()[2][0])
            wall = (time.time() - t0) * 1e3
            if rep == 0:
                continue            # (warm-up: footprint map, workspace, hit buffer)
            run = {'kernel_ms': st.kernel_ms, 'trace_and_read_ms': (t1 - t0) * 1e3, 'wall_ms': wall, 'segments': int(st.segments),
                   'receiver_hits': n_hits, 'launches': int(st.launches)}
            runs[name].append(run)
            print('%-6s run %d: kernel %.2f ms, trace + read-back %.1f ms, with the host histogram %.1f ms, %d segments, %d hits on the receiver, %d launches'
                  % (name, rep, st.kernel_ms, run['trace_and_read_ms'], wall, run['segments'], n_hits, run['launches']), flush=True)
    worst = float(N.abs(flux['chart'] - flux['host']).max() / flux['host'].max())
    print('chart map against the host route: largest difference %.3g of the largest bin, %.0f %% of %d bins filled'
          % (worst, 100. * (flux['host'] > 0).mean(), flux['host'].size), flush=True)
    for d in dev.values():
        d.close()
    out = {'rays': n, 'bins': B, 'device': ctx.device_name(), 'runs': runs, 'chart_vs_host': worst}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
