"""
The 50 x 50 map of the NSTTF receiver from the captured hits, two ways, on the hits of the same call:
  device  TracerEngine.histogram_hits: the hits binned where they lie (k_hist_hits), 20 KB come back
  host    the receiver's get_all_hits() -- the hits packed on the device and copied to page-locked host arrays -- then
          Surface.global_to_local and numpy.histogram2d: the route of the reference's example
Five repetitions after a warm-up, one ray_tracer(tree=False) call each; the two ways alternate in order from one repetition to the
next.  Prints per repetition the wall times, the time of k_hist_hits alone between two device events, and the bytes the kernel reads
-- entries reserved x (4 + 8 per column read: x, y, z and the absorbed energy) -- against the 8 TB/s of the memory; then medians and
spread (min .. max), and whether the device way is below the hit read alone.  One JSON object on the last line.
    python tools/gpu_hit_histogram.py [--rays N] [--reps R] [--out FILE]
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
RECEIVER = 218


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=float, default=1e8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from tracer_amd import _cabi, scenes
    from tracer_amd.tracer_engine import TracerEngine
    ctx = _cabi.get_context(0)
    n = int(args.rays)
    plant, field, rec, src = scenes.nsttf_field()
    ue, ve = scenes.nsttf_fluxmap_edges()
    plate = plant.get_surfaces()[RECEIVER]
    rec_opt = plate.get_optics_manager()
    eng = TracerEngine(plant)
    runs = []
    worst = 0.
    for rep in range(args.reps + 1):
        b = scenes.nsttf_source(n, src, seed=2024, ray_offset=rep * n)
        t0 = time.time()
        eng.ray_tracer(b, reps=100, min_energy=1e-10, tree=False, accel=True, seed=2024)
        ctx.synchronize()
        trace_ms = (time.time() - t0) * 1e3
        entries = eng._dev.hits_reserved()[0]
        run = {'trace_ms': trace_ms, 'entries': int(entries)}

        def device():
            t = time.time()
            H = eng.histogram_hits(plate, ue, ve)
            run['device_ms'] = (time.time() - t) * 1e3
            run['kernel_ms'] = eng._dev.histogram_hits_ms()
            return H

        def host():
            t = time.time()
            e_abs, pts = rec_opt.get_all_hits()[:2]
            run['read_ms'] = (time.time() - t) * 1e3
            local = plate.global_to_local(pts)
            H = N.histogram2d(local[0], local[1], bins=[ue, ve], weights=e_abs)[0]
            run['host_ms'] = (time.time() - t) * 1e3
            run['hits'] = int(len(e_abs))
            return H
        Hd, Hh = (device(), host()) if rep % 2 else (host(), device())[::-1]
        plant.reset_all_optics()
        worst = max(worst, float(N.abs(Hd - Hh).max() / Hh.max()))
        run['bytes'] = int(entries) * (4 + 8 * 4)
        run['tb_per_s'] = run['bytes'] / (run['kernel_ms'] * 1e-3) / 1e12 if run['kernel_ms'] > 0 else 0.
        if rep == 0:
            continue            # (warm-up: footprint map, workspace, hit buffer, page-locked blocks)
        run['first'] = 'device' if rep % 2 else 'host'
        runs.append(run)
        print('rep %d (%s first): trace %.1f ms, %d hits in %d entries; device histogram %.3f ms (kernel %.3f ms, %.1f MB, %.2f TB/s = %.0f %% of '
              '%.0f); hit read alone %.2f ms, read + global_to_local + histogram2d %.1f ms'
              % (rep, run['first'], trace_ms, run['hits'], entries, run['device_ms'], run['kernel_ms'], run['bytes'] / 1e6, run['tb_per_s'],
                 100. * run['tb_per_s'] / PEAK_TBS, PEAK_TBS, run['read_ms'], run['host_ms']), flush=True)
    med = {}
    for k in ('device_ms', 'kernel_ms', 'read_ms', 'host_ms', 'trace_ms', 'tb_per_s'):
        v = N.array([r[k] for r in runs])
        med[k] = {'median': float(N.median(v)), 'min': float(v.min()), 'max': float(v.max())}
        print('%-10s median %.3f (%.3f .. %.3f)' % (k, med[k]['median'], med[k]['min'], med[k]['max']))
    print('device map against the host route: largest difference %.3g of the largest bin' % worst)
    earned = med['device_ms']['median'] < med['read_ms']['median']
    print('the device histogram (%.3f ms) is %s the hit read alone (%.3f ms): %.1f x; against the whole host route (%.1f ms): %.0f x'
          % (med['device_ms']['median'], 'BELOW' if earned else 'NOT below', med['read_ms']['median'],
             med['read_ms']['median'] / med['device_ms']['median'], med['host_ms']['median'], med['host_ms']['median'] / med['device_ms']['median']))
    out = {'rays': n, 'reps': args.reps, 'device': ctx.device_name(), 'runs': runs, 'medians': med, 'device_vs_host': worst,
           'device_below_hit_read': bool(earned)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
