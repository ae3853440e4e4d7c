"""
Tabulated sunshapes against the Buie sources on NSTTF (scenes.nsttf_field(), the bench workload without its Kd-tree and flux map),
through the streaming form of the fast engine, alternating, three runs each:
  buie0   buie_sunshape(CSR=0)                    table0   tabulated_sunshape with the 211 Buie CSR-0 nodes as its table
  buie01  buie_sunshape(CSR=0.01)                 table05  tabulated_sunshape with a 437-point Buie-shaped table (CSR-0.05
                                                           aureole out to 43.6 mrad, tests/golden/sunshape.npz)
Prints per run the kernel time of the call (HIP events), its wall time, segments and Mray-bounces/s (segments / kernel time), and
per source the core angle, u_c and the share of rays the general path takes (1 - u_c for a table, the aureole for Buie).
One JSON object on the last line.
    python tools/gpu_sunshape.py [--rays N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=100000000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from tracer_amd import _cabi, scenes, sources
    from tracer_amd.scene import DeviceScene, compile_scene
    ctx = _cabi.get_context(0)
    plant, field, rec, src = scenes.nsttf_field()
    dev = DeviceScene(compile_scene(plant), ctx)
    gold = N.load(os.path.join(ROOT, 'tests', 'golden', 'sunshape.npz'))
    n = args.rays
    c, d, r, f = src['center'], src['direction'], src['radius'], src['flux']
    th0 = N.linspace(0., 4.65e-3, 211)
    I0 = N.cos(0.326 * th0 * 1e3) / N.cos(0.308 * th0 * 1e3)
    make = {
        'buie0': lambda: sources.buie_sunshape(n, c, d, r, 0., flux=f, seed=9),
        'table0': lambda: sources.tabulated_sunshape(n, c, d, r, th0, I0, flux=f, seed=9),
        'buie01': lambda: sources.buie_sunshape(n, c, d, r, 0.01, flux=f, seed=9),
        'table05': lambda: sources.tabulated_sunshape(n, c, d, r, gold['buie05_angles'], gold['buie05_intensity'], flux=f, seed=9),
    }
    general = {}
    for name, mk in make.items():
        b = mk()
        if b._src_table is not None:
            _, _, _, tc, uc = b._src_table.packed()
            general[name] = {'theta_c': tc, 'u_c': uc, 'general_share': 1. - uc}
        else:
            cdf_end = b.source_args()[0].buie[2 * 211 + 210]
            general[name] = {'cdf_end': cdf_end, 'general_share': max(0., 1. - cdf_end)}
        print(name, general[name], flush=True)
    runs = dict((k, []) for k in make)
    e0 = make['buie0']().source_args()[0].energy
    for rep in range(4):
        for name, mk in make.items():
            dev.reset_tallies()
            b = mk()
            t0 = time.time()
            st, _ = dev.trace_fast(b, 100, 1e-10 * e0, 9, stream=True)
            wall = (time.time() - t0) * 1e3
            a, rcv, h = dev.get_tallies()
            if rep == 0:
                continue            # (warm-up: footprint map, workspace)
            run = {'kernel_ms': st.kernel_ms, 'wall_ms': wall, 'segments': int(st.segments),
                   'mray_bounces_per_s': st.segments / (st.kernel_ms * 1e-3) / 1e6, 'receiver': float(a[-1])}
            runs[name].append(run)
            print('%-8s run %d: kernel %.1f ms, wall %.1f ms, %d segments, %.0f Mray-bounces/s, receiver %.1f'
                  % (name, rep, st.kernel_ms, wall, run['segments'], run['mray_bounces_per_s'], run['receiver']), flush=True)
    dev.close()
    out = {'rays': n, 'device': ctx.device_name(), 'general': general, 'runs': runs}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
