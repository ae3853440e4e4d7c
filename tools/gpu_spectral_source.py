"""
The spectral cavity (BASELINE configs[4]: scenes.dish_cavity(), 1.25e8 rays, reps 12) traced two ways through the streaming
form of the fast engine, alternating, three runs each:
  (a) as bench.py other_configs does it: the Buie rays materialised on the host with wavelengths uniform in 0.3-2.5 um from
      numpy, handed over as host arrays;
  (b) the same Buie descriptor with SourceSpectrum.uniform(0.3e-6, 2.5e-6): the wavelengths are drawn on the device;
  (c) as (b) with a 4000-point table (Planck at 5777 K over 0.3-4.3 um, 1 nm): what the table search costs per hit.
Prints kernel_ms (HIP events of the call, source generation included in (b)) and wall_ms of each run, and the absorbed share
of the incoming energy of both with its Monte-Carlo spread.  One JSON object on the last line.
    python tools/gpu_spectral_source.py [--rays N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as N

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=125000000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from tracer_amd import _cabi, scenes
    from tracer_amd.scene import DeviceScene
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.source_spectrum import SourceSpectrum
    ctx = _cabi.get_context(0)
    ts, src = scenes.dish_cavity()
    n = args.rays
    spec = SourceSpectrum.uniform(0.3e-6, 2.5e-6)
    b0 = scenes.dish_source(n, src, seed=9)
    v, d, e = N.asarray(b0.get_vertices()), N.asarray(b0.get_directions()), N.asarray(b0.get_energy())
    wl = N.random.default_rng(4).uniform(0.3e-6, 2.5e-6, n)
    e_in = float(e.sum())
    dev = DeviceScene(ts, ctx)
    spec_c = SourceSpectrum.planck(5777., (0.3e-6, 4.3e-6), step=1e-9)
    runs = {'a': [], 'b': [], 'c': []}
    shares = {}
    for r in range(3):
        for way in ('a', 'b', 'c'):
            dev.reset_tallies()
            if way == 'a':
                bundle = RayBundle(vertices=v, directions=d, energy=e, wavelengths=wl)
            else:
                bundle = scenes.dish_source(n, src, seed=9, spectrum=spec if way == 'b' else spec_c)
            t0 = time.time()
            st, _ = dev.trace_fast(bundle, 12, 1e-3 * e[0], 31, stream=True)
            wall = (time.time() - t0) * 1e3
            a, rcv, h = dev.get_tallies()
            runs[way].append({'kernel_ms': st.kernel_ms, 'wall_ms': wall, 'segments': int(st.segments)})
            shares[way] = float(a.sum() / e_in)
            print('%s run %d: kernel %.1f ms, wall %.1f ms, absorbed share %.6f' % (way, r, st.kernel_ms, wall, shares[way]), flush=True)
    dev.close()
    # spread of the absorbed share: each ray ends absorbed with its energy or not, to a first approximation a Bernoulli draw
    sigma = float(N.sqrt(shares['a'] * (1. - shares['a']) / n))
    out = {'rays': n, 'reps': 12, 'device': ctx.device_name(),
           'a_host_arrays': runs['a'], 'b_device_spectrum': runs['b'], 'c_device_table_%d_points' % spec_c.wavelengths.size: runs['c'],
           'absorbed_share': shares, 'share_sigma_each': sigma,
           'share_diff_in_sigma': abs(shares['a'] - shares['b']) / (sigma * N.sqrt(2.))}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
