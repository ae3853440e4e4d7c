"""
Arc-lamp sources pending on the device against the same rays sampled on the host and given, through TracerEngine.ray_tracer(tree=False):
  one    one solar-simulator module (Zhu lamp: a sphere and two cylinder emitters) and a target, --rays rays per call
  seven  seven modules (a central one and six around it, every second with a Bader lamp: an arc volume) on one target, --rays rays
         per module per call
For each: `pending` -- the lamps' pending bundles traced one after the other, nothing of the size of a bundle made on the host --
and `given` -- tracer_amd.sampling draws the same distributions with numpy, the arrays are uploaded as a given bundle; its sampling
time (once per scene: it does not depend on the device) is reported apart from its trace.  Alternating, --repeats timed runs each
after one warm-up; per variant the median and the spread (min .. max) of the wall time per set of calls.  Writes profiles/gpu_lamp_sources.txt (or
--out) and one JSON object on the last line.
    python tools/gpu_lamp_sources.py [--rays N] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A, C_ = 0.3, 0.5
F = N.sqrt(C_ ** 2 - A ** 2)
ZLIM = [-C_, -0.35]     # the cap behind the lamp: 16 degrees wide seen from the target, so that modules 37 degrees apart do not overlap


def simulator(n_modules):
    from tracer_amd.models.solar_simulator import SolarSimulator, Target
    cdf = N.array([N.linspace(0., N.pi, 37), 0.5 * (1. - N.cos(N.linspace(0., N.pi, 37)))]).T
    focus2 = N.array([0., 0., 2. * F])
    aims = [N.array([0., 0., 1.])]
    for k in range(n_modules - 1):
        az = 2. * N.pi * k / max(n_modules - 1, 1)
        aims.append(N.array([N.sin(0.7) * N.cos(az), N.sin(0.7) * N.sin(az), N.cos(0.7)]))
    dicts = [dict(a=A, b=A, c=C_, zlim=ZLIM, lampdict=(dict(model='Bader', theta_CDF=cdf) if k % 2 else dict(model='Zhu')))
             for k in range(n_modules)]
    edges = N.linspace(-0.1, 0.1, 41)
    target = Target(0.2, 0.2, focus2, N.array([0., 0., -1.]), edges, edges)
    return SolarSimulator([focus2 - 2. * F * a for a in aims], aims, dicts, [target])


def host_rays(module, n):
    """the module's lamp sampled with tracer_amd.sampling and posed, as the reference's fire_lamp does it on the host"""
    from tracer_amd import sampling
    from tracer_amd.ray_bundle import RayBundle
    lamp = module.lamp
    if hasattr(lamp, 'ths'):
        v = sampling.cylinder_sampling(lamp.r_c, lamp.l_c, n, volume=True)
        th, _ = sampling.PW_linear_distribution(lamp.ths, lamp.ths_PDF).sample(n)
        ph = N.random.uniform(size=n) * 2. * N.pi
        d = N.vstack([N.sin(th) * N.cos(ph), N.sin(th) * N.sin(ph), N.cos(th)])
        e = N.ones(n) * lamp.P / n
    else:
        vs, ds, es = [], [], []
        for share, (r, h) in ((lamp.a_s, (lamp.r_s, None)), (lamp.b_c1, (lamp.r_s, lamp.l_c)), (lamp.g_c2, (lamp.r_c2, lamp.l_c))):
            m = int(n * share)
            if h is None:
                p, nr = sampling.sphere_sampling(r, m, normals=True)
                p[2] -= lamp.l_c / 2. - lamp.r_s
            else:
                p, nr = sampling.cylinder_sampling(r, h, m, normals=True)
            vs.append(p)
            ds.append(sampling.isotropic_directions_sampling(m, N.pi / 2., normals=nr))
            es.append(N.ones(m) * lamp.P * share / m)
        v, d, e = N.hstack(vs), N.hstack(ds), N.hstack(es)
    return RayBundle(vertices=N.dot(module.rotation, v) + module.location[:, None], directions=N.dot(module.rotation, d), energy=e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=1000000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gpu_lamp_sources.txt'))
    args = ap.parse_args()
    from tracer_amd import _cabi
    from tracer_amd.tracer_engine import TracerEngine
    ctx = _cabi.get_context(0)
    n = args.rays
    lines = ['arc-lamp sources, %d rays per module per call, ray_tracer(tree=False), %s' % (n, ctx.device_name()),
             'wall time per set of calls (one call per pending bundle / one given bundle per module), results left on the device;',
             'median (min .. max) of %d runs after one warm-up, variants alternating' % args.repeats, '']
    out = {'rays': n, 'device': ctx.device_name(), 'repeats': args.repeats, 'runs': {}}
    for name, n_mod in (('one', 1), ('seven', 7)):
        sim = simulator(n_mod)
        eng = TracerEngine(sim)
        ti = sim.get_surfaces().index(sim.targets[0].get_surfaces()[0])
        n_pending = 0
        t = dict(pending=[], given=[], sample=[])
        power = {}
        # the host samples once (its time does not depend on the device, and at a million rays the per-ray rotation of the
        # directions to their normals takes many seconds); every repeat traces these arrays again
        N.random.seed(50)
        t0 = time.perf_counter()
        bundles = [host_rays(m, n) for m in sim.modules]
        t['sample'].append((time.perf_counter() - t0) * 1e3)
        for rep in range(args.repeats + 1):
            for variant in ('pending', 'given'):
                eng.reset_tallies()
                if variant == 'pending':
                    t0 = time.perf_counter()
                    n_pending = 0
                    for k, m in enumerate(sim.modules):
                        for b in m.lamp_sources(n, seed=50 + 10 * rep + k):
                            eng.ray_tracer(b, tree=False)
                            n_pending += 1
                    absorbed = eng.get_tallies()[0]         # (waits for the device)
                    dt = time.perf_counter() - t0
                else:
                    t0 = time.perf_counter()
                    for b in bundles:
                        eng.ray_tracer(b, tree=False)
                    absorbed = eng.get_tallies()[0]
                    dt = time.perf_counter() - t0
                power[variant] = float(absorbed[ti])
                if rep == 0:
                    continue
                t[variant].append(dt * 1e3)
        med = lambda x: float(N.median(x))
        fmt = lambda x: '%9.2f ms (%.2f .. %.2f)' % (med(x), min(x), max(x))
        lines += ['%s module%s:' % (name, '' if n_mod == 1 else 's'),
                  '  pending sources        %s   %d calls, target power %.1f W' % (fmt(t['pending']), n_pending, power['pending']),
                  '  given, trace alone     %s   target power %.1f W' % (fmt(t['given']), power['given']),
                  '  given, host sampling   %9.2f ms (once)' % t['sample'][0],
                  '  given, both            %9.2f ms: %.1f x the pending sources' % (med(t['given']) + med(t['sample']), (med(t['given']) + med(t['sample'])) / med(t['pending'])), '']
        out['runs'][name] = dict((k, v) for k, v in t.items())
        out['runs'][name]['target_power'] = power
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
