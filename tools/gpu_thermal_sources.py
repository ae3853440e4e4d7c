"""
What the exact sampler of a thermal emitter costs on the device: a pending disc source under a receiver plate inside an absorbing
sphere, through TracerEngine.ray_tracer(tree=False), with
  newton   the emittance table `dir` of the tests (10 points, a dip and a zero at pi/2): the safeguarded Newton iteration per ray
  closed   a constant table on 2 points: the closed form of the Lambertian law, no iteration
  lamp     cylinder_emitter_bundle(law='lambertian') of the arc-lamp kinds, for scale: a closed-form law without a table
  given    the `newton` rays materialised once and traced as a given bundle of host arrays (its time includes their upload)
at --rays rays per call: below 2^20 the megakernel runs (k_lamp_coop), from 2^20 the streaming form (k_s_gen_emit / k_s_gen_lamp).
Alternating, --repeats timed runs each after one warm-up; median and spread (min .. max) of the wall time per call, results left on
the device.  Writes profiles/gpu_thermal_sources.txt (or --out) and one JSON object on the last line.
    python tools/gpu_thermal_sources.py [--rays N [N ...]] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene():
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.sphere_surface import SphericalGM
    from tracer_amd.optics_callables import Reflective
    from tracer_amd.spatial_geometry import rotx
    receiver = AssembledObject(surfs=[Surface(geometry=RectPlateGM(0.5, 0.5), optics=Reflective(1.))], location=N.array([0., 0., 0.5]),
                               rotation=rotx(N.pi)[:3, :3])
    shell = AssembledObject(surfs=[Surface(geometry=SphericalGM(radius=3.), optics=Reflective(1.))])
    return Assembly(objects=[receiver, shell])


def tables():
    th = N.round(N.linspace(0., N.pi / 2., 10), 8)
    eps = N.round(0.9 * N.clip(N.cos(th), 0., None) ** 0.3 * (1. - 0.5 * N.exp(-((th - 1.2) / 0.2) ** 2)), 8)
    eps[-1] = 0.
    return {'newton': (th, eps), 'closed': (N.array([0., N.pi / 2.]), N.array([0.8, 0.8]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, nargs='+', default=[1000000, 1 << 22])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gpu_thermal_sources.txt'))
    args = ap.parse_args()
    from tracer_amd import _cabi, sources
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.tracer_engine import TracerEngine
    ctx = _cabi.get_context(0)
    device = ctx.device_name().strip()
    eng = TracerEngine(scene())
    zero, up = N.zeros(3), N.array([0., 0., 1.])
    disc = {'type': 'disk', 'kwargs': {'r_ext': 0.25}}

    def make(variant, n, seed):
        if variant == 'lamp':
            return sources.cylinder_emitter_bundle(n, 0.05, 0.2, zero.reshape(3, 1), up, 100., seed=seed)
        th, eps = tables()['newton' if variant == 'given' else variant]
        return sources.thermal_emitter_bundle(n, disc, th, eps, 1100., (1e-6, 2.5e-6), zero, up, spectrum=None, seed=seed)

    lines = ['thermal emitters, ray_tracer(tree=False), %s' % device,
             'wall time per call, results left on the device; median (min .. max) of %d runs after one warm-up, variants alternating' % args.repeats, '']
    out = {'device': device, 'repeats': args.repeats, 'runs': {}}
    variants = ('newton', 'closed', 'lamp', 'given')
    for n in args.rays:
        t = dict((v, []) for v in variants)
        share = {}
        m = make('given', n, 50)
        given = RayBundle(vertices=m.get_vertices(), directions=m.get_directions(), energy=m.get_energy())
        for rep in range(args.repeats + 1):
            for v in variants:
                eng.reset_tallies()
                b = given if v == 'given' else make(v, n, 50)
                t0 = time.perf_counter()
                eng.ray_tracer(b, tree=False)
                absorbed = eng.get_tallies()[0]         # (waits for the device)
                dt = time.perf_counter() - t0
                share[v] = float(absorbed[0] / absorbed.sum())
                if rep:
                    t[v].append(dt * 1e3)
        fmt = lambda x: '%9.3f ms (%.3f .. %.3f)' % (float(N.median(x)), min(x), max(x))
        lines += ['%d rays per call (%s):' % (n, 'the streaming form' if n >= 1 << 20 else 'the megakernel')]
        lines += ['  %-7s %s   share of the power on the receiver %.4f' % (v, fmt(t[v]), share[v]) for v in variants] + ['']
        out['runs'][str(n)] = dict(t, share=share)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
