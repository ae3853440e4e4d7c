"""
Generate tests/golden/fluxmap_charts.npz by running the REAL reference's get_fluxmap of every receiver shape that has one:
RectPlateGM (flat_surface.py:237-251), RoundPlateGM with and without Ri (:524-545), FiniteCylinder with a full and a partial
ang_range (cylinder.py:139-159), ParabolicDishGM (paraboloid.py:151-172) and SphericalGM (sphere_surface.py:100-115).

Run in the build container only (the reference never travels):
    python tests/golden/make_golden_fluxmaps.py
It imports the reference unmodified, as make_golden.py does.  For each case the file holds the constructor arguments, the random
local coordinates (on the shape, 3 x n) and energies that went in, and the array the reference returned at two resolutions.
Re-running writes the same file.
"""
import os
import sys

import numpy as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

N_HITS = 60
RESOLUTIONS = (4, 9)

# name -> (module, class, constructor arguments)
CASES = {'rect': ('flat_surface', 'RectPlateGM', (3., 2.)),
         'round': ('flat_surface', 'RoundPlateGM', (1.7,)),
         'round_ri': ('flat_surface', 'RoundPlateGM', (1.7, 0.6)),
         'cylinder': ('cylinder', 'FiniteCylinder', (1.2, 1.4)),
         'cylinder_part': ('cylinder', 'FiniteCylinder', (1.2, 1.4, (0.4, 3.9))),
         'dish': ('paraboloid', 'ParabolicDishGM', (1.6, 1.)),
         'sphere': ('sphere_surface', 'SphericalGM', (0.5,))}


def local_points(name, args, rng):
    """random points of the shape in its own frame (3, N_HITS)"""
    n = N_HITS
    if name == 'rect':
        return N.vstack((rng.uniform(-args[0] / 2., args[0] / 2., n), rng.uniform(-args[1] / 2., args[1] / 2., n), N.zeros(n)))
    if name.startswith('round'):
        r = N.sqrt(rng.uniform((args[1] if len(args) > 1 else 0.) ** 2, args[0] ** 2, n))
        a = rng.uniform(-N.pi, N.pi, n)
        return N.vstack((r * N.cos(a), r * N.sin(a), N.zeros(n)))
    if name.startswith('cylinder'):
        lo, hi = args[2] if len(args) > 2 else (0., 2. * N.pi)
        a = rng.uniform(lo, hi, n)
        return N.vstack((args[0] / 2. * N.cos(a), args[0] / 2. * N.sin(a), rng.uniform(-args[1] / 2., args[1] / 2., n)))
    if name == 'dish':
        r = args[0] / 2. * N.sqrt(rng.uniform(0., 1., n))
        a = rng.uniform(-N.pi, N.pi, n)
        return N.vstack((r * N.cos(a), r * N.sin(a), r ** 2 / (4. * args[1])))
    th = N.arccos(rng.uniform(-1., 1., n))
    a = rng.uniform(-N.pi, N.pi, n)
    return args[0] * N.vstack((N.sin(th) * N.cos(a), N.sin(th) * N.sin(a), N.cos(th)))


def main():
    import_reference()
    import importlib
    out = {'names': N.array(sorted(CASES)), 'resolutions': N.array(RESOLUTIONS)}
    rng = N.random.RandomState(20)
    for name in sorted(CASES):
        module, cls, args = CASES[name]
        gm = getattr(importlib.import_module('tracer.' + module), cls)(*args)
        pts = local_points(name, args, rng)
        e = rng.uniform(0.5, 2., N_HITS)
        out[name + '_points'] = pts
        out[name + '_energy'] = e
        for res in RESOLUTIONS:
            out['%s_flux_%d' % (name, res)] = gm.get_fluxmap(e.copy(), pts.copy(), res)
    N.savez_compressed(os.path.join(HERE, 'fluxmap_charts.npz'), **out)


if __name__ == '__main__':
    main()
