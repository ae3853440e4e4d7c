"""
Generate tests/golden/source_spectra.npz by running the REAL reference's piecewise-linear sampler
(ray_trace_utils/sampling.py:6-52, PW_linear_distribution) and Planck's law (ray_trace_utils/electromagnetics.py:3-14).

Run in the build container only (the reference never travels):
    python tests/golden/make_golden_spectra.py
It imports the reference unmodified, as make_golden.py does (a stub stands in for the absent `shapely`).  The tables are
given in micrometres with at most 8 decimals, so that the reference's N.round(xs, decimals=8) leaves them as they are: the
sampler does not depend on the unit.  For each table the file holds the points, the uniforms the reference drew (its global
generator, seeded) and the wavelengths PW_linear_distribution.sample returned for them.  Re-running writes the same file.
"""
import os
import sys

import numpy as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

N_SAMPLES = 2000
PLANCK_T = 5777.
PLANCK_BAND = (0.3e-6, 3.0e-6)      # m
PLANCK_STEP = 2e-9                  # m: linspace(lo, hi, int((hi - lo) / step)) as tracer/sources.py:788 builds its grid


def r8(a):
    a = N.round(N.asarray(a, dtype=float), 8)
    assert N.array_equal(N.round(a, 8), a)
    return a


def tables(electromagnetics):
    out = {}
    out['flat'] = (r8([0.4, 0.7]), r8([1., 1.]))
    out['ramp'] = (r8([0.3, 1.2, 2.5]), r8([0.25, 2., 0.5]))
    # zero density at both ends of [0.6, 0.9] and of [2.0, 2.2]; zero at the first point
    out['irregular'] = (r8([0.3, 0.45, 0.6, 0.9, 1.05, 1.3, 1.55, 2.0, 2.2, 2.4]),
                        r8([0., 1.5, 0., 0., 0.8, 0.8, 2.4, 0., 0., 0.6]))
    wls = N.linspace(PLANCK_BAND[0], PLANCK_BAND[1], int((PLANCK_BAND[1] - PLANCK_BAND[0]) / PLANCK_STEP))
    p = electromagnetics.Planck(wls, PLANCK_T)
    out['planck'] = (r8(wls * 1e6), r8(p / p.max()))
    return out, wls, p


def main():
    import_reference()
    from ray_trace_utils import sampling, electromagnetics
    tabs, planck_wl, planck_val = tables(electromagnetics)
    data = {'names': N.array(sorted(tabs)), 'planck_T': N.array(PLANCK_T), 'planck_band': N.array(PLANCK_BAND),
            'planck_step': N.array(PLANCK_STEP), 'planck_wl': planck_wl, 'planck_val': planck_val}
    for k, name in enumerate(sorted(tabs)):
        xs, ys = tabs[name]
        dist = sampling.PW_linear_distribution(xs, ys)
        N.random.seed(1000 + k)
        u = N.random.uniform(size=N_SAMPLES)
        N.random.seed(1000 + k)
        x, _ = dist.sample(N_SAMPLES)
        data[name + '_xs'] = xs
        data[name + '_ys'] = ys
        data[name + '_u'] = u
        data[name + '_x'] = x
        data[name + '_a'] = dist.a / (2. * dist.tot_integ)     # the quadratic's coefficients the reference solves, per interval
        data[name + '_b'] = dist.b / dist.tot_integ
        data[name + '_cdf'] = dist.CDF_def
    N.savez_compressed(os.path.join(HERE, 'source_spectra.npz'), **data)
    print('wrote', os.path.join(HERE, 'source_spectra.npz'))


if __name__ == '__main__':
    main()
