"""
Generate tests/golden/sunshape.npz by running the REAL reference's tabulated sunshape sampler
(tracer/sources.py:386-410, sunshape_to_ray_directions).

Run in the build container only (the reference never travels):
    python tests/golden/make_golden_sunshape.py
It imports the reference unmodified, as make_golden.py does (a stub stands in for the absent `shapely`).  For each table the file
holds the points, the uniforms the reference drew from numpy's global generator under a fixed seed (all polar uniforms
`R_thetas`, then all azimuths `phis`), the directions it returned and the CDF it built.  Re-running writes the same file.
"""
import os
import sys

import numpy as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

N_SAMPLES = 1500
THETA_DNI = 4.65e-3
THETA_TOT = 43.6e-3


def buie_disc(theta):
    """the Buie disc profile of sources.py:341 (theta in rad)"""
    return N.cos(0.326 * theta * 1e3) / N.cos(0.308 * theta * 1e3)


def equal_g_intensity(a0, i0, a1):
    """an intensity at a1 whose g = I cos sin equals that of (a0, i0) exactly in float64 (the reference's A == B branch)"""
    g0 = i0 * N.cos(a0) * N.sin(a0)
    i1 = g0 / (N.cos(a1) * N.sin(a1))
    for _ in range(64):
        g1 = i1 * N.cos(a1) * N.sin(a1)
        if g1 == g0:
            return i1
        i1 = N.nextafter(i1, N.inf if g1 < g0 else -N.inf)
    raise RuntimeError('no intensity with an equal g')


def tables():
    out = {}
    th = N.linspace(0., THETA_DNI, 211)
    out['buie0'] = (th, buie_disc(th))
    # a Buie-shaped profile with a CSR-0.05 aureole (Buie et al. 2003: phi = exp(kappa) theta^gamma beyond theta_dni, theta in
    # mrad), out to 43.6 mrad at 0.1 mrad steps
    csr = 0.05
    kappa = 0.9 * N.log(13.5 * csr) * csr ** (-0.3)
    gamma = 2.2 * N.log(0.52 * csr) * csr ** 0.43 - 0.1
    th = N.arange(437) * 1e-4
    with N.errstate(divide='ignore'):
        out['buie05'] = (th, N.where(th <= THETA_DNI, buie_disc(th), N.exp(kappa) * (th * 1e3) ** gamma))
    out['pillbox'] = (N.array([0., THETA_DNI]), N.array([1., 1.]))
    # zero-intensity stretches ([2, 4] mrad, [9, 10] mrad) and two intervals of equal g
    a = N.array([0., 1., 2., 3., 4., 5., 6., 7., 9., 10., 12.]) * 1e-3
    I = N.array([0.5, 1., 0., 0., 0., 0.8, 0., 0.6, 0., 0., 0.3])
    I[6] = equal_g_intensity(a[5], I[5], a[6])
    I[10] = 0.3
    I[9] = equal_g_intensity(a[10], I[10], a[9])
    out['irregular'] = (a, I)
    out['coarse'] = (N.array([0., 2., 5., 9., 15.]) * 1e-3, N.array([1., 0.9, 0.5, 0.1, 0.02]))
    return out


def main():
    import_reference()
    from tracer import sources
    tabs = tables()
    data = {'names': N.array(sorted(tabs))}
    for k, name in enumerate(sorted(tabs)):
        angles, intensity = tabs[name]
        N.random.seed(2000 + k)
        R = N.random.uniform(size=N_SAMPLES)
        phis = N.random.uniform(high=2. * N.pi, size=N_SAMPLES)
        N.random.seed(2000 + k)
        with N.errstate(divide='ignore', invalid='ignore'):
            d = sources.sunshape_to_ray_directions(angles, intensity, N_SAMPLES)
        g = intensity * N.cos(angles) * N.sin(angles)
        integ = 0.5 * (g[:-1] + g[1:]) * (angles[1:] - angles[:-1])
        data[name + '_angles'] = angles
        data[name + '_intensity'] = intensity
        data[name + '_R'] = R
        data[name + '_phi'] = phis
        data[name + '_dir'] = d
        data[name + '_cdf'] = N.add.accumulate(N.hstack(([0.], integ / N.sum(integ))))
    N.savez_compressed(os.path.join(HERE, 'sunshape.npz'), **data)
    print('wrote', os.path.join(HERE, 'sunshape.npz'))


if __name__ == '__main__':
    main()
