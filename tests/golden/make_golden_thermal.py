"""
Generate tests/golden/thermal_sources.npz by running the REAL reference's thermal source (tracer/sources.py:
spectral_band_axisymmetrical_thermal_emission_source), its shape samplers (ray_trace_utils/sampling.py: disk_sampling,
triangle_sampling, cylinder_sampling, frustum_sampling, sphere_sampling -- rectangle_sampling raises NameError there and is not
run) and its weighted sampler of the polar angle (PW_lincossin_distribution).

Run in the build container only (the reference never travels):
    python tests/golden/make_golden_thermal.py
It imports the reference unmodified, as make_golden.py does (a stub stands in for the absent `shapely`).  For each case and seed the
file holds the uniforms numpy's global generator handed the reference (drawn again from the same seed, in the reference's order) and
the arrays the reference returned.  The tables are rounded to 8 decimals beforehand, so that the reference's own rounding
(sampling.py:9-10) changes nothing.  Re-running writes the same file.

The tables (TABLES): `dir` a dip and a zero at pi/2, `gray` a constant on 5 points, `gray2` the same on 2 points (no reference output:
the reference's weights are NaN there, both nodes of its proposal being <= 0 after its rounding), `cone` a table that ends at 0.6,
`gap` a stretch without mass, `steep` an emittance that starts from 0 (a cubic start of the CDF).
"""
import os
import sys

import numpy as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

NS = 128      # per case, as lamp_sources.npz: a row of 128 float64 draws is 1 KB that does not compress
SEEDS = (5200, 5201)
T_WALL, BAND, REF_INDEX = 1100., (1.0e-6, 2.5e-6), 1.3
R_DISK = 0.25
HIST_SEED, HIST_N, HIST_BINS = 11, 4000000, 24
REFERENCE_TABLES = ('dir', 'gray', 'cone', 'gap', 'steep')
SHAPES = {      # the reference samplers' arguments
    'disk': dict(r_ext=R_DISK),
    'triangle': dict(A=N.array([0.1, -0.2, 0.]), B=N.array([0.7, 0.1, 0.]), C=N.array([0.3, 0.6, 0.])),
    'cylinder': dict(r_ext=0.2, h=0.7),
    'frustum_wide': dict(r0=0.1, r1=0.3, z0=0., z1=0.5, angular_span=[0.3, 2.1]),
    'frustum_narrow': dict(r0=0.4, r1=0.15, z0=0.2, z1=0.6, angular_span=[1., 5.]),
    'sphere': dict(r_ext=0.3),
}


def tables():
    th = N.round(N.linspace(0., N.pi / 2., 10), 8)
    eps = N.round(0.9 * N.cos(th) ** 0.3 * (1. - 0.5 * N.exp(-((th - 1.2) / 0.2) ** 2)), 8)
    eps[-1] = 0.
    return {'dir': (th, eps),
            'gray': (N.round(N.linspace(0., N.pi / 2., 5), 8), N.full(5, 0.8)),
            'gray2': (N.round(N.array([0., N.pi / 2.]), 8), N.array([0.8, 0.8])),
            'cone': (N.round(N.array([0., 0.3, 0.6]), 8), N.array([1., 1., 0.5])),
            'gap': (N.round(N.array([0., 0.3, 0.5, 0.9, 1.2, 1.5]), 8), N.array([0.6, 0.9, 0., 0., 0.7, 0.2])),
            'steep': (N.round(N.array([0., 0.4, 1.0, 1.5]), 8), N.array([0., 1., 0.3, 0.]))}


def uniforms(seed, count):
    """`count` blocks of NS uniforms in the order numpy hands them out from `seed`"""
    N.random.seed(seed)
    return N.array([N.random.uniform(size=NS) for _ in range(count)])


def main():
    import_reference()
    import warnings
    warnings.simplefilter('ignore')
    from ray_trace_utils import sampling
    from ray_trace_utils.electromagnetics import Planck
    from tracer import sources
    data = {'seeds': N.array(SEEDS), 'ns': N.array(NS), 'T': N.array(T_WALL), 'band': N.array(BAND), 'ref_index': N.array(REF_INDEX),
            'r_disk': N.array(R_DISK), 'hist_n': N.array(HIST_N)}
    for name, (xs, ys) in sorted(tables().items()):
        data[name + '_xs'], data[name + '_ys'] = xs, ys
    for name, kw in sorted(SHAPES.items()):
        for k, v in sorted(kw.items()):
            data['shape_%s_%s' % (name, k)] = N.asarray(v, dtype=float)
    # the band: L_band and wl_avg as the reference's function computes them inside (sources.py:788-790, :808), with its Planck
    wls = N.linspace(BAND[0], BAND[1], int((BAND[1] - BAND[0]) / 1e-9))
    B = Planck(wls, T_WALL)
    data['L_band'] = N.trapezoid(B, wls)
    data['wl_avg'] = N.sum(wls * B) / N.sum(B)
    for seed in SEEDS:
        k = '%d_' % seed
        # the uniforms of the shape samplers: every one of them starts from `seed` and draws two rows (u0 its first, u1 its second:
        # disc ths, rs; triangle r1, r2; cylinder zs, ths; frustum R, phi; sphere phis, cosths)
        data[k + 'u'] = uniforms(seed, 2)
        for name, kw in sorted(SHAPES.items()):
            fn = getattr(sampling, name.split('_')[0] + '_sampling')
            flag = 'normal_up' if name in ('disk', 'triangle') else 'normal_in'
            for tag, val in (('a', False), ('b', True)):        # both senses: a = the flag False, b = the flag True
                N.random.seed(seed)
                pos, nrm = fn(ns=NS, normals=True, **dict(kw, **{flag: val}))
                if tag == 'a':
                    data[k + name + '_pos'] = pos
                else:
                    assert N.array_equal(pos, data[k + name + '_pos'])      # (the points do not depend on the flag)
                data[k + name + '_n_' + tag] = nrm
        # the thermal source on the disc's points, normals up: its draws are the polar uniforms and the azimuths, from seed + 50
        data[k + 'src_u'] = uniforms(seed + 50, 2)
        pos, nrm = data[k + 'disk_pos'], data[k + 'disk_n_b']
        area = N.pi * R_DISK ** 2
        for name in REFERENCE_TABLES:
            xs, ys = tables()[name]
            N.random.seed(seed + 50)
            rb = sources.spectral_band_axisymmetrical_thermal_emission_source(pos.copy(), nrm.copy(), area, xs, ys, T_WALL, NS, BAND, REF_INDEX)
            e = rb.get_energy()
            assert N.all(N.isfinite(e))
            data[k + name + '_energy'] = e
            data[k + name + '_directions'] = rb.get_directions()
            data[k + name + '_wavelengths'] = rb.get_wavelengths()
            data[k + name + '_ref_index'] = rb.get_ref_index()
            if seed == SEEDS[0]:
                data[name + '_exitance'] = N.trapezoid(ys * data['L_band'] * N.cos(xs) * N.sin(xs), xs) * 2. * N.pi
                assert abs(N.sum(e) / area / data[name + '_exitance'] - 1.) < 1e-12
    # one long run of the reference's weighted sampler per table: sum of weights and of squared weights in 24 bins over the table
    for name in REFERENCE_TABLES:
        xs, ys = tables()[name]
        N.random.seed(HIST_SEED)
        x, w = sampling.PW_lincossin_distribution(xs, ys).sample(HIST_N)
        assert N.all(N.isfinite(w))
        bins = N.linspace(xs[0], xs[-1], HIST_BINS + 1)
        data[name + '_hist_w'] = N.histogram(x, bins, weights=w)[0]
        data[name + '_hist_w2'] = N.histogram(x, bins, weights=w * w)[0]
    path = os.path.join(HERE, 'thermal_sources.npz')
    N.savez_compressed(path, **data)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
