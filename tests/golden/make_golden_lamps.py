"""
Generate tests/golden/lamp_sources.npz by running the REAL reference's host samplers (ray_trace_utils/sampling.py: cylinder_sampling,
sphere_sampling, disk_sampling, Lambertian_directions_sampling, PW_linear_distribution) and its vector helpers.

Run in the build container only (the reference never travels):
    python tests/golden/make_golden_lamps.py
It imports the reference unmodified, as make_golden.py does (a stub stands in for the absent `shapely`).  For each case and seed the
file holds the uniforms numpy's global generator handed the reference (drawn again from the same seed, in the reference's order) and
the arrays the reference returned.  The tables are rounded to 8 decimals beforehand, so that the reference's own rounding
(sampling.py:9-10) changes nothing.  Re-running writes the same file.
"""
import os
import sys

import numpy as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

NS = 128      # per case: a row of 128 float64 draws is 1 KB that does not compress, and the cases below are some forty rows per seed
SEEDS = (4100, 4101)
R_C, L_C, R_S = 7.5e-4, 4.5e-3, 2.5e-4


def tables():
    th = N.round(N.linspace(0., N.pi, 19), 8)
    lobe = N.round(0.05 + N.sin(th) ** 2 * (1. + 0.6 * N.cos(th - 0.7)), 8)     # a lamp's lobe about the equator, skewed
    flat = (N.round(N.array([0., N.pi]), 8), N.array([1., 1.]))
    gap_th = N.round(N.array([0., 0.4, 0.9, 1.3, 1.8, 2.2, 2.7, 3.1]), 8)
    gap = N.array([0.2, 1., 0., 0., 0.7, 1.2, 0.3, 0.])                          # no density between 0.9 and 1.3
    return {'lobe': (th, lobe), 'flat': flat, 'gap': (gap_th, gap)}


def uniforms(seed, count):
    """`count` blocks of NS uniforms in the order numpy hands them out from `seed`"""
    N.random.seed(seed)
    return N.array([N.random.uniform(size=NS) for _ in range(count)])


def main():
    import_reference()
    from ray_trace_utils import sampling, vector_manipulations as vm
    data = {'seeds': N.array(SEEDS), 'ns': N.array(NS), 'dims': N.array([R_C, L_C, R_S])}
    for seed in SEEDS:
        k = '%d_' % seed
        # The uniforms of the position samplers: every one of them starts from `seed`, so one block of three rows serves them all
        # (cylinder volume: zs, ths, rs; wall: zs, ths; sphere: phis, cosths; disc: ths, rs)
        data[k + 'u'] = uniforms(seed, 3)
        N.random.seed(seed)
        data[k + 'vol_pos'] = sampling.cylinder_sampling(R_C, L_C, NS, volume=True)
        normals = {}
        for surf, call in (('wall', lambda inwards: sampling.cylinder_sampling(R_S, L_C, NS, normals=True, normal_in=inwards)),
                           ('sph', lambda inwards: sampling.sphere_sampling(R_S, NS, normals=True, normal_in=inwards))):
            N.random.seed(seed)
            pos, out = call(False)
            N.random.seed(seed)
            pos_in, inw = call(True)
            # (not stored: the inward normals are the outward ones negated, and the positions do not depend on them)
            assert N.array_equal(pos, pos_in) and N.array_equal(inw, -out)
            normals[surf, 'out'], normals[surf, 'in'] = out, inw
            data[k + surf + '_n_out'] = out
            if surf == 'wall':
                data[k + 'wall_pos'] = pos
            else:
                assert N.array_equal(pos, R_S * out)        # (not stored: the sphere's points are its radius times the normals)
        N.random.seed(seed)
        disk = sampling.disk_sampling(R_C, NS)
        assert not disk[2].any()
        data[k + 'disk_xy'] = disk[:2]
        # Lambertian directions about those normals: xi1, xi2 (from seed + 50, so that they differ from the positions' uniforms)
        data[k + 'lam_u'] = uniforms(seed + 50, 2)
        for surf, tag, aname, ang in (('wall', 'out', 'half', N.pi / 2.), ('sph', 'in', '03', 0.3)):
            N.random.seed(seed + 50)
            data[k + 'lam_%s_%s_%s' % (surf, tag, aname)] = sampling.Lambertian_directions_sampling(NS, ang, normals=normals[surf, tag])
        # normals that include +z and -z exactly (the sphere's, the first two replaced): the axes and angles of the rotation, and
        # the directions turned to them
        nz = normals['sph', 'out'].copy()
        nz[:, 0] = [0., 0., 1.]
        nz[:, 1] = [0., 0., -1.]
        zs = N.zeros(nz.shape)
        zs[2] = 1.
        with N.errstate(divide='ignore', invalid='ignore'):
            axes, angles = vm.axes_and_angles_between(zs, nz)
            N.random.seed(seed + 50)
            data[k + 'lam_nz'] = sampling.Lambertian_directions_sampling(NS, 0.3, normals=nz)
        data[k + 'nz_axes'] = axes
        data[k + 'nz_angles'] = angles
        # the piecewise-linear distribution: sample (one uniform each, the same for every table), CDF and PDF at the samples
        data[k + 'tab_u'] = uniforms(seed + 7, 1)[0]
        for name, (xs, ys) in sorted(tables().items()):
            dist = sampling.PW_linear_distribution(xs, ys)
            N.random.seed(seed + 7)
            x, w = dist.sample(NS)
            assert N.array_equal(w, N.ones(NS))
            data[k + name + '_x'] = x
            inside = N.clip(x, xs[0] + 1e-9, xs[-1] - 1e-9)        # (CDF and PDF are evaluated there: strictly inside the table)
            data[k + name + '_cdf_at'] = dist.CDF(inside)
            data[k + name + '_pdf_at'] = dist.PDF(inside)
    for name, (xs, ys) in sorted(tables().items()):
        dist = sampling.PW_linear_distribution(xs, ys)
        data[name + '_xs'], data[name + '_ys'] = xs, ys
        data[name + '_a'], data[name + '_b'] = dist.a / (2. * dist.tot_integ), dist.b / dist.tot_integ
        data[name + '_cdf'] = dist.CDF_def
    path = os.path.join(HERE, 'lamp_sources.npz')
    N.savez_compressed(path, **data)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
