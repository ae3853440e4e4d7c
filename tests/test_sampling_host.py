"""
The host samplers of tracer_amd.sampling and the vector helpers of tracer_amd.vector_manipulations against the reference's own arrays
(tests/golden/lamp_sources.npz, written by tests/golden/make_golden_lamps.py from the real reference under fixed numpy seeds): equal
where only draws and products are involved, 1e-14 relative otherwise.  isotropic_directions_sampling, which the reference does not
define, against its known distribution.  No GPU.
"""
import os

import numpy as N
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = N.load(os.path.join(ROOT, 'tests', 'golden', 'lamp_sources.npz'))
SEEDS = [int(s) for s in GOLD['seeds']]
NS = int(GOLD['ns'])
R_C, L_C, R_S = GOLD['dims']
TABLES = ('lobe', 'flat', 'gap')


def close(got, ref):
    """1e-14 relative to the array's scale (its largest entry)"""
    return N.all(N.abs(got - ref) <= 1e-14 * N.max(N.abs(ref)))


@pytest.mark.parametrize('seed', SEEDS)
def test_position_samplers_return_the_reference_arrays(seed):
    from tracer_amd import sampling
    g = lambda name: GOLD['%d_%s' % (seed, name)]
    N.random.seed(seed)
    vol = sampling.cylinder_sampling(R_C, L_C, NS, volume=True)
    # the draws are the fixture's: zs, then the disc's azimuths and radii
    assert N.array_equal(vol[2], g('u')[0] * L_C - L_C / 2.)
    assert close(vol, g('vol_pos'))
    for inwards, sign in ((False, 1.), (True, -1.)):
        N.random.seed(seed)
        pos, nrm = sampling.cylinder_sampling(R_S, L_C, NS, normals=True, normal_in=inwards)
        assert close(pos, g('wall_pos')) and N.array_equal(nrm, sign * g('wall_n_out'))
        N.random.seed(seed)
        pos, nrm = sampling.sphere_sampling(R_S, NS, normals=True, normal_in=inwards)
        assert N.array_equal(nrm, sign * g('sph_n_out')) and N.array_equal(pos, R_S * g('sph_n_out'))
    N.random.seed(seed)
    assert N.array_equal(sampling.cylinder_sampling(R_S, L_C, NS), g('wall_pos'))       # (without normals: the positions alone)
    N.random.seed(seed)
    disk = sampling.disk_sampling(R_C, NS)
    assert close(disk[:2], g('disk_xy')) and not disk[2].any()
    N.random.seed(seed)
    pos, nrm = sampling.disk_sampling(R_C, NS, normals=True, normal_up=False)
    assert N.array_equal(pos, disk) and N.array_equal(nrm, N.vstack([N.zeros(NS), N.zeros(NS), -N.ones(NS)]))
    with pytest.raises(NotImplementedError):
        sampling.sphere_sampling(R_S, NS, volume=True)


@pytest.mark.parametrize('seed', SEEDS)
def test_lambertian_directions_return_the_reference_arrays(seed):
    from tracer_amd import sampling
    g = lambda name: GOLD['%d_%s' % (seed, name)]
    for name, normals, ang in (('lam_wall_out_half', g('wall_n_out'), N.pi / 2.), ('lam_sph_in_03', -g('sph_n_out'), 0.3)):
        N.random.seed(seed + 50)
        got = sampling.Lambertian_directions_sampling(NS, ang, normals=normals)
        assert close(got, g(name)), name
        assert N.allclose(N.sum(got ** 2, axis=0), 1., rtol=0, atol=1e-12)
    # about +z itself, and with no cone at all: the draws and products alone
    N.random.seed(seed + 50)
    flat = sampling.Lambertian_directions_sampling(NS, 0.3)
    xi1, xi2 = g('lam_u')[0] * 2. * N.pi, g('lam_u')[1]
    s = N.sin(0.3) * N.sqrt(xi2)
    assert N.array_equal(flat, N.vstack((N.cos(xi1) * s, N.sin(xi1) * s, N.sqrt(1. - s ** 2.))))
    assert N.array_equal(sampling.Lambertian_directions_sampling(5, 0.), N.vstack((N.zeros((2, 5)), N.ones(5))))


@pytest.mark.parametrize('seed', SEEDS)
def test_axes_and_angles_between(seed):
    """on the fixture's normals, the first two of them +z and -z exactly"""
    from tracer_amd import sampling
    from tracer_amd.vector_manipulations import axes_and_angles_between, get_angle, get_angles, get_plane_normals, rotate_z_to_normal
    g = lambda name: GOLD['%d_%s' % (seed, name)]
    nz = g('sph_n_out').copy()
    nz[:, 0] = [0., 0., 1.]
    nz[:, 1] = [0., 0., -1.]
    zs = N.zeros(nz.shape)
    zs[2] = 1.
    axes, angles = axes_and_angles_between(zs, nz)
    assert close(axes, g('nz_axes')) and close(angles, g('nz_angles'))
    assert N.array_equal(axes[:, :2], [[1., 1.], [0., 0.], [0., 0.]]) and angles[0] == 0. and angles[1] == N.pi
    assert N.array_equal(get_plane_normals(zs.T, nz.T), axes) and N.array_equal(get_angles(zs, nz), angles)
    # one vector against one vector, and one normal for every column
    k = 5
    axis, angle = axes_and_angles_between(N.array([0., 0., 1.]), nz[:, k])
    assert close(axis, g('nz_axes')[:, k]) and abs(angle - g('nz_angles')[k]) <= 1e-14 * N.pi
    assert get_angle(N.array([0., 0., 2.]), N.array([3., 0., 0.])) == N.pi / 2.
    assert get_angle(N.array([0., 0., 1.]), N.array([0., 0., -1.]), signed=True) == -N.pi
    assert N.array_equal(get_angles(zs, nz[:, k]), N.full(NS, get_angles(zs, nz)[k]))
    N.random.seed(seed + 50)
    assert close(sampling.Lambertian_directions_sampling(NS, 0.3, normals=nz), g('lam_nz'))
    # -z: a half turn about x
    assert N.allclose(rotate_z_to_normal(N.array([[0.1], [0.2], [0.9]]), N.array([0., 0., -1.])), [[0.1], [-0.2], [-0.9]], rtol=0, atol=1e-14)


@pytest.mark.parametrize('name', TABLES)
def test_pw_linear_distribution_returns_the_reference_arrays(name):
    from tracer_amd.sampling import PW_linear_distribution
    xs, ys = GOLD[name + '_xs'], GOLD[name + '_ys']
    dist = PW_linear_distribution(xs, ys)
    assert N.array_equal(dist.xs, xs) and N.array_equal(dist.ys, ys)        # (rounded to 8 decimals already)
    assert N.array_equal(dist.CDF_def, GOLD[name + '_cdf'])
    assert N.array_equal(dist.a / (2. * dist.tot_integ), GOLD[name + '_a']) and N.array_equal(dist.b / dist.tot_integ, GOLD[name + '_b'])
    for seed in SEEDS:
        g = lambda what: GOLD['%d_%s_%s' % (seed, name, what)]
        N.random.seed(seed + 7)
        x, w = dist.sample(NS)
        assert close(x, g('x')) and N.array_equal(w, N.ones(NS))
        inside = N.clip(g('x'), xs[0] + 1e-9, xs[-1] - 1e-9)
        assert close(dist.CDF(inside), g('cdf_at')) and close(dist.PDF(inside), g('pdf_at'))
        assert N.all((x >= xs[0]) & (x <= xs[-1]))
    if name == 'gap':
        assert not N.any((x > 0.9) & (x < 1.3))


def ks_uniform(x, lo, hi):
    """the Kolmogorov-Smirnov distance of the sample x from U(lo, hi)"""
    x = N.sort((N.ravel(x) - lo) / (hi - lo))
    n = x.size
    return max(N.max(N.arange(1, n + 1) / float(n) - x), N.max(x - N.arange(n) / float(n)))


@pytest.mark.parametrize('ang', [N.pi / 2., 0.3])
def test_isotropic_directions_are_uniform_in_solid_angle(ang):
    """cos(theta) of 2e5 draws about +z is U(cos(ang), 1): KS below 1.5 x 1.36 / sqrt(n) (the 5 % point, with the margin
    test_gpu_sunshape.py uses); the azimuth is uniform too, and the draws are xi1, then xi2"""
    from tracer_amd.sampling import isotropic_directions_sampling
    from tracer_amd import sources
    assert sources.isotropic_directions_sampling is isotropic_directions_sampling
    n = 200000
    N.random.seed(77)
    d = isotropic_directions_sampling(n, ang, normals=N.tile(N.array([[0.], [0.], [1.]]), (1, n)))
    bound = 1.5 * 1.36 / N.sqrt(n)
    assert N.allclose(N.sum(d ** 2, axis=0), 1., rtol=0, atol=1e-12)
    assert ks_uniform(d[2], N.cos(ang), 1.) < bound
    az = N.arctan2(d[1], d[0])
    az[az < 0.] += 2. * N.pi
    assert ks_uniform(az, 0., 2. * N.pi) < bound
    N.random.seed(77)
    xi1 = N.random.uniform(low=0., high=2. * N.pi, size=n)
    xi2 = N.random.uniform(size=n)
    assert N.array_equal(d[2], 1. - xi2 * (1. - N.cos(ang)))
    N.random.seed(77)
    assert N.array_equal(isotropic_directions_sampling(n, ang), d)      # (normals = +z: no rotation)
    assert N.allclose(az, xi1, rtol=0, atol=1e-9)
    # about another normal: the same cone about it
    nrm = N.array([0.6, 0., 0.8])
    N.random.seed(78)
    d2 = isotropic_directions_sampling(20000, ang, normals=nrm)
    assert ks_uniform(N.dot(nrm, d2), N.cos(ang), 1.) < 1.5 * 1.36 / N.sqrt(20000)


def test_compat_resolves_the_modules_of_the_model():
    import sys
    from tracer_amd import compat
    compat.install()
    import ray_trace_utils.sampling as s
    import tracer.models.solar_simulator as m
    from tracer.sources import isotropic_directions_sampling
    from ray_trace_utils.vector_manipulations import axes_and_angles_between       # noqa: F401
    import tracer_amd.sampling
    assert s is tracer_amd.sampling and isotropic_directions_sampling is s.isotropic_directions_sampling
    assert sys.modules['tracer.models.solar_simulator'] is m
    for name in ('Target', 'SolarSimulator', 'SolarSimulatorModule', 'SimulatorReflector', 'SimulatorLampBader', 'SimulatorLampZhu'):
        assert hasattr(m, name)
