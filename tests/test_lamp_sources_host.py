"""
The arc-lamp source kinds of the per-ray core on the host (no GPU): trc_lamp_local_u / trc_lamp_ray_t of csrc/trc_core.h, compiled
with g++ (tests/hostcheck/lamp_check.cpp), fed the uniforms numpy handed the reference (tests/golden/lamp_sources.npz) in place of
their Philox draws, against the reference's own positions and directions; their Philox streams; the packing of the polar table; and
what the bundle constructors of tracer_amd.sources refuse.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = N.load(os.path.join(ROOT, 'tests', 'golden', 'lamp_sources.npz'))
SEEDS = [int(s) for s in GOLD['seeds']]
NS = int(GOLD['ns'])
R_C, L_C, R_S = [float(x) for x in GOLD['dims']]
_p = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_p)


@pytest.fixture(scope='module')
def hl():
    from tracer_amd import _cabi
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_lamp_check.so'))
    sd = C.POINTER(_cabi.SourceDesc)
    lib.hl_sizeof_source_desc.restype = C.c_long
    lib.hl_angle_table_pack.argtypes = [C.c_int, _p, _p, _p]
    lib.hl_lamp_rays_u.argtypes = [sd, _p, C.c_int, C.c_long, _p] + [_p] * 6
    lib.hl_lamp_rays.argtypes = [sd, _p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_long] + [_p] * 6
    lib.hl_uniforms.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_uint, _p]
    return lib


def pack(hl, xs, ys):
    xs, ys = N.ascontiguousarray(xs, dtype=float), N.ascontiguousarray(ys, dtype=float)
    tab = N.zeros(3 * xs.size)
    assert hl.hl_angle_table_pack(xs.size, _ptr(xs), _ptr(ys), _ptr(tab)) == 1
    return tab


def desc_of(bundle):
    return bundle._src_desc         # (the descriptor as the constructor filled it: no device, no table id)


def rays_u(hl, desc, tab, u):
    u = N.ascontiguousarray(u, dtype=float)
    m = u.shape[1]
    out = [N.zeros(m) for _ in range(6)]
    hl.hl_lamp_rays_u(C.byref(desc), _ptr(tab) if tab is not None else None, 0 if tab is None else tab.size // 3, m, _ptr(u), *[_ptr(o) for o in out])
    return N.array(out[:3]), N.array(out[3:])


def rays(hl, desc, tab, seed, rid0, m):
    out = [N.zeros(m) for _ in range(6)]
    hl.hl_lamp_rays(C.byref(desc), _ptr(tab) if tab is not None else None, 0 if tab is None else tab.size // 3, seed, rid0, m, *[_ptr(o) for o in out])
    return N.array(out[:3]), N.array(out[3:])


def uniforms(hl, seed, rid0, m, block):
    u = N.zeros((m, 4))
    for k in range(m):
        hl.hl_uniforms(seed, rid0 + k, block, _ptr(u[k]))
    return u.T.copy()


ORIGIN = N.zeros((3, 1))
TILT = dict(center=N.array([[0.3], [-0.2], [1.1]]), direction=N.array([0.48, -0.6, 0.64]))


def posed(pos, dirs, center, direction):
    from tracer_amd.vector_manipulations import rotate_z_to_normal
    rot = rotate_z_to_normal(N.eye(3), N.asarray(direction, dtype=float))
    return N.dot(rot, pos) + center, N.dot(rot, dirs)


def test_the_kinds_and_the_descriptor_keep_the_abi(hl):
    from tracer_amd import _cabi
    assert [hl.hl_kind(k) for k in range(3)] == [_cabi.SRC_ARC_VOLUME, _cabi.SRC_EMIT_SPHERE, _cabi.SRC_EMIT_CYLINDER] == [9, 10, 11]
    assert hl.hl_sizeof_source_desc() == C.sizeof(_cabi.SourceDesc)
    assert 'trc_angle_table_create' in _cabi.SIGNATURES


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('pose', [dict(center=ORIGIN, direction=N.array([0., 0., 1.])), TILT], ids=['local', 'tilted'])
def test_arc_volume_from_the_reference_uniforms(hl, seed, pose):
    """positions to 1e-12 x the source's size; the polar angle to the criterion of test_source_spectrum.py (where the reference's own
    closed form is accurate: 1e-12 x the table's width); the azimuth of the direction to 1e-12"""
    from tracer_amd import sources
    g = lambda name: GOLD['%d_%s' % (seed, name)]
    u_az = N.random.RandomState(seed).uniform(size=NS)
    for name in ('lobe', 'flat', 'gap'):
        xs, ys = GOLD[name + '_xs'], GOLD[name + '_ys']
        tab = pack(hl, xs, ys)
        b = sources.arc_volume_bundle(NS, R_C, L_C, xs, ys, pose['center'], pose['direction'], 1500., seed=1)
        u = N.vstack((g('u'), g('tab_u')[None, :], u_az[None, :]))
        pos, dirs = rays_u(hl, desc_of(b), tab, u)
        theta_ref = g(name + '_x')
        phis = u_az * 2. * N.pi
        ref_dirs = N.vstack([N.sin(theta_ref) * N.cos(phis), N.sin(theta_ref) * N.sin(phis), N.cos(theta_ref)])
        ref_pos, ref_dirs = posed(g('vol_pos'), ref_dirs, pose['center'], pose['direction'])
        assert N.abs(pos - ref_pos).max() <= 1e-12 * max(R_C, L_C)
        # back in the lamp's frame: polar angle and azimuth
        from tracer_amd.vector_manipulations import rotate_z_to_normal
        rot = rotate_z_to_normal(N.eye(3), pose['direction'])
        loc = N.dot(rot.T, dirs)
        theta = N.arctan2(N.sqrt(loc[0] ** 2 + loc[1] ** 2), loc[2])
        width = xs[-1] - xs[0]
        a, bb, cdf, uu = GOLD[name + '_a'], GOLD[name + '_b'], GOLD[name + '_cdf'], g('tab_u')
        i = N.clip(N.searchsorted(cdf, uu, side='right') - 1, 0, xs.size - 2)
        with N.errstate(divide='ignore', invalid='ignore'):
            D = bb[i] ** 2 + 4. * a[i] * (uu - cdf[i] + a[i] * xs[i] ** 2 + bb[i] * xs[i])
            ref_err = N.where(a[i] != 0., 8. * N.finfo(float).eps * (N.abs(bb[i]) + N.sqrt(N.abs(D))) / N.abs(2. * a[i]), 0.)
        accurate = ref_err < 1e-13 * width
        assert accurate.mean() > 0.5
        err = N.abs(theta - theta_ref)
        assert N.all(err[accurate] <= 1e-12 * width), (name, err[accurate].max() / width)
        assert N.all((theta >= xs[0] - 1e-12) & (theta <= xs[-1] + 1e-12))
        if name == 'gap':
            assert not N.any((theta > 0.9 + 1e-12) & (theta < 1.3 - 1e-12))
        st = N.sin(theta)
        ok = st > 1e-3
        assert N.abs(loc[0][ok] / st[ok] - N.cos(phis[ok])).max() <= 1e-12 and N.abs(loc[1][ok] / st[ok] - N.sin(phis[ok])).max() <= 1e-12
        assert N.abs(N.sum(dirs ** 2, axis=0) - 1.).max() <= 1e-12
        # the directions themselves where the reference's angle is accurate
        assert N.abs(dirs - ref_dirs)[:, accurate].max() <= 2e-12 * width


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('pose', [dict(center=ORIGIN, direction=N.array([0., 0., 1.])), TILT], ids=['local', 'tilted'])
def test_emitters_from_the_reference_uniforms(hl, seed, pose):
    """positions to 1e-12 x the source's size, directions to 1e-12: sphere (normals in, cone 0.3) and wall (normals out, half space)"""
    from tracer_amd import sources
    g = lambda name: GOLD['%d_%s' % (seed, name)]
    u = N.vstack((g('u')[:2], g('lam_u'), N.full((1, NS), 0.123)))
    b = sources.sphere_emitter_bundle(NS, R_S, pose['center'], pose['direction'], 10., ang_range=0.3, law='lambertian', rays_in=True, seed=1)
    pos, dirs = rays_u(hl, desc_of(b), None, u)
    ref_pos, ref_dirs = posed(R_S * g('sph_n_out'), g('lam_sph_in_03'), pose['center'], pose['direction'])
    assert N.abs(pos - ref_pos).max() <= 1e-12 * R_S and N.abs(dirs - ref_dirs).max() <= 1e-12
    b = sources.cylinder_emitter_bundle(NS, R_S, L_C, pose['center'], pose['direction'], 10., seed=1)
    pos, dirs = rays_u(hl, desc_of(b), None, u)
    ref_pos, ref_dirs = posed(g('wall_pos'), g('lam_wall_out_half'), pose['center'], pose['direction'])
    assert N.abs(pos - ref_pos).max() <= 1e-12 * max(R_S, L_C) and N.abs(dirs - ref_dirs).max() <= 1e-12
    # the isotropic law about the same normals: the host sampler's directions (the reference has none)
    from tracer_amd import sampling
    N.random.seed(seed + 50)
    iso = sampling.isotropic_directions_sampling(NS, 0.7, normals=g('wall_n_out'))
    b = sources.cylinder_emitter_bundle(NS, R_S, L_C, pose['center'], pose['direction'], 10., ang_range=0.7, law='isotropic', seed=1)
    pos, dirs = rays_u(hl, desc_of(b), None, u)
    assert N.abs(dirs - posed(g('wall_pos'), iso, pose['center'], pose['direction'])[1]).max() <= 1e-12
    # normals +z and -z exactly (the sphere's poles: cos = 1 is u1 = 1, which no draw gives; -1 is u1 = 0)
    up = N.array([[0.25], [0.], [0.3], [0.4], [0.]])
    b = sources.sphere_emitter_bundle(1, R_S, ORIGIN, [0., 0., 1.], 1., ang_range=0.3, seed=1)
    pos, dirs = rays_u(hl, desc_of(b), None, up)
    s = N.sin(0.3) * N.sqrt(0.4)
    assert N.allclose(pos[:, 0], [0., 0., -R_S], rtol=0, atol=1e-18)
    assert N.allclose(dirs[:, 0], [N.cos(0.6 * N.pi) * s, -N.sin(0.6 * N.pi) * s, -N.sqrt(1. - s * s)], rtol=0, atol=1e-14)


def test_philox_streams(hl):
    """a ray is the same for ray_offset a, index i, as for offset 0, index a + i; the rays are those of the uniforms of block 0
    and -- ARC_VOLUME alone -- the first uniform of block 1"""
    from tracer_amd import sources
    xs, ys = GOLD['lobe_xs'], GOLD['lobe_ys']
    tab = pack(hl, xs, ys)
    seed, a, m = 987654321, 1000, 64
    lamps = [(sources.arc_volume_bundle(m, R_C, L_C, xs, ys, TILT['center'], TILT['direction'], 1., seed=seed), tab),
             (sources.sphere_emitter_bundle(m, R_S, TILT['center'], TILT['direction'], 1., law='isotropic', seed=seed), None),
             (sources.cylinder_emitter_bundle(m, R_S, L_C, TILT['center'], TILT['direction'], 1., rays_in=True, seed=seed), None)]
    u0, u1 = uniforms(hl, seed, a, m, 0), uniforms(hl, seed, a, m, 1)
    for k, (b, t) in enumerate(lamps):
        d = desc_of(b)
        whole = rays(hl, d, t, seed, 0, a + m)
        part = rays(hl, d, t, seed, a, m)
        assert N.array_equal(whole[0][:, a:], part[0]) and N.array_equal(whole[1][:, a:], part[1])
        with_b1 = rays_u(hl, d, t, N.vstack((u0, u1[:1])))
        other = rays_u(hl, d, t, N.vstack((u0, (1. - u1[:1]))))
        assert N.array_equal(with_b1[0], part[0]) and N.array_equal(with_b1[1], part[1])
        assert N.array_equal(other[0], part[0])
        if k == 0:
            assert not N.array_equal(other[1], part[1])     # block 1 turns the arc's directions about the axis
        else:
            assert N.array_equal(other[1], part[1])         # the emitters never read it
        assert N.abs(N.sum(part[1] ** 2, axis=0) - 1.).max() < 1e-12


@pytest.mark.parametrize('name', ['lobe', 'flat', 'gap'])
def test_angle_table_packing_is_the_spectrum_packing(hl, name):
    from tracer_amd.source_spectrum import SourceSpectrum
    xs, ys = GOLD[name + '_xs'], GOLD[name + '_ys']
    wl, val, cdf = SourceSpectrum.tabulated(xs, ys).table()
    tab = pack(hl, xs, ys)
    n = xs.size
    assert N.array_equal(tab[:n], wl) and N.array_equal(tab[n:2 * n], val) and N.array_equal(tab[2 * n:], cdf)
    assert tab[2 * n] == 0. and tab[-1] == 1.
    zero = N.zeros(3 * n)
    assert hl.hl_angle_table_pack(n, _ptr(N.ascontiguousarray(xs)), _ptr(N.zeros(n)), _ptr(zero)) == 0


def test_constructors_refuse_bad_input():
    from tracer_amd import sources
    c, d = ORIGIN, [0., 0., 1.]
    th, dens = N.linspace(0., N.pi, 5), N.ones(5)
    for bad_th, bad_d in ((th[::-1], dens), (th, -dens), (th, N.zeros(5)), (th + 0.1, dens), (th[:1], dens[:1]), (th, dens[:4]),
                          (N.where(N.arange(5) == 2, N.nan, th), dens)):
        with pytest.raises(ValueError):
            sources.arc_volume_bundle(10, R_C, L_C, bad_th, bad_d, c, d, 1.)
    for r, l in ((0., L_C), (-1., L_C), (R_C, 0.), (N.inf, L_C)):
        with pytest.raises(ValueError):
            sources.arc_volume_bundle(10, r, l, th, dens, c, d, 1.)
        with pytest.raises(ValueError):
            sources.cylinder_emitter_bundle(10, r, l, c, d, 1.)
    for r in (0., -2., N.nan):
        with pytest.raises(ValueError):
            sources.sphere_emitter_bundle(10, r, c, d, 1.)
    for law in ('Lambertian', 'uniform', None, 1):
        with pytest.raises(ValueError):
            sources.sphere_emitter_bundle(10, R_S, c, d, 1., law=law)
        with pytest.raises(ValueError):
            sources.cylinder_emitter_bundle(10, R_S, L_C, c, d, 1., law=law)
    with pytest.raises(ValueError):
        sources.sphere_emitter_bundle(10, R_S, c, d, 1., ang_range=2.)
    with pytest.raises(TypeError):
        sources.sphere_emitter_bundle(10, R_S, c, d, 1., spectrum='white')
    # what they accept: pending bundles with power / n per ray, the laws and the sign in the descriptor
    from tracer_amd import _cabi
    b = sources.cylinder_emitter_bundle(40, R_S, L_C, c, d, 8., law='isotropic', rays_in=True)
    assert b.is_pending() and b.get_num_rays() == 40 and b._src_desc.energy == 0.2 and b._src_desc.kind == _cabi.SRC_EMIT_CYLINDER
    assert list(b._src_desc.p)[:5] == [R_S, L_C, N.pi / 2., float(_cabi.EMIT_ISOTROPIC), -1.]
    b = sources.sphere_emitter_bundle(40, R_S, c, d, 8.)
    assert list(b._src_desc.p)[:4] == [R_S, N.pi / 2., float(_cabi.EMIT_LAMBERTIAN), 1.]
    b = sources.arc_volume_bundle(40, R_C, L_C, th, dens, c, d, 8.)
    assert b.is_pending() and list(b._src_desc.p)[:2] == [R_C, L_C] and b._src_table is sources.angle_table(th, dens)


def test_the_lamps_of_the_model_without_a_device():
    from tracer_amd.models import solar_simulator as M
    with pytest.raises(ValueError):
        M.SimulatorLampBader()
    cdf = N.array([N.linspace(0., N.pi, 9), N.linspace(0., 1., 9) ** 2]).T
    lamp = M.SimulatorLampBader(theta_CDF=cdf)
    (b,) = lamp.sources(1000, part_load=0.5, seed=3)
    assert b.is_pending() and b.get_num_rays() == 1000 and abs(b._src_desc.energy - 0.5 * 1500. / 1000) < 1e-15
    assert N.allclose(lamp.ths, (cdf[:-1, 0] + cdf[1:, 0]) / 2., atol=1e-8) and N.allclose(lamp.ths_PDF, N.diff(cdf[:, 1]) / N.diff(cdf[:, 0]), atol=1e-8)
    zhu = M.SimulatorLampZhu()
    parts = zhu.sources(10000, seed=5)
    assert [p.get_num_rays() for p in parts] == [3000, 412, 6588] and all(p.is_pending() for p in parts)
    assert [p._src_offset for p in parts] == [0, 3000, 3412] and len(set(p._src_seed for p in parts)) == 1
    assert abs(sum(p._src_desc.energy * p.get_num_rays() for p in parts) - zhu.P) < 1e-9
    assert list(parts[0]._src_desc.center) == [0., 0., -(zhu.l_c / 2. - zhu.r_s)]
    with pytest.raises(ValueError):
        M.SolarSimulatorModule(0.3, 0.3, 0.5, [-0.5, 0.], lampdict={'model': 'Halogen'})
    mod = M.SolarSimulatorModule(0.3, 0.3, 0.5, [-0.5, 0.], lampdict={'model': 'Zhu'}, first_focus_location=[1., 2., 3.], aiming_vector=[0., 0.6, 0.8])
    assert N.allclose(N.dot(mod.rotation, [0., 0., 1.]), [0., 0.6, 0.8], atol=1e-14)
    posed = mod.lamp_sources(1000, seed=1)
    assert N.allclose(list(posed[1]._src_desc.center), [1., 2., 3.]) and N.allclose(N.array(list(posed[1]._src_desc.rot_dir)).reshape(3, 3), mod.rotation)
    sim = M.SolarSimulator([[0., 0., 0.]], [[0., 0., 1.]], [dict(a=0.3, b=0.3, c=0.5, zlim=[-0.5, 0.], lampdict={'model': 'Zhu'})],
                           [M.Target(0.1, 0.1, [0., 0., 0.8], N.array([0., 0., -1.]), N.linspace(-.05, .05, 6), N.linspace(-.05, .05, 5))])
    assert len(sim.get_surfaces()) == 2 and sim.targets[0].areas.shape == (5, 4)
    with pytest.raises(NotImplementedError):
        sim.simulate(100, rendering=True)


def test_estimator_takes_a_two_dimensional_map():
    """a Target's map is (nx, ny): mean and confidence interval keep its shape; bins that never vary have an interval of 0"""
    from tracer_amd.estimator import Estimator
    est = Estimator()
    rs = N.random.RandomState(4)
    for _ in range(4):
        m = rs.uniform(1., 2., size=(5, 3))
        m[0, 0] = 0.
        est.update(m, num_samples=100)
    ci = est.get_CI()
    assert est.mean.shape == ci.shape == (5, 3) and N.all(N.isfinite(ci)) and ci[0, 0] == 0. and N.all(ci[1:] > 0.)
