"""
The thermal emitters on the device: the rays of thermal_emitter_bundle and gray_source as trc_source_generate makes them against the
host build of the same per-ray code (tests/hostcheck/thermal_check.cpp); the device table against the host packing; the polar
distribution against the exact CDF; the engines' agreement -- the streaming form (k_s_gen_emit), the megakernel (the lamps'
k_lamp_coop / k_lamp_fast), the ordered engine and the materialised bundle given -- in a closed cavity, with and without a source
spectrum; a known answer (the view factor between coaxial discs); tables of another packing, destroyed tables, refused tables.
"""
import ctypes as C

import numpy as N
import pytest

import thermal_cases as TC

pytestmark = pytest.mark.gpu

CENTER = N.array([0.3, -0.2, 1.1])
AXIS = N.array([0.48, -0.6, 0.64])
SHAPES = {'disk': TC.shape_dict('disk'), 'rectangle': {'type': 'rectangle', 'kwargs': {'x': 0.4, 'y': 1.2}},
          'triangle': TC.shape_dict('triangle'), 'cylinder': TC.shape_dict('cylinder'), 'frustum': TC.shape_dict('frustum_narrow'),
          'sphere': TC.shape_dict('sphere')}
SIZES = {'disk': 0.25, 'rectangle': 1.2, 'triangle': 0.7, 'cylinder': 0.7, 'frustum': 0.6, 'sphere': 0.3}


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


@pytest.fixture(scope='module')
def ht():
    return TC.load_hostcheck()


def emitter(shape, n, seed, offset=0, table='dir', center=CENTER, direction=AXIS, **kw):
    from tracer_amd import sources
    xs, ys = TC.raw_table(table)
    return sources.thermal_emitter_bundle(n, shape, xs, ys, TC.T_WALL, TC.BAND, center, direction, seed=seed, ray_offset=offset, **kw)


def device_table(b):
    t, e, cdf, tc, mass = b._src_table.packed()
    return N.ascontiguousarray(N.concatenate((t, e, cdf))), tc, mass


# 1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rays_in', [False, True], ids=['out', 'in'])
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_generate_matches_the_host_build(ctx, ht, name, rays_in):
    """
    2e4 rays at ray offset 1000, tilted, table `dir`: no ray left out; points to 1e-12 x the shape's size; directions through the
    CDF -- theta_dev = atan2(|d x n|, d . n) about the host build's normal n has |F(theta_dev) - u2| <= 1e-12 with u2 from the host
    build's Philox, and the device direction is the host build's rebuilt from (theta_dev, u3, n) to 1e-12.  (theta is ill-conditioned
    where the density vanishes -- towards 0, and at the zero of eps at pi/2, where F = 1 - k delta^3 makes a residual of 1e-15 an
    angle of 1e-9 -- and the device's and the host's sincos differ in the last place, so theta is not compared with theta.)
    """
    m, seed, off = 20000, 17, 1000
    b = emitter(SHAPES[name], m, seed, off, rays_in=rays_in)
    tab, tc, mass = device_table(b)
    xs, ys = TC.table('dir')
    host_tab, host_mass = TC.pack(ht, *TC.raw_table('dir'))
    assert N.array_equal(tab, host_tab) and mass == host_mass and tc == xs[-1]
    pos, dirs, local_n, u = TC.host_rays(ht, b.source_args()[0], tab, seed, off, m)
    rot = N.array(list(b.source_args()[0].rot_dir)).reshape(3, 3)
    nrm = N.dot(rot, local_n)
    v, d = b.get_vertices(), b.get_directions()
    assert v.shape == (3, m) and N.all(N.isfinite(v)) and N.all(N.isfinite(d))
    assert N.abs(N.sum(d * d, axis=0) - 1.).max() <= 1e-12
    assert N.abs(v - pos).max() <= 1e-12 * SIZES[name]
    cross = N.cross(d, nrm, axis=0)
    th_dev = N.arctan2(N.sqrt(N.sum(cross * cross, axis=0)), N.sum(d * nrm, axis=0))
    res = N.abs(TC.cdf_at(xs, ys, N.clip(th_dev, xs[0], xs[-1])) - u[2])
    print(name, rays_in, 'CDF residual', res.max(), 'theta range', th_dev.min(), th_dev.max())
    assert res.max() <= 1e-12
    assert th_dev.max() <= xs[-1] + 1e-9
    # (rebuilt in the source's own frame, where the minimal rotation from +z to the normal is taken -- about the host build's normal
    # there as it is, +-z exactly on the flat shapes -- and posed by rot_dir)
    rebuilt = N.dot(rot, TC.host_dirs(ht, th_dev, u[3], local_n))
    print(name, rays_in, 'direction against the rebuilt one', N.abs(d - rebuilt).max())
    assert N.abs(d - rebuilt).max() <= 1e-12
    assert N.array_equal(b.get_energy(), N.full(m, b.source_args()[0].energy))
    assert N.array_equal(b.get_wavelengths(), N.full(m, b.source_spectrum().wavelength))
    # the sense: the rays leave along the shape's normal, against it with rays_in
    assert N.allclose(rot, rot_of(AXIS), atol=1e-15)
    if name in ('disk', 'rectangle', 'triangle'):
        assert N.allclose(local_n, N.array([[0.], [0.], [-1. if rays_in else 1.]]) * N.ones((1, m)), atol=1e-12)
    elif name in ('cylinder', 'sphere'):
        lp = N.dot(rot_of(AXIS).T, v - CENTER[:, None])
        radial = lp.copy()
        if name == 'cylinder':
            radial[2] = 0.
        assert N.all(N.sum(radial * local_n, axis=0) * (-1. if rays_in else 1.) > 0.)
    # the two halves at their own offsets are the whole
    if not rays_in:
        h1, h2 = emitter(SHAPES[name], m // 2, seed, off), emitter(SHAPES[name], m - m // 2, seed, off + m // 2)
        assert N.array_equal(N.hstack((h1.get_vertices(), h2.get_vertices())), v)
        assert N.array_equal(N.hstack((h1.get_directions(), h2.get_directions())), d)


def rot_of(direction):
    from tracer_amd.vector_manipulations import rotate_z_to_normal
    return rotate_z_to_normal(N.eye(3), N.asarray(direction, dtype=float))


# 2 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('table', TC.TABLES)
def test_every_table_on_the_device(ctx, ht, table):
    """2e4 rays of a disc per table: the device table is the host packing; the polar angle about +z solves the CDF to 1e-12; nothing
    in `gap`'s empty stretch, nothing beyond a table's last angle"""
    m, seed = 20000, 23
    b = emitter(SHAPES['disk'], m, seed, table=table, center=N.zeros(3), direction=N.array([0., 0., 1.]), quadrature='exact')
    tab, tc, mass = device_table(b)
    host_tab, host_mass = TC.pack(ht, *TC.raw_table(table))
    assert N.array_equal(tab, host_tab) and mass == host_mass
    xs, ys = TC.table(table)
    d = b.get_directions()
    pos, dirs, nrm, u = TC.host_rays(ht, b.source_args()[0], tab, seed, 0, m)
    th = N.arctan2(N.hypot(d[0], d[1]), d[2])
    res = N.abs(TC.cdf_at(xs, ys, N.clip(th, xs[0], xs[-1])) - u[2])
    print(table, 'CDF residual', res.max())
    assert res.max() <= 1e-12
    assert th.max() <= xs[-1] + 1e-9
    if table == 'gap':
        assert not N.any((th > 0.5 + 1e-9) & (th < 0.9 - 1e-9))


def test_gray_source_is_the_lambertian_law(ctx, ht):
    """gray_source on the wall of a cylinder, points posed by `direction` and directions by rays_direction: against the host build, and
    sin^2(theta) / sin^2(ang_range) about the normal uniform (Kolmogorov-Smirnov below 1.5 x 1.36 / sqrt(n))"""
    from tracer_amd import sources
    n, ang = 200000, 0.7
    d1, d2 = N.array([0., 0.6, 0.8]), N.array([0.6, 0., 0.8])
    b = sources.gray_source(SHAPES['cylinder'], CENTER, d1, n, {'type': 'Lambertian', 'kwargs': {'ang_range': ang}}, 50.,
                            rays_direction=d2, seed=29)
    tab, tc, mass = device_table(b)
    pos, dirs, local_n, u = TC.host_rays(ht, b.source_args()[0], tab, 29, 0, n)
    nrm = N.dot(rot_of(d2), local_n)
    v, d = b.get_vertices(), b.get_directions()
    assert N.abs(v - pos).max() <= 1e-12 * SIZES['cylinder'] and N.abs(d - dirs).max() <= 1e-12      # (the closed form: no zero of the density inside)
    assert N.allclose(b.get_energy(), 50. / n * N.cos(N.dot(d2, d1)), rtol=1e-15)
    lp = N.dot(rot_of(d1).T, v - CENTER[:, None])
    assert N.abs(N.hypot(lp[0], lp[1]) - 0.2).max() <= 1e-12 and N.abs(lp[2]).max() <= 0.35 + 1e-12
    cos = N.sum(d * nrm, axis=0)
    assert cos.min() >= N.cos(ang) - 1e-12
    x = N.sort(N.clip(1. - cos ** 2, 0., None) / N.sin(ang) ** 2)
    ks = max(N.abs(N.arange(1, n + 1) / float(n) - x).max(), N.abs(x - N.arange(n) / float(n)).max())
    assert ks < 1.5 * 1.36 / N.sqrt(n)


# 3 -------------------------------------------------------------------------------------------------------------------------------
def cavity():
    """a receiver plate over an emitting disc, inside an absorbing sphere.  Surfaces: mirror ring (a reflecting plate beside the axis),
    receiver, enclosure."""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.sphere_surface import SphericalGM
    from tracer_amd.optics_callables import Reflective
    from tracer_amd.spatial_geometry import rotx
    mirror = AssembledObject(surfs=[Surface(geometry=RectPlateGM(0.6, 0.6), optics=Reflective(0.1))], location=N.array([0.5, 0., 0.4]),
                             rotation=rotx(N.pi)[:3, :3])
    receiver = AssembledObject(surfs=[Surface(geometry=RectPlateGM(0.5, 0.5), optics=Reflective(1.))], location=N.array([0., 0., 0.5]),
                               rotation=rotx(N.pi)[:3, :3])
    shell = AssembledObject(surfs=[Surface(geometry=SphericalGM(radius=3.), optics=Reflective(1.))])
    return Assembly(objects=[mirror, receiver, shell])


def trace(ctx, cs, bundle, how, reps=20):
    from tracer_amd.scene import DeviceScene
    dev = DeviceScene(cs, ctx)
    edges = N.linspace(-0.25, 0.25, 6)
    dev.set_fluxmap(1, edges, edges)
    e0 = bundle.source_args()[0].energy if how != 'given' else bundle.get_energy()[0]
    if how == 'ordered':
        res, st = dev.trace_ordered(bundle, reps, 1e-6 * e0, 5)
        res.close()
    else:
        dev.trace_fast(bundle, reps, 1e-6 * e0, 5, stream={'stream': True, 'mega': False, 'given': True, 'auto': None}[how])
    a, r, h = dev.get_tallies()
    fm = dev.get_fluxmap(1)
    dev.close()
    return a.copy(), h.copy(), fm.copy()


@pytest.mark.parametrize('spectrum', ['band_average', 'planck'])
@pytest.mark.parametrize('name', ['disk', 'frustum', 'sphere'])
def test_engines_agree_in_a_cavity(ctx, name, spectrum):
    """5e4 rays of an emitter under a receiver: the streaming form, the megakernel, the ordered engine and the materialised bundle given
    -- the same hits per surface, absorbed energies and flux maps to 1e-9, the bundle still pending; the same with 50 rays, where the
    plan picks the megakernel, and with 64, the fewest the streaming form takes.  Under spectrum='planck' the SPEC instances run."""
    from tracer_amd.scene import compile_scene
    from tracer_amd.ray_bundle import RayBundle
    cs = compile_scene(cavity())
    for n, hows in ((50000, ('stream', 'mega', 'ordered')), (50, ('auto', 'ordered')), (64, ('stream', 'mega'))):
        mk = lambda: emitter(SHAPES[name], n, 5, center=N.zeros(3), direction=N.array([0., 0., 1.]), spectrum=spectrum, ref_index=1.)
        m = mk()
        given = RayBundle(vertices=m.get_vertices(), directions=m.get_directions(), energy=m.get_energy())
        a_ref, h_ref, fm_ref = trace(ctx, cs, given, 'given')
        assert h_ref.sum() >= n
        if n >= 1000:
            assert h_ref[1] > 0.05 * n and fm_ref.sum() > 0.
        for how in hows:
            b = mk()
            got_a, got_h, got_fm = trace(ctx, cs, b, how)
            assert b.is_pending(), how
            assert N.array_equal(got_h, h_ref), (how, n)
            assert N.allclose(got_a, a_ref, rtol=1e-9, atol=1e-12 * a_ref.max()), (how, n)
            assert N.allclose(got_fm, fm_ref, rtol=1e-9, atol=1e-12 * max(fm_ref.max(), a_ref.max())), (how, n)


def test_a_planck_spectrum_leaves_the_rays_as_they_are(ctx):
    """one wavelength per ray drawn in the band; points and directions those of the band-average bundle"""
    s, p = emitter(SHAPES['cylinder'], 50000, 41, spectrum='planck'), emitter(SHAPES['cylinder'], 50000, 41)
    assert s.is_pending()
    assert N.array_equal(s.get_vertices(), p.get_vertices()) and N.array_equal(s.get_directions(), p.get_directions())
    wl = s.get_wavelengths()
    assert wl.shape == (50000,) and wl.min() >= TC.BAND[0] and wl.max() <= TC.BAND[1] and N.unique(wl).size > 45000
    assert N.array_equal(p.get_wavelengths(), N.full(50000, p.source_spectrum().wavelength))


# 4 -------------------------------------------------------------------------------------------------------------------------------
def test_view_factor_between_coaxial_discs(ctx):
    """
    A gray diffuse disc of radius 1 under an equal disc at height 1: the share of its rays that lands on the other is the view factor
    F = (3 - sqrt(5)) / 2 (coaxial parallel discs, R1 = R2 = h: X = 3, F = (X - sqrt(X^2 - 4)) / 2), within 4 binomial standard
    deviations at 4e5 rays -- by every form, from the constant table (the closed form) and from a table whose emittance is 0.8 too but
    is stated on 5 points.  The power over the tallies is conserved to 1e-12.
    """
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RoundPlateGM
    from tracer_amd.sphere_surface import SphericalGM
    from tracer_amd.optics_callables import Reflective
    from tracer_amd.scene import compile_scene, DeviceScene
    from tracer_amd.spatial_geometry import rotx
    top = AssembledObject(surfs=[Surface(geometry=RoundPlateGM(Re=1.), optics=Reflective(1.))], location=N.array([0., 0., 1.]),
                          rotation=rotx(N.pi)[:3, :3])
    shell = AssembledObject(surfs=[Surface(geometry=SphericalGM(radius=5.), optics=Reflective(1.))])
    cs = compile_scene(Assembly(objects=[top, shell]))
    n = 400000
    F = 0.5 * (3. - N.sqrt(5.))
    sigma = N.sqrt(F * (1. - F) / n)
    for table, how in (('gray2', 'mega'), ('gray', 'stream')):
        b = emitter({'type': 'disk', 'kwargs': {'r_ext': 1.}}, n, 13, table=table, center=N.zeros(3), direction=N.array([0., 0., 1.]),
                    quadrature='exact')     # (the node trapezoid of a two-point table over [0, pi/2] is no power at all)
        e = b.source_args()[0].energy
        dev = DeviceScene(cs, ctx)
        dev.trace_fast(b, 5, 1e-6 * e, 5, stream=(how == 'stream'))
        a, r, h = dev.get_tallies()
        dev.close()
        assert h[0] + h[1] == n and abs(a.sum() - n * e) <= 1e-12 * n * e
        print(table, how, 'view factor', h[0] / float(n), F, (h[0] / float(n) - F) / sigma, 'sigmas')
        assert abs(h[0] / float(n) - F) <= 4. * sigma


# 5 -------------------------------------------------------------------------------------------------------------------------------
def test_tables_of_another_packing_and_destroyed_tables_are_errors(ctx):
    from tracer_amd import _cabi, sources
    b = emitter(SHAPES['disk'], 1000, 3)
    cols = [N.empty(1000) for _ in range(7)]         # (kept alive: the struct holds their addresses)
    rays = _cabi.make_rays(1000, *cols)

    def generate(desc):
        return ctx.lib.trc_source_generate(ctx.handle, C.byref(desc), 1000, 3, 0, C.byref(rays))

    good = b.source_args()[0].table
    assert generate(b._src_desc) == 0
    for other in (sources.AngleTable([0., 1., 1.5], [1., 0.5, 0.1]), sources.SunshapeTable([0., 0.004, 0.01], [1., 0.5, 0.1])):
        b._src_desc.table = other.table_id()
        assert generate(b._src_desc) == _cabi.ERR_INVALID
    t = sources.EmittanceTable([0., 1., 1.5], [1., 0.5, 0.1])
    b._src_desc.table = t.table_id()
    assert generate(b._src_desc) == 0
    t.destroy()
    assert generate(b._src_desc) == _cabi.ERR_INVALID
    b._src_desc.table = 0
    assert generate(b._src_desc) == _cabi.ERR_INVALID
    # a shape the kind does not have, and the frustum that is a cylinder
    b._src_desc.table = good
    b._src_desc.p[0] = 6.
    assert generate(b._src_desc) == _cabi.ERR_INVALID
    b._src_desc.p[0], b._src_desc.p[1], b._src_desc.p[2] = 4., 0.2, 0.2
    assert generate(b._src_desc) == _cabi.ERR_INVALID
    # what trc_emittance_table_create refuses
    h = C.c_void_p()
    for th, eps in (([0., 1., 1.6], [1., 1., 1.]), ([0., 1.2, 1.], [1., 1., 1.]), ([0., 1., 1.5], [0., 0., 0.]), ([0., 1., 1.5], [1., -1., 1.]),
                    ([0., 1., 1.5], [1., N.nan, 1.])):
        th, eps = N.array(th), N.array(eps)
        assert ctx.lib.trc_emittance_table_create(ctx.handle, 3, _cabi.ptr(th), _cabi.ptr(eps), C.byref(h)) == _cabi.ERR_INVALID
    one = N.array([0.5])
    assert ctx.lib.trc_emittance_table_create(ctx.handle, 1, _cabi.ptr(one), _cabi.ptr(one), C.byref(h)) == _cabi.ERR_INVALID
