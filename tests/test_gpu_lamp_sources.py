"""
The arc-lamp sources on the device: the rays of arc_volume_bundle, sphere_emitter_bundle and cylinder_emitter_bundle as
trc_source_generate makes them against the host build of the same per-ray code; their distributions; the engines' agreement on one
module of a solar simulator; a known answer (a point lamp at one focus of a perfect ellipsoid); a source spectrum beside them; the
model (models/solar_simulator.py); a destroyed polar table.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = N.load(os.path.join(ROOT, 'tests', 'golden', 'lamp_sources.npz'))
_p = C.POINTER(C.c_double)
R_C, L_C, R_S = 7.5e-4, 4.5e-3, 2.5e-4
CENTER = N.array([[0.3], [-0.2], [1.1]])
AXIS = N.array([0.48, -0.6, 0.64])
KINDS = ['arc', 'sphere-lambertian', 'sphere-isotropic', 'cylinder-lambertian', 'cylinder-isotropic']
# the ellipsoid of the module: semi-axes A, A, C_; the foci F from its centre; the first focus is the origin
A, C_ = 0.3, 0.5
F = N.sqrt(C_ ** 2 - A ** 2)
ZLIM = [-C_, 0.]


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


@pytest.fixture(scope='module')
def hl():
    from tracer_amd import _cabi
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_lamp_check.so'))
    lib.hl_lamp_rays.argtypes = [C.POINTER(_cabi.SourceDesc), _p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_long] + [_p] * 6
    return lib


def _ptr(a):
    return a.ctypes.data_as(_p)


def lamp(kind, n, seed, offset=0, spectrum=None, center=CENTER, direction=AXIS, table='lobe', ang=None, size=1.):
    """a lamp part of kind `kind`; size: a factor on its dimensions"""
    from tracer_amd import sources
    what, _, law = kind.partition('-')
    if what == 'arc':
        return sources.arc_volume_bundle(n, R_C * size, L_C * size, GOLD[table + '_xs'], GOLD[table + '_ys'], center, direction, 1500.,
                                         seed=seed, ray_offset=offset, spectrum=spectrum)
    kw = dict(ang_range=(0.6 if law == 'lambertian' else N.pi / 2.) if ang is None else ang, law=law, seed=seed, ray_offset=offset, spectrum=spectrum)
    if what == 'sphere':
        return sources.sphere_emitter_bundle(n, R_S * size, center, direction, 900., **kw)
    return sources.cylinder_emitter_bundle(n, R_S * size, L_C * size, center, direction, 900., rays_in=(law == 'isotropic'), **kw)


def local(b, direction=AXIS, center=CENTER):
    """(positions, directions) of the bundle's rays in the lamp's own frame"""
    from tracer_amd.vector_manipulations import rotate_z_to_normal
    rot = rotate_z_to_normal(N.eye(3), direction)
    return N.dot(rot.T, b.get_vertices() - center), N.dot(rot.T, b.get_directions())


def ks(x, cdf_of_x=None):
    """the Kolmogorov-Smirnov distance of the sample from the distribution whose CDF at the sorted sample is given (default: U(0, 1))"""
    x = N.sort(N.ravel(x))
    Fx = x if cdf_of_x is None else cdf_of_x(x)
    n = x.size
    return max(N.abs(N.arange(1, n + 1) / float(n) - Fx).max(), N.abs(Fx - N.arange(n) / float(n)).max())


# 1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_generate_matches_the_host_build(ctx, hl, kind):
    """1e5 rays at a ray offset, tilted: positions to 1e-12 x the source's size, directions to 1e-12; the two halves at their own
    offsets are the whole"""
    m, seed, off = 100000, 17, 1000
    b = lamp(kind, m, seed, off)
    tab, n_tab = None, 0
    if kind == 'arc':
        t, g, cdf, tc, uc = b._src_table.packed()
        tab = N.ascontiguousarray(N.concatenate((t, g, cdf)))
        n_tab = t.size
        assert tc == GOLD['lobe_xs'][-1] and uc == 1. and cdf[-1] == 1.
    out = [N.empty(m) for _ in range(6)]
    hl.hl_lamp_rays(C.byref(b.source_args()[0]), _ptr(tab) if tab is not None else None, n_tab, seed, off, m, *[_ptr(o) for o in out])
    v, d = b.get_vertices(), b.get_directions()
    size = max(R_C, L_C)
    assert N.abs(v - N.array(out[:3])).max() <= 1e-12 * size
    assert N.abs(d - N.array(out[3:])).max() <= 1e-12
    assert N.array_equal(b.get_energy(), N.full(m, b.source_args()[0].energy))
    h1, h2 = lamp(kind, m // 2, seed, off), lamp(kind, m - m // 2, seed, off + m // 2)
    assert N.array_equal(N.hstack((h1.get_vertices(), h2.get_vertices())), v)
    assert N.array_equal(N.hstack((h1.get_directions(), h2.get_directions())), d)


# 2 -------------------------------------------------------------------------------------------------------------------------------
def test_distributions_of_the_arc(ctx):
    """1e6 rays: the polar angle against the exact CDF of the piecewise-linear density (quadratic within an interval); r^2, z and
    the azimuths uniform; no polar angle in the stretch without density.  KS below 1.5 x 1.36 / sqrt(n)."""
    n = 1000000
    bound = 1.5 * 1.36 / N.sqrt(n)
    for table in ('lobe', 'gap'):
        b = lamp('arc', n, 31, table=table)
        pos, d = local(b)
        xs, g = GOLD[table + '_xs'], GOLD[table + '_ys']
        mass = N.sum(0.5 * (g[:-1] + g[1:]) * N.diff(xs))
        cum = N.r_[0., N.cumsum(0.5 * (g[:-1] + g[1:]) * N.diff(xs))] / mass

        def cdf(th):
            k = N.clip(N.searchsorted(xs, th, side='right') - 1, 0, xs.size - 2)
            t = th - xs[k]
            s = (g[k + 1] - g[k]) / (xs[k + 1] - xs[k])
            return cum[k] + (g[k] * t + 0.5 * s * t * t) / mass
        th = N.arctan2(N.hypot(d[0], d[1]), d[2])
        assert ks(th, cdf) < bound
        if table == 'gap':
            assert not N.any((th > 0.9 + 1e-12) & (th < 1.3 - 1e-12))
            assert th.max() <= xs[-1] + 1e-12
    az = N.arctan2(d[1], d[0])
    assert ks((az + N.pi) / (2. * N.pi)) < bound
    assert ks((pos[0] ** 2 + pos[1] ** 2) / R_C ** 2) < bound
    assert ks(pos[2] / L_C + 0.5) < bound
    assert ks((N.arctan2(pos[1], pos[0]) + N.pi) / (2. * N.pi)) < bound
    assert (pos[0] ** 2 + pos[1] ** 2).max() <= R_C ** 2 * (1. + 1e-12) and N.abs(pos[2]).max() <= L_C / 2. * (1. + 1e-12)


@pytest.mark.parametrize('kind', KINDS[1:])
def test_distributions_of_the_emitters(ctx, kind):
    """1e6 rays: cos(theta) of the points uniform on the sphere (z and the azimuth on the wall); about the true local normal,
    sin^2 / sin^2(a) uniform for the Lambertian law, cos uniform on [cos a, 1] for the isotropic one"""
    n = 1000000
    bound = 1.5 * 1.36 / N.sqrt(n)
    what, _, law = kind.partition('-')
    ang = 0.6 if law == 'lambertian' else 1.1
    b = lamp(kind, n, 37, ang=ang)
    pos, d = local(b)
    if what == 'sphere':
        normal = pos / R_S
        assert N.abs(N.sum(normal ** 2, axis=0) - 1.).max() < 1e-9
        assert ks((normal[2] + 1.) / 2.) < bound
    else:
        normal = N.vstack((pos[0], pos[1], N.zeros(n))) / R_S
        assert N.abs(N.sum(normal ** 2, axis=0) - 1.).max() < 1e-9
        assert ks(pos[2] / L_C + 0.5) < bound
        if law == 'isotropic':
            normal = -normal        # (these are made with rays_in)
    assert ks((N.arctan2(pos[1], pos[0]) + N.pi) / (2. * N.pi)) < bound
    cos = N.sum(d * normal, axis=0)
    assert cos.min() >= N.cos(ang) - 1e-12
    if law == 'lambertian':
        assert ks(N.clip(1. - cos ** 2, 0., None) / N.sin(ang) ** 2) < bound
    else:
        assert ks((cos - N.cos(ang)) / (1. - N.cos(ang))) < bound


# 3 -------------------------------------------------------------------------------------------------------------------------------
def module_scene(reflectivity=0.9, slope_error=2.5e-3, edges=None):
    """one simulator module with its first focus at the origin, aimed along +z; a Target at the second focus; an absorbing sphere
    around all.  Surfaces: reflector, target, enclosure."""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.sphere_surface import SphericalGM
    from tracer_amd.optics_callables import Reflective
    from tracer_amd.models.solar_simulator import SimulatorReflector, Target
    edges = N.linspace(-0.1, 0.1, 9) if edges is None else edges
    refl = SimulatorReflector(A, A, C_, ZLIM, N.zeros(3), N.eye(3), reflectivity, slope_error)
    target = Target(0.2, 0.2, N.array([0., 0., 2. * F]), N.array([0., 0., -1.]), edges, edges)
    shell = AssembledObject(surfs=[Surface(geometry=SphericalGM(radius=2.), optics=Reflective(1.))], location=N.array([0., 0., F]))
    return Assembly(objects=[refl, target, shell]), target


def trace(ctx, cs, bundle, how, edges, reps=20):
    from tracer_amd.scene import DeviceScene
    dev = DeviceScene(cs, ctx)
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


@pytest.mark.parametrize('kind', KINDS)
def test_engines_agree_on_one_simulator_module(ctx, kind):
    """2e5 rays of a lamp part at the first focus: the streaming form, the megakernel, the ordered engine and the materialised bundle
    given -- the same hits per surface, absorbed energies and flux maps to 1e-9, the bundle still pending; the same with 50 rays,
    where the plan picks the megakernel, and with 64, the fewest the streaming form takes"""
    from tracer_amd.scene import compile_scene
    from tracer_amd.ray_bundle import RayBundle
    asm, target = module_scene()
    cs = compile_scene(asm)
    edges = target.binx
    for n, hows in ((200000, ('stream', 'mega', 'ordered')), (50, ('auto', 'ordered')), (64, ('stream', 'mega'))):
        mk = lambda: lamp(kind, n, 5, center=N.zeros((3, 1)), direction=N.array([0., 0., 1.]))
        m = mk()
        given = RayBundle(vertices=m.get_vertices(), directions=m.get_directions(), energy=m.get_energy())
        a_ref, h_ref, fm_ref = trace(ctx, cs, given, 'given', edges)
        # every ray ends on the target or on the enclosure (but for one that is still between the mirror's walls after `reps` hits)
        assert h_ref.sum() >= n and 0.99 * n <= h_ref[1] + h_ref[2] <= n
        if n >= 1000:
            assert h_ref[0] > 0.2 * n and h_ref[1] > 0.1 * n and fm_ref.sum() > 0.
        for how in hows:
            b = mk()
            got_a, got_h, got_fm = trace(ctx, cs, b, how, edges)
            assert b.is_pending(), how
            assert N.array_equal(got_h, h_ref), (how, n)
            assert N.allclose(got_a, a_ref, rtol=1e-9, atol=1e-12 * a_ref.max()), (how, n)
            assert N.allclose(got_fm, fm_ref, rtol=1e-9, atol=1e-12 * max(fm_ref.max(), a_ref.max())), (how, n)


# 4 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['arc', 'sphere-isotropic', 'cylinder-lambertian'])
def test_a_point_lamp_at_the_first_focus_lands_on_the_second(ctx, kind):
    """
    A lamp of size 1e-9 at the first focus of a perfect mirror (no slope error, no absorption): every ray that meets the reflector
    lands on the target within 1e-6 of the second focus.  The bound: an ellipsoid images a point at distance delta from one focus
    within M delta of the other, M = (c + f) / (c - f) = 9 here at most (the ray by the vertex: it travels c - f to the mirror and
    c + f from it), and the flat target stretches that by 1 / cos of the incidence, at most 1 / 0.8 for the rays from the rim at
    z = the centre (tan = a / f = 0.75).  delta <= 1.2e-9 (the far corner of the cylinder, the sphere's radius): 1.4e-8 at most,
    seventy times inside 1e-6; rounding in float64 is some 1e-16.  The power is conserved over the three tallies to 1e-12.
    """
    from tracer_amd.scene import compile_scene
    edges = N.array([-0.1, -1e-6, 1e-6, 0.1])
    asm, target = module_scene(reflectivity=1., slope_error=0., edges=edges)
    cs = compile_scene(asm)
    n = 200000
    scale = {'arc': 1e-9 / L_C, 'sphere': 1e-9 / R_S, 'cylinder': 1e-9 / L_C}[kind.partition('-')[0]]
    mk = lambda: lamp(kind, n, 11, center=N.zeros((3, 1)), direction=N.array([0., 0., 1.]), size=scale)
    e = mk().source_args()[0].energy
    for how in ('stream', 'mega'):
        a, h, fm = trace(ctx, cs, mk(), how, edges)
        assert h[0] > 0.2 * n
        assert a[0] == 0.
        # the rays off the mirror are those in the middle bin, 2e-6 wide; the others on the plate came straight from the lamp
        assert abs(fm[1, 1] - h[0] * e) <= 1e-9 * h[0] * e, how
        assert h[1] >= h[0] and abs(fm.sum() - a[1]) <= 1e-9 * a[1]
        assert abs(a.sum() - n * e) <= 1e-12 * n * e, how
        assert h[1] + h[2] == n


# 5 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['arc', 'sphere-lambertian', 'cylinder-isotropic'])
def test_a_spectrum_leaves_the_rays_as_they_are(ctx, kind):
    from tracer_amd.source_spectrum import SourceSpectrum
    spec = SourceSpectrum.tabulated([0.4e-6, 0.7e-6, 1.2e-6], [1., 2., 0.5])
    s, p = lamp(kind, 100000, 41, spectrum=spec), lamp(kind, 100000, 41)
    assert s.is_pending()
    assert N.array_equal(s.get_vertices(), p.get_vertices()) and N.array_equal(s.get_directions(), p.get_directions())
    wl = s.get_wavelengths()
    assert wl.shape == (100000,) and wl.min() >= 0.4e-6 and wl.max() <= 1.2e-6 and N.unique(wl).size > 90000
    # ... and traced: pending still, the tallies those of the rays without it (mirrors and absorbers do not read the wavelength)
    from tracer_amd.scene import compile_scene
    asm, target = module_scene()
    cs = compile_scene(asm)
    origin = dict(center=N.zeros((3, 1)), direction=N.array([0., 0., 1.]))
    for how in ('stream', 'mega'):
        bs, bp = lamp(kind, 20000, 43, spectrum=spec, **origin), lamp(kind, 20000, 43, **origin)
        a_s, h_s, fm_s = trace(ctx, cs, bs, how, target.binx)
        a_p, h_p, fm_p = trace(ctx, cs, bp, how, target.binx)
        assert bs.is_pending() and N.array_equal(h_s, h_p) and N.allclose(a_s, a_p, rtol=1e-9)


# 6 -------------------------------------------------------------------------------------------------------------------------------
def test_the_model(ctx):
    """two modules, a Bader and a Zhu lamp, on one target: four batches of 1e4 rays per module"""
    from tracer_amd.models.solar_simulator import SolarSimulator, Target
    from tracer_amd.ray_bundle import concatenate_rays
    cdf = N.array([N.linspace(0., N.pi, 13), 0.5 * (1. - N.cos(N.linspace(0., N.pi, 13)))]).T      # an isotropic lamp's
    aim2 = N.array([0.6, 0., 0.8])
    focus2 = N.array([0., 0., 2. * F])
    dicts = [dict(a=A, b=A, c=C_, zlim=ZLIM, lampdict=dict(model='Bader', theta_CDF=cdf)),
             dict(a=A, b=A, c=C_, zlim=ZLIM, lampdict=dict(model='Zhu'))]
    edges = N.linspace(-0.1, 0.1, 11)
    target = Target(0.2, 0.2, focus2, N.array([0., 0., -1.]), edges, edges[::2])
    sim = SolarSimulator([N.zeros(3), focus2 - 2. * F * aim2], [N.array([0., 0., 1.]), aim2], dicts, [target])
    est = sim.simulate(nrays=40000, ray_batch=10000, seed=100)
    assert est == [target.fluxmap] and est[0].n == 40000. and est[0].n2 == 4 * 1e8      # four updates of 1e4 rays
    ti = sim.get_surfaces().index(target.get_surfaces()[0])
    absorbed = sim.engine.get_tallies()[0]
    assert absorbed[ti] > 0.
    # the estimate is the mean over the batches of a batch's power per area: four batches make up the tally
    assert abs(4. * N.sum(est[0].mean * target.areas) - absorbed[ti]) <= 1e-9 * absorbed[ti]
    assert est[0].mean.shape == (10, 5) and N.all(N.isfinite(est[0].get_CI()))
    # the mirrors send theirs to the middle of the plate
    assert est[0].mean[4:6, 2].mean() > 2. * est[0].mean.mean()
    for m in sim.modules:
        parts = m.lamp.sources(10000, seed=9)
        whole = m.lamp.generate_rays(10000, seed=9)
        assert all(p.is_pending() for p in parts)
        cat = concatenate_rays(parts) if len(parts) > 1 else parts[0]
        assert N.array_equal(whole.get_vertices(), cat.get_vertices()) and N.array_equal(whole.get_directions(), cat.get_directions())
        assert N.array_equal(whole.get_energy(), cat.get_energy())
        assert abs(whole.get_energy().sum() - m.lamp.P) <= 1e-3 * m.lamp.P      # (int(n x share) rays per part)
        posed = m.fire_lamp(10000, seed=9)
        assert N.allclose(posed.get_vertices(), N.dot(m.rotation, whole.get_vertices()) + m.location[:, None], rtol=0, atol=1e-12)
        assert N.allclose(posed.get_directions(), N.dot(m.rotation, whole.get_directions()), rtol=0, atol=1e-12)


# 7 -------------------------------------------------------------------------------------------------------------------------------
def test_destroyed_table_is_an_error(ctx):
    from tracer_amd import _cabi, sources
    b = lamp('arc', 1000, 3)
    t = sources.AngleTable([0., 1., 3.], [1., 0.5, 0.1])
    b._src_desc.table = t.table_id()
    t.destroy()
    cols = [N.empty(1000) for _ in range(7)]         # (kept alive: the struct holds their addresses)
    rays = _cabi.make_rays(1000, *cols)
    with pytest.raises(_cabi.TracerAmdError) as e:
        _cabi.check(ctx.lib.trc_source_generate(ctx.handle, C.byref(b._src_desc), 1000, 3, 0, C.byref(rays)))
    assert e.value.status == _cabi.ERR_INVALID
    assert ctx.lib.trc_source_generate(ctx.handle, C.byref(b.source_args()[0]), 1000, 3, 0, C.byref(rays)) == 0
    # what trc_angle_table_create refuses
    h = C.c_void_p()
    for th, dens in (([0., 1., 3.2], [1., 1., 1.]), ([0., 2., 1.], [1., 1., 1.]), ([0., 1., 2.], [0., 0., 0.]), ([0., 1., 2.], [1., -1., 1.])):
        th, dens = N.array(th), N.array(dens)
        assert ctx.lib.trc_angle_table_create(ctx.handle, 3, _cabi.ptr(th), _cabi.ptr(dens), C.byref(h)) == _cabi.ERR_INVALID
