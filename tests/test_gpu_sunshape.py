"""
Tabulated sunshapes on the device: the rays of tabulated_sunshape / rect_tabulated_sunshape as trc_source_generate makes them,
against the host build of the same per-ray code and against the Buie sources; their distribution; the engines' agreement.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = N.load(os.path.join(ROOT, 'tests', 'golden', 'sunshape.npz'))
_p = C.POINTER(C.c_double)
TH0 = N.linspace(0., 4.65e-3, 211)
I0 = N.cos(0.326 * TH0 * 1e3) / N.cos(0.308 * TH0 * 1e3)          # the Buie CSR-0 nodes (sources.py:338-341)


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


@pytest.fixture(scope='module')
def hs():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_sunshape_check.so'))
    lib.hs_sunshape_rays.argtypes = [C.c_void_p, _p, C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_long] + [_p] * 6
    return lib


def _ptr(a):
    return a.ctypes.data_as(_p)


def _src(kind, n, angles, intensity, seed, offset=0, spectrum=None):
    from tracer_amd import sources
    d = N.r_[0.1, -0.2, -1.] / N.linalg.norm([0.1, -0.2, -1.])
    if kind == 'disc':
        return sources.tabulated_sunshape(n, N.c_[[1., 2., 30.]], d, 4., angles, intensity, flux=900., seed=seed, ray_offset=offset,
                                          spectrum=spectrum)
    return sources.rect_tabulated_sunshape(n, N.c_[[1., 2., 30.]], d, 4., 3., angles, intensity, flux=900., seed=seed,
                                           ray_offset=offset, spectrum=spectrum)


@pytest.mark.parametrize('kind', ['disc', 'rect'])
def test_generate_matches_the_host_build(ctx, hs, kind):
    a, I = GOLD['buie05_angles'], GOLD['buie05_intensity']
    m = 200000
    b = _src(kind, m, a, I, seed=17, offset=1000)
    t, g, cdf, tc, uc = b._src_table.packed()
    tab = N.ascontiguousarray(N.concatenate((t, g, cdf)))
    out = [N.empty(m) for _ in range(6)]
    hs.hs_sunshape_rays(C.addressof(b.source_args()[0]), _ptr(tab), a.size, tc, uc, 17, 1000, m, *[_ptr(o) for o in out])
    v, d = b.get_vertices(), b.get_directions()
    assert N.abs(v - N.array(out[:3])).max() <= 1e-12 * 30.
    assert N.abs(d - N.array(out[3:])).max() <= 1e-12


@pytest.mark.parametrize('kind', ['disc', 'rect'])
def test_buie_nodes_reproduce_the_buie_source(ctx, kind):
    from tracer_amd import sources
    n = 1000000
    d = N.r_[0.1, -0.2, -1.] / N.linalg.norm([0.1, -0.2, -1.])
    t = _src(kind, n, TH0, I0, seed=23)
    if kind == 'disc':
        b = sources.buie_sunshape(n, N.c_[[1., 2., 30.]], d, 4., 0., flux=900., seed=23)
    else:
        b = sources.rect_buie_sunshape(n, N.c_[[1., 2., 30.]], d, 4., 3., 0., flux=900., seed=23)
    assert N.array_equal(t.get_vertices(), b.get_vertices())
    assert N.array_equal(t.get_energy(), b.get_energy())
    # the angle between two unit vectors is their chord to first order (arccos of their dot product is blind below 1e-8)
    chord = N.sqrt(N.sum((t.get_directions() - b.get_directions()) ** 2, axis=0))
    assert chord.max() < 1e-12


def _thetas(b):
    from tracer_amd.spatial_geometry import rotation_to_z
    d = b.get_directions()
    R = rotation_to_z(N.r_[0.1, -0.2, -1.] / N.linalg.norm([0.1, -0.2, -1.]))
    loc = N.dot(R.T, d)
    return N.arctan2(N.hypot(loc[0], loc[1]), loc[2])


def test_distributions(ctx):
    n = 10000000
    a, I = GOLD['buie05_angles'], GOLD['buie05_intensity']
    b = _src('disc', n, a, I, seed=31)
    th = N.sort(_thetas(b))
    g = I * N.cos(a) * N.sin(a)
    cum = N.r_[0., N.cumsum(0.5 * (g[:-1] + g[1:]) * N.diff(a))]
    cum /= cum[-1]
    # the CDF of a piecewise-linear density, exactly: within interval k, F = cum_k + g_k t + s t^2 / 2
    k = N.clip(N.searchsorted(a, th, side='right') - 1, 0, a.size - 2)
    t = th - a[k]
    s = (g[k + 1] - g[k]) / (a[k + 1] - a[k])
    F = cum[k] + (g[k] * t + 0.5 * s * t * t) / N.sum(0.5 * (g[:-1] + g[1:]) * N.diff(a))
    emp_hi = N.arange(1, n + 1) / float(n)
    ks = max(N.abs(emp_hi - F).max(), N.abs(F - (emp_hi - 1. / n)).max())
    assert ks < 1.5 * 1.36 / N.sqrt(n), ks
    # the 2-point constant table is the pillbox: P(theta < x) = sin^2 x / sin^2 a
    ang = 4.65e-3
    th = N.sort(_thetas(_src('rect', n // 4, [0., ang], [1., 1.], seed=37)))
    m = th.size
    F = N.sin(th) ** 2 / N.sin(ang) ** 2
    ks = max(N.abs(N.arange(1, m + 1) / float(m) - F).max(), N.abs(F - N.arange(m) / float(m)).max())
    assert ks < 1.5 * 1.36 / N.sqrt(m), ks
    assert th.max() <= ang * (1. + 1e-15)


def _nsttf_trace(ctx, cs, bundle, how, reps=12):
    from tracer_amd.scene import DeviceScene
    dev = DeviceScene(cs, ctx)
    e0 = bundle.source_args()[0].energy if how != 'given' else bundle.get_energy()[0]
    if how == 'ordered':
        res, st = dev.trace_ordered(bundle, reps, 1e-3 * e0, 5)
        res.close()
    else:
        st, _ = dev.trace_fast(bundle, reps, 1e-3 * e0, 5, stream={'stream': True, 'fresh0': True, 'mega': False, 'given': True}[how])
    a, r, h = dev.get_tallies()
    dev.close()
    return a.copy(), h.copy()


def test_engines_agree_on_nsttf(ctx):
    """NSTTF under the 437-point table: the streaming form (footprint map and the general path; the general path alone), the
    megakernel, the ordered engine and the materialised bundle traced as a given one -- the same hits, the same energies"""
    from tracer_amd import scenes, sources
    from tracer_amd.scene import compile_scene
    from tracer_amd.ray_bundle import RayBundle
    plant, field, rec, src = scenes.nsttf_field()
    cs = compile_scene(plant)
    a, I = GOLD['buie05_angles'], GOLD['buie05_intensity']
    n = 2000000
    mk = lambda: sources.tabulated_sunshape(n, src['center'], src['direction'], src['radius'], a, I, flux=src['flux'], seed=5)
    m = mk()
    given = RayBundle(vertices=m.get_vertices(), directions=m.get_directions(), energy=m.get_energy())
    a_ref, h_ref = _nsttf_trace(ctx, cs, given, 'given')
    assert h_ref.sum() > 0.01 * n
    for how in ('stream', 'fresh0', 'mega', 'ordered'):
        b = mk()
        env = {'fresh0': ('TRC_STREAM_FRESH', '0')}.get(how)
        if env:
            os.environ[env[0]] = env[1]
        try:
            got_a, got_h = _nsttf_trace(ctx, cs, b, how)
        finally:
            if env:
                del os.environ[env[0]]
        assert b.is_pending()
        assert N.array_equal(got_h, h_ref), how
        assert N.allclose(got_a, a_ref, rtol=1e-9, atol=1e-12 * a_ref.max()), how


def test_spectrum_leaves_the_rays_as_they_are(ctx):
    from tracer_amd.source_spectrum import SourceSpectrum
    a, I = GOLD['buie05_angles'], GOLD['buie05_intensity']
    spec = SourceSpectrum.tabulated([0.4e-6, 0.7e-6, 1.2e-6], [1., 2., 0.5])
    for kind in ('disc', 'rect'):
        s = _src(kind, 100000, a, I, seed=41, spectrum=spec)
        p = _src(kind, 100000, a, I, seed=41)
        assert s.is_pending()
        assert N.array_equal(s.get_vertices(), p.get_vertices()) and N.array_equal(s.get_directions(), p.get_directions())
        wl = s.get_wavelengths()
        assert wl.shape == (100000,) and wl.min() >= 0.4e-6 and wl.max() <= 1.2e-6 and N.unique(wl).size > 90000


def test_public_entry_point_tree_and_fast(ctx):
    from tracer_amd import scenes, sources
    from tracer_amd.tracer_engine import TracerEngine
    asm, dish_surf, rec_surf, dsrc = scenes.dish()
    a, I = GOLD['buie05_angles'], GOLD['buie05_intensity']
    out = {}
    for tree in (True, False):
        asm, dish_surf, rec_surf, dsrc = scenes.dish()
        eng = TracerEngine(asm)
        b = sources.tabulated_sunshape(200000, dsrc['center'], dsrc['direction'], dsrc['radius'], a, I, flux=dsrc['flux'], seed=7)
        eng.ray_tracer(b, reps=8, min_energy=1e-12, tree=tree, seed=7)
        ab, r, h = eng.get_tallies()
        out[tree] = (ab.copy(), h.copy())
    assert out[True][1].sum() > 100000
    assert N.array_equal(out[True][1], out[False][1])
    assert N.allclose(out[True][0], out[False][0], rtol=1e-9)


def test_destroyed_table_is_an_error(ctx):
    from tracer_amd import _cabi, sources
    b = _src('disc', 1000, [0., 0.004, 0.006], [1., 0.5, 0.1], seed=3)
    t = sources.SunshapeTable([0., 0.004, 0.006], [1., 0.5, 0.1])
    b._src_desc.table = t.table_id()
    t.destroy()
    cols = [N.empty(1000) for _ in range(7)]         # (kept alive: the struct holds their addresses)
    rays = _cabi.make_rays(1000, *cols)
    with pytest.raises(_cabi.TracerAmdError) as e:
        _cabi.check(ctx.lib.trc_source_generate(ctx.handle, C.byref(b._src_desc), 1000, 3, 0, C.byref(rays)))
    assert e.value.status == _cabi.ERR_INVALID
    assert ctx.lib.trc_source_generate(ctx.handle, C.byref(b.source_args()[0]), 1000, 3, 0, C.byref(rays)) == 0
