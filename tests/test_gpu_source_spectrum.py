"""
Spectra of sources on the device: wavelengths drawn from the spectrum attached to a source descriptor (trc_source_generate_x,
trc_trace_fast_x, trc_trace_ordered_x; SourceSpectrum and the `spectrum=` keyword of the sources).
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = N.load(os.path.join(ROOT, 'tests', 'golden', 'source_spectra.npz'))
_p = C.POINTER(C.c_double)


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


@pytest.fixture(scope='module')
def hs():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_spectrum_check.so'))
    lib.hs_spectrum_draw.argtypes = [_p, _p, _p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_long, _p, _p]
    return lib


def irregular(scale=1e-6):
    from tracer_amd.source_spectrum import SourceSpectrum
    return SourceSpectrum.tabulated(GOLD['irregular_xs'] * scale, GOLD['irregular_ys'])


def every_source(n, seed, spectrum):
    from tracer_amd import sources
    z = N.array([0., 0., 1.])
    return [
        sources.disk_bundle(n, N.c_[[0., 0., 1.]], z, 1., 0.01, radius_in=0.2, x_cut=0.3, seed=seed, ray_offset=7, spectrum=spectrum),
        sources.rect_bundle(n, N.c_[[0., 1., 0.]], z, 1., 2., 0.02, flux=10., seed=seed, spectrum=spectrum),
        sources.buie_sunshape(n, N.c_[[0., 0., 2.9]], -z, 2.5, 0.05, flux=1000., seed=seed, ray_offset=11, spectrum=spectrum),
        sources.rect_buie_sunshape(n, N.c_[[0., 0., 2.9]], -z, 2., 1., 0.02, flux=1000., seed=seed, spectrum=spectrum),
        sources.triangular_bundle(n, [0, 0, 0], [1, 0, 0], [0, 1, 0], seed=seed, spectrum=spectrum),
        sources.vf_cylinder_bundle(n, 1., 2., N.zeros(3), z, flux=3., seed=seed, spectrum=spectrum),
        sources.vf_frustum_bundle(n, 1., 0.5, 1., N.zeros(3), z, flux=3., seed=seed, spectrum=spectrum),
    ]


def test_draws_leave_the_rays_as_they_are(ctx, hs):
    from tracer_amd.source_spectrum import SourceSpectrum
    n, seed = 20000, 4242
    spec = SourceSpectrum.tabulated(GOLD['planck_xs'] * 1e-6, GOLD['planck_ys'], ref_index=1.25)
    with_spec, without = every_source(n, seed, spec), every_source(n, seed, None)
    assert sorted(b.source_args()[0].kind for b in with_spec) == list(range(7))
    wl, val, cdf = spec.table()
    for a, b in zip(with_spec, without):
        assert a.is_pending()
        for col in ('vertices', 'directions', 'energy'):
            assert N.array_equal(getattr(a, 'get_' + col)(), getattr(b, 'get_' + col)()), (a.source_args()[0].kind, col)
        off = a.source_args()[3]
        want = N.empty(n)
        hs.hs_spectrum_draw(wl.ctypes.data_as(_p), val.ctypes.data_as(_p), cdf.ctypes.data_as(_p), wl.size, seed, off, n, None,
                            want.ctypes.data_as(_p))
        got = a.get_wavelengths()
        assert N.allclose(got, want, rtol=1e-12, atol=0)
        assert N.all(a.get_ref_index() == 1.25)


def test_distribution_of_ten_million_draws(ctx):
    from tracer_amd import sources
    spec = irregular()
    n = 10 ** 7
    b = sources.rect_bundle(n, N.c_[[0., 0., 0.]], N.array([0., 0., 1.]), 1., 1., 0., seed=77, spectrum=spec)
    x = N.sort(b.get_wavelengths())
    wl, val, cdf = spec.table()
    i = N.clip(N.searchsorted(wl, x, side='right') - 1, 0, wl.size - 2)
    p = val[i] + (val[i + 1] - val[i]) * (x - wl[i]) / (wl[i + 1] - wl[i])
    F = cdf[i] + (x - wl[i]) * (val[i] + p) / 2.
    k = N.arange(1, n + 1) / float(n)
    ks = max(N.max(N.abs(F - k)), N.max(N.abs(F - (k - 1. / n))))
    assert ks < 3. / N.sqrt(n), ks
    for j in range(wl.size - 1):
        if val[j] == 0. and val[j + 1] == 0.:
            assert not N.any((x > wl[j]) & (x < wl[j + 1]))


def _cavity_trace(ctx, ts, bundle, how, reps=12, seed=9):
    # (a pending source bundle is traced with its own seed: the given bundle gets the same one)
    from tracer_amd.scene import DeviceScene
    dev = DeviceScene(ts, ctx)
    e0 = bundle.source_args()[0].energy if how != 'given' else bundle.get_energy()[0]
    if how == 'ordered':
        res, st = dev.trace_ordered(bundle, reps, 1e-3 * e0, seed)
        res.close()
    else:
        st, _ = dev.trace_fast(bundle, reps, 1e-3 * e0, seed, stream={'stream': True, 'mega': False, 'given': True}[how])
    a, r, h = dev.get_tallies()
    dev.close()
    return a.copy(), h.copy()


@pytest.mark.parametrize('n,hows', [(200000, ('stream', 'mega', 'ordered')), (20000000, ('stream',))])
def test_engines_agree_on_the_spectral_cavity(ctx, n, hows):
    """the central test: a Buie source with a table spectrum into the cavity of wavelength-tabulated optics, traced fused (streaming
    form, megakernel, ordered engine) and as the materialised bundle of today's path -- the same hits, the same energies"""
    from tracer_amd import scenes
    from tracer_amd.ray_bundle import RayBundle
    ts, src = scenes.dish_cavity()
    spec = irregular()
    b = scenes.dish_source(n, src, seed=9, spectrum=spec)
    m = scenes.dish_source(n, src, seed=9, spectrum=spec)
    given = RayBundle(vertices=m.get_vertices(), directions=m.get_directions(), energy=m.get_energy(), wavelengths=m.get_wavelengths())
    a_ref, h_ref = _cavity_trace(ctx, ts, given, 'given')
    assert h_ref[1:].sum() > 0
    for how in hows:
        bb = scenes.dish_source(n, src, seed=9, spectrum=spec)
        a, h = _cavity_trace(ctx, ts, bb, how)
        assert bb.is_pending()
        assert N.array_equal(h, h_ref), how
        assert N.allclose(a, a_ref, rtol=1e-9, atol=1e-12 * a_ref.max()), how


def _plate_scene(absorptance_wl, absorptance):
    from tracer_amd.surface import Surface
    from tracer_amd.object import AssembledObject
    from tracer_amd.assembly import Assembly
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.spatial_geometry import rotx, translate
    from tracer_amd import optics_callables as opt
    plate_opt = opt.Reflective_spectral(absorptance, absorptance_wl)
    plate = AssembledObject(surfs=[Surface(RectPlateGM(2., 2.), plate_opt)])
    rec_opt = opt.LambertianReceiver(1.)
    rec = AssembledObject(surfs=[Surface(RectPlateGM(6., 6.), rec_opt)], transform=N.dot(translate(0., 0., 2.), rotx(N.pi)))
    return Assembly(objects=[plate, rec]), rec_opt


LAM0 = 1e-6
ABS_WL = N.array([0.3e-6, 0.95e-6, 1.05e-6, 2.5e-6])
ABS = N.array([1., 1., 0., 0.])


def _plate_source(n, spectrum, seed=21):
    from tracer_amd import sources
    return sources.rect_bundle(n, N.c_[[0., 0., 1.]], N.array([0., 0., -1.]), 1., 1., 1e-3, flux=1000., seed=seed, spectrum=spectrum)


def test_known_answer_of_a_spectrally_selective_plate(ctx):
    from tracer_amd.tracer_engine import TracerEngine
    from tracer_amd.source_spectrum import SourceSpectrum
    n = 2000000
    spec = irregular()
    asm, _ = _plate_scene(ABS_WL, ABS)
    eng = TracerEngine(asm)
    b = _plate_source(n, spec)
    e_in = b.source_args()[0].energy * n
    eng.ray_tracer(b, reps=5, min_energy=1e-12, tree=False)
    a, r, h = eng.get_tallies()
    ratio = a[0] / e_in
    # the same on the host: integral of p(lambda) a(lambda), both piecewise linear (fine grid, trapezoid)
    wl, val, cdf = spec.table()
    x = N.linspace(wl[0], wl[-1], 2000001)
    p = N.interp(x, wl, val)
    want = N.trapezoid(p * N.interp(x, ABS_WL, ABS), x) if hasattr(N, 'trapezoid') else N.trapz(p * N.interp(x, ABS_WL, ABS), x)
    sigma = N.sqrt(want * (1. - want) / n)
    assert abs(ratio - want) < 3. * sigma + 1e-9, (ratio, want, sigma)
    for lam, expect in ((0.5e-6, 1.), (2.e-6, 0.)):
        eng = TracerEngine(_plate_scene(ABS_WL, ABS)[0])
        b = _plate_source(200000, SourceSpectrum.monochromatic(lam))
        eng.ray_tracer(b, reps=5, min_energy=1e-12, tree=False)
        a, r, h = eng.get_tallies()
        assert abs(a[0] / (b.source_args()[0].energy * 200000) - expect) < 1e-12


def test_public_entry_point_tree_and_fast(ctx):
    from tracer_amd.tracer_engine import TracerEngine
    from tracer_amd import sources
    n = 100000
    spec = irregular()
    out = {}
    for tree in (True, False):
        asm, rec_opt = _plate_scene(ABS_WL, ABS)
        eng = TracerEngine(asm)
        b = _plate_source(n, spec, seed=5)
        eng.ray_tracer(b, reps=5, min_energy=1e-12, tree=tree, seed=5)
        if tree:
            lvl0 = eng.tree._bunds[0].get_wavelengths()
            assert N.array_equal(lvl0, _plate_source(n, spec, seed=5).get_wavelengths())
            assert eng.tree._bunds[1].get_wavelengths().shape[0] == eng.tree._bunds[1].get_num_rays()
        a, r, h = eng.get_tallies()
        hits = rec_opt.get_all_hits()
        out[tree] = (a.copy(), h.copy(), N.sort(N.ravel(N.asarray(hits[0], dtype=float))))
    assert N.array_equal(out[True][1], out[False][1])
    assert N.allclose(out[True][0], out[False][0], rtol=1e-9)
    assert N.allclose(out[True][2], out[False][2], rtol=1e-12)
    # oblique_solar_rect_bundle(wavelength=, ref_index=): pending, and its fused trace equals the trace of its materialised copy
    mk = lambda: sources.oblique_solar_rect_bundle(n, N.c_[[0., 0., 1.]], N.array([0., 0., -1.]), N.array([0.1, 0., -1.]) / N.sqrt(1.01),
                                                   1., 1., 1e-3, flux=1000., wavelength=0.7e-6, ref_index=1.0, seed=8)
    b = mk()
    assert b.is_pending()
    res = []
    for bundle in (b, mk()):
        if bundle is not b:
            assert N.all(bundle.get_wavelengths() == 0.7e-6) and N.all(bundle.get_ref_index() == 1.0)
            assert not bundle.is_pending()
        eng = TracerEngine(_plate_scene(ABS_WL, ABS)[0])
        eng.ray_tracer(bundle, reps=5, min_energy=1e-12, tree=False, seed=8)
        res.append(eng.get_tallies())
    assert N.array_equal(res[0][2], res[1][2])
    assert N.allclose(res[0][0], res[1][0], rtol=1e-12)


def test_spectrum_with_a_given_bundle_is_invalid(ctx):
    from tracer_amd import _cabi, scenes
    from tracer_amd.scene import DeviceScene
    ts, src = scenes.dish_cavity()
    dev = DeviceScene(ts, ctx)
    spec = irregular()
    x = N.zeros(4)
    rays = _cabi.make_rays(4, x, x, x, x, x, x + 1., x + 1.)
    st = dev.lib.trc_trace_fast_x(dev.handle, C.byref(rays), None, C.byref(spec.desc()), 4, 1, 0., 1, 0, 0, None, None)
    assert st == _cabi.ERR_INVALID
    bad = _cabi.SourceSpectrumDesc()
    bad.kind, bad.n, bad.ref_index = _cabi.SPECTRUM_TABLE, 1, 1.
    desc = scenes.dish_source(4, src, seed=1).source_args()[0]
    st = dev.lib.trc_trace_fast_x(dev.handle, None, C.byref(desc), C.byref(bad), 4, 1, 0., 1, 0, 0, None, None)
    assert st == _cabi.ERR_INVALID and b'points' in dev.lib.trc_last_error()
    dev.close()
