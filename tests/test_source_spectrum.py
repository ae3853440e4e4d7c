"""
Spectra of sources on the host (no GPU): the per-ray sampler of csrc/trc_core.h (trc_spectrum_sample), host-compiled, against
the reference's PW_linear_distribution.sample (tests/golden/source_spectra.npz, tests/golden/make_golden_spectra.py); the
packing and the checks of SourceSpectrum; the `spectrum=` keyword of the descriptor-backed sources.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = N.load(os.path.join(ROOT, 'tests', 'golden', 'source_spectra.npz'))
_p = C.POINTER(C.c_double)


@pytest.fixture(scope='module')
def hs():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_spectrum_check.so'))
    lib.hs_sizeof_spectrum.restype = C.c_long
    lib.hs_spectrum_sample.argtypes = [_p, _p, _p, C.c_int, C.c_long, _p, _p]
    return lib


def _ptr(a):
    return a.ctypes.data_as(_p)


def host_sample(hs, spectrum, u):
    wl, val, cdf = spectrum.table()
    u = N.ascontiguousarray(u, dtype=float)
    out = N.empty_like(u)
    hs.hs_spectrum_sample(_ptr(wl), _ptr(val), _ptr(cdf), wl.size, u.size, _ptr(u), _ptr(out))
    return out


@pytest.mark.parametrize('name', ['flat', 'irregular', 'planck', 'ramp'])
def test_sampler_reproduces_the_reference(hs, name):
    from tracer_amd.source_spectrum import SourceSpectrum
    xs, ys = GOLD[name + '_xs'], GOLD[name + '_ys']
    u, ref = GOLD[name + '_u'], GOLD[name + '_x']
    got = host_sample(hs, SourceSpectrum.tabulated(xs, ys), u)
    width = xs[-1] - xs[0]
    # where the reference's closed form (-b + sqrt(D)) / 2a is accurate: its rounding error is about eps (|b| + sqrt(D)) / |2a|
    a, b = GOLD[name + '_a'], GOLD[name + '_b']
    i = N.clip(N.searchsorted(GOLD[name + '_cdf'], u, side='right') - 1, 0, xs.size - 2)
    with N.errstate(divide='ignore', invalid='ignore'):
        D = b[i] ** 2 + 4. * a[i] * (u - GOLD[name + '_cdf'][i] + a[i] * xs[i] ** 2 + b[i] * xs[i])
        ref_err = N.where(a[i] != 0., 8. * N.finfo(float).eps * (N.abs(b[i]) + N.sqrt(N.abs(D))) / N.abs(2. * a[i]), 0.)
    accurate = ref_err < 1e-13 * width
    assert accurate.mean() > 0.5
    err = N.abs(got - ref)
    assert N.all(err[accurate] <= 1e-12 * width), (name, err[accurate].max() / width)
    # every sample, accurate reference or not, lies in an interval of positive mass
    assert N.all((got >= xs[0]) & (got <= xs[-1]))


def test_no_sample_in_a_zero_density_stretch(hs):
    from tracer_amd.source_spectrum import SourceSpectrum
    xs, ys = GOLD['irregular_xs'], GOLD['irregular_ys']
    u = N.random.RandomState(3).uniform(size=200000)
    got = host_sample(hs, SourceSpectrum.tabulated(xs, ys), u)
    for k in range(xs.size - 1):
        if ys[k] == 0. and ys[k + 1] == 0.:
            assert not N.any((got > xs[k]) & (got < xs[k + 1]))


def test_sampler_edges(hs):
    """u = 0 gives the first point of positive mass; u just below 1 the end of the band; a flat band is the linear map"""
    from tracer_amd.source_spectrum import SourceSpectrum
    s = SourceSpectrum.tabulated([1., 2., 3., 4.], [0., 0., 1., 1.])
    got = host_sample(hs, s, N.array([0., 1. - 2. ** -53]))
    assert got[0] == 2. and abs(got[1] - 4.) < 1e-12
    flat = SourceSpectrum.uniform(0.3e-6, 2.5e-6)
    u = N.linspace(0., 0.999, 7)
    assert N.allclose(host_sample(hs, flat, u), 0.3e-6 + u * 2.2e-6, rtol=0, atol=1e-21)


def test_packing_cdf_is_the_trapezoid_integral():
    from tracer_amd.source_spectrum import SourceSpectrum
    xs, ys = GOLD['irregular_xs'] * 1e-6, GOLD['irregular_ys'] * 3.7
    wl, val, cdf = SourceSpectrum.tabulated(xs, ys).table()
    integ = N.concatenate(([0.], N.cumsum((xs[1:] - xs[:-1]) * (ys[1:] + ys[:-1]) / 2.)))
    assert cdf[0] == 0. and cdf[-1] == 1.
    assert N.allclose(cdf, integ / N.trapezoid(ys, xs) if hasattr(N, 'trapezoid') else integ / N.trapz(ys, xs), rtol=1e-14, atol=1e-15)
    assert N.allclose(val, ys / integ[-1], rtol=1e-15)


def test_planck_matches_the_reference():
    from tracer_amd.source_spectrum import SourceSpectrum, planck
    T, band, step = float(GOLD['planck_T']), tuple(GOLD['planck_band']), float(GOLD['planck_step'])
    s = SourceSpectrum.planck(T, band, step=step)
    assert N.array_equal(s.wavelengths, GOLD['planck_wl'])
    assert N.allclose(s.values, GOLD['planck_val'], rtol=1e-14, atol=0)
    assert N.allclose(planck(GOLD['planck_wl'], T), GOLD['planck_val'], rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match='larger step'):
        SourceSpectrum.planck(T, (0.3e-6, 10e-6), step=1e-9)


@pytest.mark.parametrize('args', [
    ([0.5], [1.]),                          # one point
    ([0.5, 0.4], [1., 1.]),                 # not increasing
    ([0.4, 0.4], [1., 1.]),                 # repeated
    ([0.4, 0.5], [1., -1.]),                # negative
    ([0.4, 0.5], [1., N.nan]),              # not finite
    ([0.4, N.inf], [1., 1.]),
    ([0.4, 0.5], [0., 0.]),                 # zero integral
    ([0.4, 0.5, 0.6], [1., 1.]),            # lengths differ
    (N.linspace(1., 2., 4097), N.ones(4097)),     # too many points
])
def test_invalid_tables_raise(args):
    from tracer_amd.source_spectrum import SourceSpectrum
    with pytest.raises(ValueError):
        SourceSpectrum.tabulated(*args)


def test_invalid_other_inputs_raise():
    from tracer_amd.source_spectrum import SourceSpectrum
    for bad in (lambda: SourceSpectrum.monochromatic(N.nan), lambda: SourceSpectrum.monochromatic(1e-6, ref_index=0.),
                lambda: SourceSpectrum.uniform(2e-6, 1e-6), lambda: SourceSpectrum.uniform(1e-6, 2e-6, ref_index=N.inf),
                lambda: SourceSpectrum.planck(-1., (1e-6, 2e-6)), lambda: SourceSpectrum.planck(5000., (2e-6, 1e-6))):
        with pytest.raises(ValueError):
            bad()


def test_ctypes_struct_has_the_compilers_size(hs):
    from tracer_amd import _cabi
    assert hs.hs_sizeof_spectrum() == C.sizeof(_cabi.SourceSpectrumDesc) == 40


def test_desc_packs_the_table():
    from tracer_amd import _cabi
    from tracer_amd.source_spectrum import SourceSpectrum
    s = SourceSpectrum.tabulated([1e-6, 2e-6, 3e-6], [0., 1., 0.5], ref_index=1.5)
    d = s.desc()
    assert (d.kind, d.n, d.ref_index) == (_cabi.SPECTRUM_TABLE, 3, 1.5)
    assert [d.wl[i] for i in range(3)] == [1e-6, 2e-6, 3e-6] and [d.value[i] for i in range(3)] == [0., 1., 0.5]
    m = SourceSpectrum.monochromatic(5e-7).desc()
    assert (m.kind, m.wavelength, m.ref_index) == (_cabi.SPECTRUM_CONSTANT, 5e-7, 1.)


def test_sources_take_a_spectrum_and_stay_pending():
    from tracer_amd import sources
    from tracer_amd.source_spectrum import SourceSpectrum
    spec = SourceSpectrum.uniform(0.3e-6, 2.5e-6)
    b = sources.buie_sunshape(1000, N.zeros(3), N.array([0., 0., -1.]), 1., 0.02, flux=1000., spectrum=spec, seed=5)
    assert b.is_pending() and b.source_spectrum() is spec
    b = sources.oblique_solar_rect_bundle(1000, N.zeros(3), N.array([0., 0., -1.]), N.array([0., 0., -1.]), 1., 1., 4.65e-3,
                                          flux=1000., wavelength=5e-7, ref_index=1.2, seed=5)
    assert b.is_pending()
    assert b.source_spectrum().wavelength == 5e-7 and b.source_spectrum().ref_index == 1.2
    for make in (lambda s: sources.disk_bundle(10, N.zeros(3), N.array([0, 0, 1.]), 1., 0.01, spectrum=s),
                 lambda s: sources.solar_disk_bundle(10, N.zeros(3), N.array([0, 0, 1.]), 1., 0.01, spectrum=s),
                 lambda s: sources.rect_bundle(10, N.zeros(3), N.array([0, 0, 1.]), 1., 1., 0.01, spectrum=s),
                 lambda s: sources.triangular_bundle(10, [0, 0, 0], [1, 0, 0], [0, 1, 0], spectrum=s),
                 lambda s: sources.rect_buie_sunshape(10, N.zeros(3), N.array([0, 0, 1.]), 1., 1., 0.02, flux=1., spectrum=s),
                 lambda s: sources.vf_cylinder_bundle(10, 1., 1., N.zeros(3), N.array([0, 0, 1.]), spectrum=s),
                 lambda s: sources.vf_frustum_bundle(10, 1., 0.5, 1., N.zeros(3), N.array([0, 0, 1.]), spectrum=s)):
        assert make(spec).is_pending()
    with pytest.raises(TypeError):
        sources.rect_bundle(10, N.zeros(3), N.array([0, 0, 1.]), 1., 1., 0.01, spectrum=5e-7)
    with pytest.raises(ValueError):
        sources.oblique_solar_rect_bundle(10, N.zeros(3), N.array([0., 0., -1.]), N.array([0., 0., -1.]), 1., 1., 0.01,
                                          wavelength=5e-7, spectrum=spec)


def test_draws_next_to_interval_ends_are_finite(hs):
    """uniforms within a few ulps of every CDF entry (densities falling to zero at an interval's end make the discriminant of the
    root round towards, and below, zero there) give finite wavelengths inside the band"""
    from tracer_amd.source_spectrum import SourceSpectrum
    for name in ('irregular', 'planck', 'ramp'):
        s = SourceSpectrum.tabulated(GOLD[name + '_xs'] * 1e-6, GOLD[name + '_ys'])
        wl, val, cdf = s.table()
        u = cdf[:, None] + N.arange(-8, 9)[None, :] * N.spacing(cdf)[:, None]
        u = u[(u >= 0.) & (u < 1.)]
        got = host_sample(hs, s, u)
        assert N.all(N.isfinite(got)) and N.all((got >= wl[0]) & (got <= wl[-1])), name
