"""
Tabulated sunshapes on the host (no GPU): the host sampler sunshape_to_ray_directions against the reference
(tests/golden/sunshape.npz, tests/golden/make_golden_sunshape.py); the device's polar-angle sampler (csrc/trc_core.h,
trc_sunshape_theta), host-compiled, against the reference's angles; the packing and the core / tail split; the checks; the
descriptor-backed sources; the footprint map of the two new kinds.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = N.load(os.path.join(ROOT, 'tests', 'golden', 'sunshape.npz'))
NAMES = sorted(str(n) for n in GOLD['names'])
_p = C.POINTER(C.c_double)


@pytest.fixture(scope='module')
def hs():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_sunshape_check.so'))
    lib.hs_sizeof_source_desc.restype = C.c_long
    lib.hs_sunshape_pack.restype = C.c_int
    lib.hs_sunshape_pack.argtypes = [C.c_int, _p, _p, _p, _p, _p]
    lib.hs_sunshape_theta.argtypes = [_p, C.c_int, C.c_long, _p, _p]
    lib.hs_sunshape_rays.argtypes = [C.c_void_p, _p, C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_long] + [_p] * 6
    lib.hs_sunshape_u2.argtypes = [C.c_uint64, C.c_uint64, C.c_long, _p]
    return lib


def _ptr(a):
    return a.ctypes.data_as(_p)


def pack(hs, angles, intensity):
    a = N.ascontiguousarray(angles, dtype=float)
    I = N.ascontiguousarray(intensity, dtype=float)
    tab = N.empty(3 * a.size)
    tc, uc = C.c_double(), C.c_double()
    assert hs.hs_sunshape_pack(a.size, _ptr(a), _ptr(I), _ptr(tab), C.byref(tc), C.byref(uc)) == 1
    return tab, tc.value, uc.value


def theta_of(hs, tab, u):
    n = tab.size // 3
    u = N.ascontiguousarray(u, dtype=float)
    out = N.empty_like(u)
    hs.hs_sunshape_theta(_ptr(tab), n, u.size, _ptr(u), _ptr(out))
    return out


def test_host_sampler_reproduces_the_reference():
    from tracer_amd import sources
    for k, name in enumerate(NAMES):
        N.random.seed(2000 + k)
        with N.errstate(divide='ignore', invalid='ignore'):
            d = sources.sunshape_to_ray_directions(GOLD[name + '_angles'], GOLD[name + '_intensity'], GOLD[name + '_R'].size)
        assert N.abs(d - GOLD[name + '_dir']).max() <= 1e-15, name


def test_compat_exposes_the_host_sampler():
    from tracer_amd import compat, sources
    compat.install()
    import tracer.sources
    assert tracer.sources.sunshape_to_ray_directions is sources.sunshape_to_ray_directions
    assert tracer.sources.tabulated_sunshape is sources.tabulated_sunshape


@pytest.mark.parametrize('name', NAMES)
def test_device_theta_sampler_reproduces_the_reference(hs, name):
    a, I = GOLD[name + '_angles'], GOLD[name + '_intensity']
    R, d, cdf = GOLD[name + '_R'], GOLD[name + '_dir'], GOLD[name + '_cdf']
    ref = N.arctan2(N.hypot(d[0], d[1]), d[2])
    tab, _, _ = pack(hs, a, I)
    got = theta_of(hs, tab, R)
    width = a[-1] - a[0]
    # where the reference's closed form -(-A t1 + B t0 + sqrt(D)) / (A - B) is accurate: its rounding error is about
    # eps (|A t1| + |B t0| + sqrt(D)) / |A - B| (the A == B branch is a linear map)
    g = I * N.cos(a) * N.sin(a)
    i = N.clip(N.searchsorted(cdf, R, side='right') - 1, 0, a.size - 2)
    A, B, t0, t1 = g[i], g[i + 1], a[i], a[i + 1]
    with N.errstate(divide='ignore', invalid='ignore'):
        D = ((t0 - t1) * A) ** 2 + 2. * N.sum(0.5 * (g[:-1] + g[1:]) * N.diff(a)) * (R - cdf[i]) * (t1 - t0) * (B - A)
        ref_err = N.where(A != B, 8. * N.finfo(float).eps * (N.abs(A * t1) + N.abs(B * t0) + N.sqrt(N.abs(D))) / N.abs(A - B), 0.)
    # (draws at or beyond the reference's CDF[-1] keep theta = 0 there); the reference's angle from its direction: a few ulp of theta
    inside = R < cdf[-1]
    accurate = inside & (ref_err < 1e-12 * width)
    assert accurate.mean() > 0.5
    err = N.abs(got - ref)
    assert N.all(err[accurate] <= 1e-12 * width + 4e-16 * ref[accurate]), (name, (err[accurate] / width).max())
    # elsewhere within the reference's own rounding error
    assert N.all(err[inside] <= 1e-12 * width + 2. * ref_err[inside] + 4e-16 * ref[inside]), name
    # every sample lies in an interval of positive mass
    assert N.all((got >= a[0]) & (got <= a[-1]))
    for k in range(a.size - 1):
        if g[k] == 0. and g[k + 1] == 0.:
            assert not N.any((got > a[k]) & (got < a[k + 1])), (name, k)


def test_no_sample_in_a_zero_mass_stretch(hs):
    a, I = GOLD['irregular_angles'], GOLD['irregular_intensity']
    tab, _, _ = pack(hs, a, I)
    got = theta_of(hs, tab, N.random.RandomState(3).uniform(size=200000))
    g = I * N.cos(a) * N.sin(a)
    stretches = [k for k in range(a.size - 1) if g[k] == 0. and g[k + 1] == 0.]
    assert stretches
    for k in stretches:
        assert not N.any((got > a[k]) & (got < a[k + 1]))


@pytest.mark.parametrize('name', NAMES)
def test_packing(hs, name):
    a, I = GOLD[name + '_angles'], GOLD[name + '_intensity']
    tab, tc, uc = pack(hs, a, I)
    n = a.size
    th, g, cdf = tab[:n], tab[n:2 * n], tab[2 * n:]
    g_ref = I * N.cos(a) * N.sin(a)
    mass = N.sum(0.5 * (g_ref[:-1] + g_ref[1:]) * N.diff(a))
    assert N.array_equal(th, a)
    assert N.allclose(g, g_ref / mass, rtol=1e-14, atol=0)
    assert cdf[0] == 0. and cdf[-1] == 1.
    assert N.allclose(cdf, N.cumsum(N.r_[0., 0.5 * (g_ref[:-1] + g_ref[1:]) * N.diff(a)]) / mass, rtol=0, atol=1e-14)
    assert N.all(N.diff(cdf) >= 0.)
    # the core: the smallest point beyond which at most 1 % of the mass lies
    k = int(N.flatnonzero(th == tc)[0])
    assert uc == cdf[k] and 1. - cdf[k] <= 0.01 + 1e-15
    assert k == 1 or 1. - cdf[k - 1] > 0.01


@pytest.mark.parametrize('name', NAMES)
def test_core_rays_stay_in_the_core(hs, name):
    a, I = GOLD[name + '_angles'], GOLD[name + '_intensity']
    tab, tc, uc = pack(hs, a, I)
    u = N.random.RandomState(11).uniform(0., uc, size=1000000)
    u[:4] = [0., uc * (1. - 2. ** -52), N.nextafter(uc, 0.), uc * 0.5]
    got = theta_of(hs, tab, u)
    assert got.max() <= tc * (1. + 2. ** -52), (name, got.max() - tc)


def test_reference_cdf_ends_below_one():
    """the defect the device table avoids: the reference's CDF of the 437-point table ends a little below 1"""
    assert GOLD['buie05_cdf'][-1] < 1.


@pytest.mark.parametrize('args', [
    ([0.], [1.]),                                      # one point
    (N.linspace(0., 0.01, 4097), N.ones(4097)),        # too many
    ([0., N.nan, 0.01], [1., 1., 1.]),
    ([0., 0.02, 0.01], [1., 1., 1.]),                  # not increasing
    ([0., 0.01, 0.01], [1., 1., 1.]),                  # not strictly increasing
    ([-0.001, 0.01], [1., 1.]),                        # below 0
    ([0., N.pi / 2.], [1., 1.]),                       # reaches pi/2
    ([0., 0.01], [1., -1.]),                           # negative
    ([0., 0.01], [1., N.inf]),
    ([0., 0.01], [0., 0.]),                            # no mass
    ([0., 0.01, 0.02], [0., 0., 0.]),
    ([0., 0.01], [1.]),                                # lengths differ
])
def test_invalid_tables_raise(args):
    from tracer_amd import sources
    with pytest.raises(ValueError):
        sources.tabulated_sunshape(10, N.c_[[0., 0., 10.]], N.r_[0., 0., -1.], 1., args[0], args[1], flux=1., seed=1)
    with pytest.raises(ValueError):
        sources.rect_tabulated_sunshape(10, N.c_[[0., 0., 10.]], N.r_[0., 0., -1.], 1., 2., args[0], args[1], flux=1., seed=1)


def test_ctypes_struct_has_the_compilers_size(hs):
    from tracer_amd import _cabi
    assert C.sizeof(_cabi.SourceDesc) == hs.hs_sizeof_source_desc()
    assert _cabi.SourceDesc.table.offset == 4


def test_sources_are_pending_and_take_a_spectrum():
    from tracer_amd import _cabi, sources
    from tracer_amd.source_spectrum import SourceSpectrum
    a, I = GOLD['buie05_angles'], GOLD['buie05_intensity']
    spec = SourceSpectrum.tabulated([0.4e-6, 0.7e-6], [1., 1.])
    b = sources.tabulated_sunshape(100, N.c_[[0., 0., 10.]], N.r_[0., 0., -1.], 2., a, I, flux=1000., seed=3)
    r = sources.rect_tabulated_sunshape(100, N.c_[[0., 0., 10.]], N.r_[0., 0., -1.], 2., 3., a, I, flux=1000., seed=3,
                                        spectrum=spec)
    assert b.is_pending() and r.is_pending()
    assert b._src_desc.kind == _cabi.SRC_SUNSHAPE_DISK and r._src_desc.kind == _cabi.SRC_SUNSHAPE_RECT
    assert N.isclose(b._src_desc.energy, 1000. * N.pi * 4. / 100.) and N.isclose(r._src_desc.energy, 1000. * 6. / 100.)
    assert r.source_spectrum() is spec and b.source_spectrum() is None
    # one table per content: a Monte-Carlo loop that makes a bundle per batch packs and uploads it once
    b2 = sources.tabulated_sunshape(100, N.c_[[0., 0., 10.]], N.r_[0., 0., -1.], 2., list(a), list(I), flux=1000., seed=4)
    assert b2._src_table is b._src_table is r._src_table


def _resolved(desc, tab, tc, uc):
    """the descriptor as the library resolves it (p[5..7], the table's address in buie[0])"""
    from tracer_amd import _cabi
    d = _cabi.SourceDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    d.p[5], d.p[6], d.p[7] = tc, uc, float(tab.size // 3)
    d.buie[0] = N.array([tab.ctypes.data], dtype=N.uint64).view(N.float64)[0]
    return d


def test_host_sources_match_the_buie_sources(hs):
    """the Buie CSR-0 nodes as a table reproduce buie_sunshape(CSR=0)'s rays (host builds of both)"""
    from tracer_amd import sources
    hc = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_hostcheck.so'))
    th = N.linspace(0., 4.65e-3, 211)
    I = N.cos(0.326 * th * 1e3) / N.cos(0.308 * th * 1e3)
    tab, tc, uc = pack(hs, th, I)
    d = N.r_[0.2, -0.1, -1.] / N.linalg.norm([0.2, -0.1, -1.])
    m = 20000
    for tab_src, buie_src in [(sources.tabulated_sunshape(m, N.c_[[1., 2., 30.]], d, 4., th, I, flux=1., seed=9),
                               sources.buie_sunshape(m, N.c_[[1., 2., 30.]], d, 4., 0., flux=1., seed=9)),
                              (sources.rect_tabulated_sunshape(m, N.c_[[1., 2., 30.]], d, 4., 3., th, I, flux=1., seed=9),
                               sources.rect_buie_sunshape(m, N.c_[[1., 2., 30.]], d, 4., 3., 0., flux=1., seed=9))]:
        out = [N.empty(m) for _ in range(6)]
        hs.hs_sunshape_rays(C.addressof(tab_src._src_desc), _ptr(tab), th.size, tc, uc, 9, 0, m, *[_ptr(o) for o in out])
        ref = [N.empty(m) for _ in range(6)]
        assert hc.hc_source(C.byref(buie_src._src_desc), C.c_long(m), C.c_uint64(9), C.c_uint64(0), *[_ptr(o) for o in ref]) == 0
        for k in range(3):
            assert N.array_equal(out[k], ref[k])
        assert N.abs(N.array(out[3:]) - N.array(ref[3:])).max() < 1e-12


def _fp(hc, cs, desc, n, M=512, seed=77, offset=0):
    out = N.zeros(10)
    why = C.create_string_buffer(128)
    extra = N.ascontiguousarray(cs.extra if len(cs.extra) else N.zeros(1))
    hc.hc_footprint.restype = C.c_int
    rc = hc.hc_footprint(cs.n_surf, cs.descs, _ptr(extra), C.byref(desc), C.c_long(n), C.c_uint64(seed), C.c_uint64(offset), M,
                         _ptr(out), why, 128)
    return rc, out, why.value.decode()


def test_footprint_map_is_conservative(hs):
    """
    The footprint map of the two sunshape kinds (trc_footprint.h): every core ray (u2 < u_c) whose float64 brute-force nearest hit
    exists starts in a set cell of the mask, finds the surface in its cell's list and passes its oriented-box test.  NSTTF under
    the 437-point table, the dish under a disc and a rectangle.
    """
    from tracer_amd import scenes, sources
    from tracer_amd.scene import compile_scene
    hc = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_hostcheck.so'))
    a, I = GOLD['buie05_angles'], GOLD['buie05_intensity']
    tab, tc, uc = pack(hs, a, I)
    assert 4.65e-3 < tc < 0.04 and 0.98 < uc < 1.
    plant, field, rec, src = scenes.nsttf_field()
    cs = compile_scene(plant)
    b = sources.tabulated_sunshape(10, src['center'], src['direction'], src['radius'], a, I, flux=src['flux'], seed=1)
    rc, o, why = _fp(hc, cs, _resolved(b._src_desc, tab, tc, uc), 150000)
    assert rc == 0, why
    assert o[4] == 0 and o[3] > 5000 and o[8] < 0.1 * o[9], list(o)
    assert 0.5 * (1. - uc) < o[1] / o[0] < 2. * (1. - uc)         # the tail takes the general path
    asm, dish_surf, rec_surf, dsrc = scenes.dish()
    dcs = compile_scene(asm)
    for b in (sources.tabulated_sunshape(10, dsrc['center'], dsrc['direction'], dsrc['radius'], a, I, flux=1., seed=1),
              sources.rect_tabulated_sunshape(10, dsrc['center'], dsrc['direction'], 4., 3., a, I, flux=1., seed=1)):
        rc, o, why = _fp(hc, dcs, _resolved(b._src_desc, tab, tc, uc), 60000)
        assert rc == 0 and o[4] == 0 and o[3] > 40000, (why, list(o))
    # a table whose core reaches 0.5 rad or more gets no map (every ray takes the general path)
    wide = N.linspace(0., 1.2, 50)
    tab_w, tc_w, uc_w = pack(hs, wide, N.ones(50))
    assert tc_w >= 0.5
    b = sources.tabulated_sunshape(10, dsrc['center'], dsrc['direction'], dsrc['radius'], wide, N.ones(50), flux=1., seed=1)
    rc, o, why = _fp(hc, dcs, _resolved(b._src_desc, tab_w, tc_w, uc_w), 10)
    assert rc == -3 and 'cone' in why
