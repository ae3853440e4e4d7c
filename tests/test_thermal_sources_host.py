"""
The thermal emitters on the host (no GPU): the emittance table's packing and its exact sampler (trc_emittance_pack, trc_emittance_theta
of csrc/trc_core.h, compiled with g++: tests/hostcheck/thermal_check.cpp, and the same source as a program built with the
sanitizers), the six shapes against the reference's samplers with its draws replayed (tests/golden/thermal_sources.npz), the host
function against the reference's, the exact sampler against the reference's weighted one, what csrc/trc_forms.h decides for the kind,
and the Python constructors without a device.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

import thermal_cases as TC
from thermal_cases import GOLD, NS, ROOT, SEEDS

THERMAL = 12
SHAPES = ('disk', 'triangle', 'cylinder', 'frustum_wide', 'frustum_narrow', 'sphere')


@pytest.fixture(scope='module')
def ht():
    return TC.load_hostcheck()


# 1 -- pack ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TC.TABLES)
def test_pack_matches_a_gauss_quadrature(ht, name):
    """cdf against a 16-point Gauss-Legendre rule per interval to 1e-13; the last entry exactly 1; theta and eps / M as given; the
    mass is the Python table's"""
    from tracer_amd import sources
    xs_raw, ys = TC.raw_table(name)
    xs, _ = TC.table(name)
    tab, mass = TC.pack(ht, xs_raw, ys)
    n = xs.size
    cdf, m_gauss = TC.gauss_cdf(xs, ys)
    print(name, 'cdf - gauss', N.abs(tab[2 * n:] - cdf).max(), 'mass', mass, m_gauss)
    assert N.abs(tab[2 * n:] - cdf).max() <= 1e-13
    assert tab[3 * n - 1] == 1. and tab[2 * n] == 0. and N.all(N.diff(tab[2 * n:]) >= 0.)
    assert N.array_equal(tab[:n], xs) and N.array_equal(tab[n:2 * n], ys / mass)
    assert abs(mass - m_gauss) <= 1e-13 * m_gauss
    assert abs(sources.EmittanceTable(xs_raw, ys).mass - mass) <= 1e-15
    if name == 'dir':       # the mass the reference's tot_integ_cossin misses (0.9690 there: DESIGN.md 14.16)
        assert abs(mass - 0.3504) < 1e-4
    if name in ('dir', 'gray', 'gray2'):        # pi/2 as 8 decimals state it is read as pi/2
        assert xs_raw[-1] > N.pi / 2. and xs[-1] == N.pi / 2.


def test_pack_refusals(ht):
    """theta beyond pi/2, angles not increasing, negative or non-finite emittances, no mass, 1 point and 4097 points: the library's
    check and the Python one"""
    from tracer_amd import sources

    def refused(th, eps):
        th, eps = N.ascontiguousarray(th, dtype=float), N.ascontiguousarray(eps, dtype=float)
        fault = ht.ht_table_fault(th.size, TC.ptr(th), TC.ptr(eps)) != b''
        if not fault:
            fault = ht.ht_pack(th.size, TC.ptr(th), TC.ptr(eps), TC.ptr(N.zeros(3 * th.size)), None) == 0
        with pytest.raises(ValueError):
            sources.check_emittance_table(th, eps)
        return fault

    assert refused([0., 1., 1.6], [1., 1., 1.])
    assert refused([0., 1., N.pi / 2. + 1e-8], [1., 1., 1.])
    assert refused([-0.1, 1., 1.5], [1., 1., 1.])
    assert refused([0., 1.2, 1.], [1., 1., 1.])
    assert refused([0., 1., 1.], [1., 1., 1.])
    assert refused([0., N.pi / 2., N.pi / 2. + 1e-9], [1., 1., 1.])      # (both are pi/2 once read)
    assert refused([0., 1., 1.5], [1., -0.1, 1.])
    assert refused([0., 1., 1.5], [1., N.inf, 1.])
    assert refused([0., 1., 1.5], [1., N.nan, 1.])
    assert refused([0., N.nan, 1.5], [1., 1., 1.])
    assert refused([0., 1., 1.5], [0., 0., 0.])
    assert refused([0.5], [1.])
    assert refused(N.linspace(0., 1.5, 4097), N.ones(4097))
    assert not ht.ht_table_fault(4096, TC.ptr(N.linspace(0., 1.5, 4096)), TC.ptr(N.ones(4096)))
    with pytest.raises(ValueError):
        sources.check_emittance_table([0., 1.], [1., 1., 1.])
    assert abs(ht.ht_theta_max() - (N.pi / 2. + 5e-9)) < 1e-15


# 2 -- inversion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TC.TABLES)
def test_inversion_on_the_grid(ht, name):
    """
    1e5 seeded uniforms with the edge values and the CDF's nodes among them: |F(theta) - u| <= 1e-12 with F restated in NumPy from
    the table; theta within the table and non-decreasing in u; fewer than 64 iterations (the cap never ends the loop); nothing
    inside `gap`'s empty stretch; `gray` and `gray2` are the Lambertian law asin(sqrt(u)) to 1e-12.

    asin(sqrt(u)) is stated as atan2(sqrt(u), sqrt(1 - u)), which is the same angle and is exact to rounding everywhere: NumPy's
    arcsin(sqrt(u)) is itself 4e-9 off at u = 1 - 2^-53, an edge value of this grid (sqrt(u) rounds to 1 - 2^-53, whose arc sine is
    pi/2 - 1.49e-8, where the angle is pi/2 - 1.05e-8), so no sampler that is exact to 1e-12 can agree with it there.  The bound
    stays 1e-12 in theta.
    """
    xs, ys = TC.table(name)
    tab, _ = TC.pack(ht, *TC.raw_table(name))
    u = TC.inversion_grid(tab[2 * xs.size:])
    th, it = TC.theta_of(ht, tab, u)
    res = N.abs(TC.cdf_at(xs, ys, th) - u)
    print(name, 'residual', res.max(), 'iterations max %d mean %.2f' % (it.max(), it.mean()), 'range', th.min(), th.max())
    assert res.max() <= 1e-12
    assert th.min() >= xs[0] and th.max() <= xs[-1]
    order = N.argsort(u, kind='stable')
    assert N.all(N.diff(th[order]) >= 0.)
    assert it.max() < 64
    assert th[0] == xs[0]                                       # u = 0
    if name == 'gap':
        assert not N.any((th > 0.5) & (th < 0.9))
    if name in ('gray', 'gray2'):
        lam = N.arctan2(N.sqrt(u), N.sqrt(1. - u))
        print(name, 'against the Lambertian law', N.abs(th - lam).max())
        assert N.abs(th - lam).max() <= 1e-12
        assert it.max() == 0                                    # the closed form


@pytest.mark.parametrize('name', TC.TABLES)
def test_inversion_against_a_quadrature_of_the_density(ht, name):
    """the same grid against F by Gauss-Legendre quadrature of eps cos sin up to theta -- a yardstick that does not share the
    sampler's antiderivative: |F(theta) - u| <= 1e-12 (a 16-point rule on at most 0.6 rad of this analytic integrand is exact to
    rounding)"""
    xs, ys = TC.table(name)
    tab, _ = TC.pack(ht, *TC.raw_table(name))
    u = TC.inversion_grid(tab[2 * xs.size:])
    th, _ = TC.theta_of(ht, tab, u)
    res = N.abs(TC.gauss_cdf_at(xs, ys, th) - u)
    print(name, 'residual against the quadrature', res.max())
    assert res.max() <= 1e-12


def test_inversion_on_irregular_and_narrow_tables(ht):
    """
    Tables the six do not reach: 100 tables of 20..60 randomly spaced points with random emittances, and a step of the emittance
    over an interval 1e-3 .. 1e-10 wide.  The CDF over an interval is evaluated in theta - theta_i (trc_emittance_G), so its rounding
    is 1e-16 of the interval's own mass whatever the slope, and the iteration ends on its stop |G - t| <= 2^-50.  Against the
    quadrature: |F(theta) - u| <= 2^-48 -- the stop, and as much again three times over for the rounding of u - cdf_i, of the
    running sums of the cdf and of the yardstick itself; theta non-decreasing in u; fewer than 64 iterations.  (As a difference of
    two values of the antiderivative the residuals were 4e-12 on these tables and 1e-9 on the narrowest steps.)
    """
    rs = N.random.RandomState(1)
    worst, most = 0., 0
    for trial in range(100):
        n = rs.randint(20, 61)
        xs = N.sort(rs.uniform(0., N.pi / 2., n))
        xs[0] = 0.
        ys = rs.uniform(0., 1., n)
        tab, _ = TC.pack(ht, xs, ys)
        u = N.sort(rs.uniform(size=5000))
        th, it = TC.theta_of(ht, tab, u)
        worst, most = max(worst, N.abs(TC.gauss_cdf_at(xs, ys, th) - u).max()), max(most, it.max())
        assert N.all(N.diff(th) >= 0.) and th.min() >= 0. and th.max() <= xs[-1]
    print('irregular tables: worst residual', worst, 'most iterations', most)
    assert worst <= 2. ** -48 and most < 64
    for width in (1e-3, 1e-5, 1e-7, 1e-10):
        xs, ys = N.array([0., 0.7, 0.7 + width, 1.5]), N.array([0.2, 0.1, 0.9, 0.3])
        tab, _ = TC.pack(ht, xs, ys)
        cdf = tab[8:]
        assert cdf[2] > cdf[1]
        u = N.linspace(cdf[1], cdf[2], 2001)[1:-1]
        th, it = TC.theta_of(ht, tab, u)
        res = N.abs(TC.gauss_cdf_at(xs, ys, th) - u).max()
        print('a step over', width, 'rad: residual', res, '=', res / (cdf[2] - cdf[1]), 'of the interval mass, iterations', it.max())
        assert res <= 2. ** -48
        assert N.all(N.diff(th) >= 0.) and th.min() >= xs[1] and th.max() <= xs[2] and it.max() < 64


def test_a_constant_table_is_the_lambertian_sampler(ht):
    """a constant table over [0, ang] reproduces Lambertian_directions_sampling: sin(theta) = sin(ang) sqrt(u)"""
    for ang in (0.3, 1.0, N.pi / 2.):
        tab, _ = TC.pack(ht, [0., ang], [1., 1.])
        u = N.random.RandomState(3).uniform(size=20000)
        th, it = TC.theta_of(ht, tab, u)
        assert N.abs(N.sin(th) - N.sin(ang) * N.sqrt(u)).max() <= 1e-14 and it.max() == 0


def test_the_sanitizer_program_runs_the_grid_clean():
    """the same source as a program of its own, built with the address and undefined-behaviour sanitizers, run as a child process"""
    subprocess.check_call(['make', '-s', '-C', ROOT, 'thermalcheck'])
    r = subprocess.run([os.path.join(ROOT, 'tests', 'hostcheck', 'thermal_check')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0 and 'thermal_check: OK' in out, out
    assert 'runtime error' not in out and 'AddressSanitizer' not in out, out


# 3 -- shapes against the reference, replayed draws ----------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('name', SHAPES)
def test_shapes_from_the_reference_uniforms(ht, name, seed):
    """
    points to 1e-12 x the shape's size, normals to 1e-12, in both senses of the sampler's flag.  u0 is the reference sampler's first
    draw and u1 its second: disc ths, rs; triangle r1, r2; cylinder zs, ths; frustum R, phi (uniform(low, high) is low + (high - low)
    u); sphere phis, cosths (uniform(-1, 1) is 2 u - 1).
    """
    from tracer_amd import sources
    g = lambda what: GOLD['%d_%s_%s' % (seed, name, what)]
    u = GOLD['%d_u' % seed]
    flag = 'normal_up' if name in ('disk', 'triangle') else 'normal_in'
    for tag, val in (('a', False), ('b', True)):
        p, area, origin, sign = sources._thermal_shape('test', TC.shape_dict(name, **{flag: val}))
        pos, nrm = TC.points_u(ht, p, u)
        assert N.abs(pos + origin[:, None] - g('pos')).max() <= 1e-12 * TC.shape_size(name)
        assert N.abs(sign * nrm - g('n_' + tag)).max() <= 1e-12
        assert sign == ({'normal_up': 1. if val else -1., 'normal_in': -1. if val else 1.}[flag])
    # the default of the flag is the shape's own normal: up, outwards
    assert sources._thermal_shape('test', TC.shape_dict(name))[3] == 1.


def test_the_rectangle_as_it_is_meant(ht):
    """the reference's rectangle_sampling raises NameError; here: (X (u0 - 1/2), Y (u1 - 1/2), 0), the host sampler the same points"""
    from tracer_amd import sampling, sources
    p, area, origin, sign = sources._thermal_shape('test', {'type': 'rectangle', 'kwargs': {'x': 0.4, 'y': 1.2}})
    u = N.random.RandomState(8).uniform(size=(2, 500))
    pos, nrm = TC.points_u(ht, p, u)
    assert N.abs(pos - N.vstack((0.4 * (u[0] - 0.5), 1.2 * (u[1] - 0.5), N.zeros(500)))).max() <= 1e-15
    assert N.array_equal(nrm, N.vstack((N.zeros(500), N.zeros(500), N.ones(500)))) and area == 0.4 * 1.2
    N.random.seed(8)
    host, hn = sampling.rectangle_sampling(0.4, 1.2, 500, normals=True, normal_up=False)
    assert N.abs(host - pos).max() <= 1e-15 and N.array_equal(hn, -nrm)


@pytest.mark.parametrize('seed', SEEDS)
def test_host_shape_samplers_are_the_references(seed):
    from tracer_amd import sampling
    for name in ('triangle', 'frustum_wide', 'frustum_narrow'):
        fn = getattr(sampling, name.split('_')[0] + '_sampling')
        for tag, val in (('a', False), ('b', True)):
            N.random.seed(seed)
            pos, nrm = fn(ns=NS, normals=True, **dict(TC.shape_kwargs(name), **{'normal_up' if name == 'triangle' else 'normal_in': val}))
            assert N.abs(pos - GOLD['%d_%s_pos' % (seed, name)]).max() <= 1e-12 * TC.shape_size(name)
            assert N.abs(nrm - GOLD['%d_%s_n_%s' % (seed, name, tag)]).max() <= 1e-12


# 4 -- the host function against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('name', TC.REFERENCE_TABLES)
def test_host_function_from_the_reference_draws(name, seed):
    """energy, directions, wavelengths and ref_index to 1e-12 relative; the band's radiance, mean wavelength and the exitance too"""
    from tracer_amd import sources
    xs, ys = TC.raw_table(name)
    pos, nrm = GOLD['%d_disk_pos' % seed], GOLD['%d_disk_n_b' % seed]
    area = N.pi * float(GOLD['r_disk']) ** 2
    N.random.seed(seed + 50)
    rb = sources.spectral_band_axisymmetrical_thermal_emission_source(pos.copy(), nrm.copy(), area, xs, ys, TC.T_WALL, NS, TC.BAND,
                                                                      TC.REF_INDEX)
    g = lambda what: GOLD['%d_%s_%s' % (seed, name, what)]
    assert N.abs(rb.get_energy() - g('energy')).max() <= 1e-12 * g('energy').max()
    assert N.abs(rb.get_directions() - g('directions')).max() <= 1e-12
    assert N.abs(rb.get_wavelengths() / g('wavelengths') - 1.).max() <= 1e-12
    assert N.array_equal(rb.get_ref_index(), g('ref_index'))
    assert N.array_equal(rb.get_vertices(), pos)
    L_band, wl_avg, wls = sources.band_radiance(TC.T_WALL, TC.BAND)
    assert abs(L_band / float(GOLD['L_band']) - 1.) <= 1e-12 and abs(wl_avg / float(GOLD['wl_avg']) - 1.) <= 1e-12
    assert abs(rb.get_energy().sum() / area / float(GOLD[name + '_exitance']) - 1.) <= 1e-12


@pytest.mark.parametrize('name', TC.REFERENCE_TABLES)
def test_the_device_bundle_carries_the_references_power(name):
    """thermal_emitter_bundle(quadrature='trapezoid'): the same total power and the same wl_avg to 1e-12 relative, without a device"""
    from tracer_amd import sources
    xs, ys = TC.raw_table(name)
    r = float(GOLD['r_disk'])
    n = 1000
    b = sources.thermal_emitter_bundle(n, {'type': 'disk', 'kwargs': {'r_ext': r}}, xs, ys, TC.T_WALL, TC.BAND, N.zeros(3),
                                       N.array([0., 0., 1.]), ref_index=TC.REF_INDEX, seed=1)
    assert b.is_pending()
    power = float(GOLD[name + '_exitance']) * N.pi * r ** 2
    assert abs(b._src_desc.energy * n / power - 1.) <= 1e-12
    assert abs(GOLD['%d_%s_energy' % (SEEDS[0], name)].sum() / power - 1.) <= 1e-12
    spec = b.source_spectrum()
    assert abs(spec.wavelength / float(GOLD['wl_avg']) - 1.) <= 1e-12 and spec.ref_index == TC.REF_INDEX and not spec.has_table()
    # 'exact': the table's analytic mass in place of the node trapezoid
    bx = sources.thermal_emitter_bundle(n, {'type': 'disk', 'kwargs': {'r_ext': r}}, xs, ys, TC.T_WALL, TC.BAND, N.zeros(3),
                                        N.array([0., 0., 1.]), quadrature='exact', seed=1)
    m = sources.emittance_table(xs, ys).mass
    assert abs(bx._src_desc.energy * n / (2. * N.pi * float(GOLD['L_band']) * m * N.pi * r ** 2) - 1.) <= 1e-12


# 5 -- the exact sampler against the reference's weighted one -----------------------------------------------------------------------
@pytest.mark.parametrize('name', TC.REFERENCE_TABLES)
def test_exact_sampler_against_the_references_weighted_histogram(ht, name):
    """
    1e6 angles of the host build from a fixed seed in the fixture's 24 bins: |h_new - h_ref| <= 4 sqrt(s_new^2 + s_ref^2) in every
    bin, s_ref from the fixture's sum of squared weights (4e6 weighted samples of the reference), s_new binomial; a bin is empty
    in one histogram exactly where it is empty in the other.
    """
    xs_raw, ys = TC.raw_table(name)
    tab, _ = TC.pack(ht, xs_raw, ys)
    n = 1000000
    th, _ = TC.theta_of(ht, tab, N.random.RandomState(77).uniform(size=n))
    bins = N.linspace(xs_raw[0], xs_raw[-1], 25)
    h_new = N.histogram(th, bins)[0] / float(n)
    s_new2 = h_new * (1. - h_new) / n
    n_ref = float(GOLD['hist_n'])
    h_ref = GOLD[name + '_hist_w'] / n_ref
    s_ref2 = N.maximum(GOLD[name + '_hist_w2'] / n_ref - h_ref ** 2, 0.) / n_ref
    s = N.sqrt(s_new2 + s_ref2)
    z = N.abs(h_new - h_ref) / N.where(s > 0., s, 1.)
    print(name, 'worst bin', z.max(), 'sigmas')
    assert abs(h_new.sum() - 1.) < 1e-12 and abs(h_ref.sum() - 1.) < 1e-9
    assert N.array_equal(h_new == 0., h_ref == 0.)
    assert N.all(N.abs(h_new - h_ref) <= 4. * s)


# 6 -- decisions, from the host-compiled header ---------------------------------------------------------------------------------------
TRACE_ACCEL, TRACE_STREAM, TRACE_MEGAKERNEL = 1, 4, 8


@pytest.fixture(scope='module')
def hl():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_lamp_check.so'))
    lib.hl_decide.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int] + \
        [C.POINTER(C.c_int)] * 3
    return lib


def decide(hl, kind, n_surf=3, n=200000, flags=TRACE_ACCEL, spec=0, walk_ok=1):
    bufs = [C.create_string_buffer(96) for _ in range(3)]
    ints = [C.c_int() for _ in range(3)]
    use_stream = hl.hl_decide(kind, n_surf, n, flags, spec, walk_ok, bufs[0], bufs[1], bufs[2], 96, *[C.byref(i) for i in ints])
    return dict(use_stream=bool(use_stream), mega=bufs[0].value.decode(), gen0=bufs[1].value.decode(), first=bufs[2].value.decode(),
                has_map=bool(ints[0].value), use_first=ints[1].value, valid=bool(ints[2].value))


def test_the_kind_and_the_descriptor_keep_the_abi(ht):
    from tracer_amd import _cabi
    assert ht.ht_kind() == _cabi.SRC_EMIT_THERMAL == THERMAL
    assert ht.ht_sizeof_source_desc() == C.sizeof(_cabi.SourceDesc)
    assert 'trc_emittance_table_create' in _cabi.SIGNATURES
    assert (TRACE_ACCEL, TRACE_STREAM, TRACE_MEGAKERNEL) == (_cabi.TRACE_ACCEL, _cabi.TRACE_STREAM, _cabi.TRACE_MEGAKERNEL)
    # an emitter is a lamp or the thermal kind; the lamps' predicate stays theirs
    assert [k for k in range(-1, 16) if ht.ht_is_emitter(k)] == [9, 10, 11, 12]
    assert [k for k in range(-1, 16) if ht.ht_is_lamp(k)] == [9, 10, 11]
    assert (_cabi.THERMAL_DISK, _cabi.THERMAL_RECT, _cabi.THERMAL_TRIANGLE, _cabi.THERMAL_CYLINDER, _cabi.THERMAL_FRUSTUM,
            _cabi.THERMAL_SPHERE) == (0, 1, 2, 3, 4, 5)


@pytest.mark.parametrize('n_surf', [3, 20, 200])
def test_the_thermal_kind_takes_the_general_path_and_the_lamps_megakernel(hl, n_surf):
    _t = lambda b: 'true' if b else 'false'
    for spec in (0, 1):
        d = decide(hl, THERMAL, n_surf=n_surf, spec=spec)
        assert not d['has_map']
        assert d['gen0'] == 'k_s_gen_emit'
        assert d['use_first'] == 0
        assert d['mega'] == 'k_lamp_coop<512, %s, false>' % _t(spec)      # the lamps' instances: trc_lamp_ray_t<-1> knows the kind
        assert d['valid']
    # the stream thresholds test_lamp_forms_host.py asserts for a lamp
    assert not decide(hl, THERMAL, n_surf=n_surf, n=200000)['use_stream']
    assert not decide(hl, THERMAL, n_surf=n_surf, n=50, flags=TRACE_ACCEL | TRACE_STREAM)['use_stream']
    assert decide(hl, THERMAL, n_surf=n_surf, n=64, flags=TRACE_ACCEL | TRACE_STREAM)['use_stream']
    assert decide(hl, THERMAL, n_surf=n_surf, n=1 << 20)['use_stream']
    assert not decide(hl, THERMAL, n_surf=n_surf, n=1 << 20, flags=TRACE_ACCEL | TRACE_MEGAKERNEL)['use_stream']
    # a scene without a general path (the large grid) gives the call to the megakernel
    for flags in (TRACE_ACCEL, TRACE_ACCEL | TRACE_STREAM):
        assert not decide(hl, THERMAL, n_surf=200, n=1 << 20, flags=flags, walk_ok=0)['use_stream']


def test_the_header_holds_k_s_gen_emit_and_no_other_new_id():
    import search_cases as S
    names = S.library_ids(ints=(-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 128, 256, 512, 1024))
    assert names.count('k_s_gen_emit') == 1
    assert not [n for n in names if n != 'k_s_gen_emit' and 'emit' in n]
    import re
    assert not [n for n in names if re.search(r'[<, ](12|13)[,>]', n)]        # no instance of any family names the kind


def test_library_holds_k_s_gen_emit_by_name():
    import re
    import shutil
    lib = os.path.join(ROOT, 'tracer_amd', 'lib', 'libtracer_amd.so')
    if not os.path.exists(lib) or shutil.which('nm') is None:
        pytest.skip('no built library, or no nm')
    held = [l for l in subprocess.check_output(['nm', '-C', lib]).decode().splitlines()
            if re.search(r'\bk_s_gen_emit\(StreamParams\)', l) and '__device_stub__' not in l]
    assert held


# 7 -- Python without a device --------------------------------------------------------------------------------------------------------
POSE = dict(center=N.array([0.3, -0.2, 1.1]), direction=N.array([0.48, -0.6, 0.64]))


def bundle(shape, n=1000, table='dir', **kw):
    from tracer_amd import sources
    xs, ys = TC.raw_table(table)
    kw = dict(dict(POSE, seed=5), **kw)
    return sources.thermal_emitter_bundle(n, shape, xs, ys, TC.T_WALL, TC.BAND, **kw)


@pytest.mark.parametrize('name', SHAPES + ('rectangle',))
def test_bundles_are_pending_descriptors(name):
    from tracer_amd import _cabi, sources
    from tracer_amd.vector_manipulations import rotate_z_to_normal
    shape = {'type': 'rectangle', 'kwargs': {'x': 0.4, 'y': 1.2}} if name == 'rectangle' else TC.shape_dict(name)
    b = bundle(shape)
    d = b._src_desc
    assert b.is_pending() and b.get_num_rays() == 1000
    assert d.kind == _cabi.SRC_EMIT_THERMAL and d.table == 0          # (the table is made on the device when the rays are needed)
    p = list(d.p)
    kw = shape['kwargs']
    want, area = {
        'disk': lambda: ([0., kw['r_ext'], 0., 0., 0., 0.], N.pi * kw['r_ext'] ** 2),
        'rectangle': lambda: ([1., 0.4, 1.2, 0., 0., 0.], 0.48),
        'triangle': lambda: ([2.] + list((kw['B'] - kw['A'])[:2]) + list((kw['C'] - kw['A'])[:2]) + [0.],
                             0.5 * abs(N.cross(kw['B'] - kw['A'], kw['C'] - kw['A'])[2])),
        'cylinder': lambda: ([3., kw['r_ext'], kw['h'], 0., 0., 0.], 2. * N.pi * kw['r_ext'] * kw['h']),
        'frustum': lambda: ([4., kw['r0'], kw['r1'], kw['z1'] - kw['z0']] + list(kw['angular_span']),
                            (kw['angular_span'][1] - kw['angular_span'][0]) / 2. * (kw['r0'] + kw['r1']) *
                            N.hypot(kw['r1'] - kw['r0'], kw['z1'] - kw['z0'])),
        'sphere': lambda: ([5., kw['r_ext'], 0., 0., 0., 0.], 4. * N.pi * kw['r_ext'] ** 2),
    }[shape['type']]()
    assert N.allclose(p[:6], want, rtol=0, atol=1e-15) and p[6] == 1. and p[7] == 0.
    xs, ys = TC.raw_table('dir')
    exitance = 2. * N.pi * float(GOLD['L_band']) * N.sum(N.diff(xs) * ((ys * N.cos(xs) * N.sin(xs))[1:] + (ys * N.cos(xs) * N.sin(xs))[:-1]) / 2.)
    assert abs(d.energy / (exitance * area / 1000.) - 1.) <= 1e-12
    rot = rotate_z_to_normal(N.eye(3), POSE['direction'])
    assert N.allclose(N.array(d.rot_pos).reshape(3, 3), rot, atol=1e-15) and N.array_equal(list(d.rot_pos), list(d.rot_dir))
    origin = kw['A'] if name == 'triangle' else N.zeros(3)
    assert N.allclose(list(d.center), POSE['center'] + N.dot(rot, origin), atol=1e-15)
    # rays_in, and the sampler's own flag, turn the sign
    assert bundle(shape, rays_in=True)._src_desc.p[6] == -1.
    flag = 'normal_up' if shape['type'] in ('disk', 'rectangle', 'triangle') else 'normal_in'
    turned = {'type': shape['type'], 'kwargs': dict(kw, **{flag: flag == 'normal_in'})}
    assert bundle(turned)._src_desc.p[6] == -1. and bundle(turned, rays_in=True)._src_desc.p[6] == 1.
    assert isinstance(b._src_table, sources.EmittanceTable)


def test_the_table_cache_and_a_scalar_emittance():
    from tracer_amd import sources
    xs, ys = TC.raw_table('gray')
    t = sources.emittance_table(xs, ys)
    assert sources.emittance_table(xs.copy(), list(ys)) is t
    assert sources.emittance_table(xs, ys * 0.5) is not t
    shape = TC.shape_dict('disk')
    a = sources.thermal_emitter_bundle(10, shape, xs, 0.8, TC.T_WALL, TC.BAND, **POSE)
    assert a._src_table is t                                   # a scalar is the constant table over thetas
    assert bundle(shape)._src_table is bundle(shape)._src_table
    assert not isinstance(t, sources.AngleTable) and isinstance(t, sources.SunshapeTable)


def test_spectrum_options():
    from tracer_amd import sources
    from tracer_amd.source_spectrum import SourceSpectrum
    shape = TC.shape_dict('disk')
    pl = bundle(shape, spectrum='planck', ref_index=1.3).source_spectrum()
    want = SourceSpectrum.planck(TC.T_WALL, TC.BAND, ref_index=1.3)
    assert pl.has_table() and not pl.is_carried() and pl.ref_index == 1.3
    assert N.array_equal(pl.wavelengths, want.wavelengths) and N.array_equal(pl.values, want.values)
    assert bundle(shape, spectrum=None).source_spectrum() is None
    own = SourceSpectrum.uniform(1e-6, 2e-6)
    assert bundle(shape, spectrum=own).source_spectrum() is own
    assert bundle(shape, spectrum='planck').is_pending()
    with pytest.raises(ValueError):
        bundle(shape, spectrum='white')
    with pytest.raises(ValueError):
        bundle(shape, quadrature='simpson')


def test_gray_source_descriptor_and_energy():
    """energy / num_rays, times cos(dot(rays_direction, direction)) when rays_direction is given (the reference's :63 as written);
    rot_pos from direction, rot_dir from rays_direction; the constant table over [0, ang_range]"""
    from tracer_amd import _cabi, sources
    from tracer_amd.vector_manipulations import rotate_z_to_normal
    law = {'type': 'Lambertian', 'kwargs': {'ang_range': 0.7}}
    loc, d1, d2 = N.array([1., 2., 3.]), N.array([0., 0.6, 0.8]), N.array([0.6, 0., 0.8])
    b = sources.gray_source(TC.shape_dict('cylinder'), loc, d1, 400, law, 20., seed=3)
    d = b._src_desc
    assert b.is_pending() and d.kind == _cabi.SRC_EMIT_THERMAL and d.energy == 20. / 400 and d.p[6] == 1.
    assert N.array_equal(b._src_table.angles, [0., 0.7]) and N.array_equal(b._src_table.intensity, [1., 1.])
    assert N.array_equal(list(d.rot_pos), list(d.rot_dir)) and N.array_equal(list(d.center), loc)
    assert b.source_spectrum() is None
    b2 = sources.gray_source(TC.shape_dict('cylinder'), loc, d1, 400, law, 20., rays_direction=d2, seed=3)
    assert abs(b2._src_desc.energy - 20. / 400 * N.cos(N.dot(d2, d1))) <= 1e-18
    assert N.allclose(N.array(b2._src_desc.rot_pos).reshape(3, 3), rotate_z_to_normal(N.eye(3), d1), atol=1e-15)
    assert N.allclose(N.array(b2._src_desc.rot_dir).reshape(3, 3), rotate_z_to_normal(N.eye(3), d2), atol=1e-15)
    for bad in ({'type': 'Lambertian', 'kwargs': {'ang_range': 0.}}, {'type': 'isotropic', 'kwargs': {'ang_range': 0.5}},
                {'type': 'Lambertian', 'kwargs': {}}, {'type': 'Lambertian', 'kwargs': {'ang_range': 2.}}, None):
        with pytest.raises(ValueError):
            sources.gray_source(TC.shape_dict('disk'), loc, d1, 10, bad, 1.)


def test_value_errors():
    from tracer_amd import sources
    tri = TC.shape_kwargs('triangle')
    for shape in ({'type': 'triangle', 'kwargs': dict(tri, C=tri['C'] + N.array([0., 0., 0.1]))},        # unequal z
                  {'type': 'frustum', 'kwargs': dict(r0=0.2, r1=0.2, z0=0., z1=1.)},                      # use the cylinder
                  {'type': 'frustum', 'kwargs': dict(r0=0.2, r1=0.3, z0=1., z1=1.)},
                  {'type': 'polygon', 'kwargs': {}}, {'type': 'disk', 'kwargs': {}}, {'type': 'disk', 'kwargs': {'r_ext': -1.}},
                  {'type': 'disk', 'kwargs': {'r_ext': 1., 'h': 2.}}, {'type': 'cylinder', 'kwargs': {'r_ext': 1., 'h': 1., 'volume': True}},
                  {'type': 'sphere', 'kwargs': {'r_ext': N.inf}}, 'disk'):
        with pytest.raises(ValueError):
            bundle(shape)
    ok = TC.shape_dict('disk')
    with pytest.raises(ValueError):
        bundle(ok, n=-1)
    with pytest.raises(ValueError):
        bundle(ok, rotation=N.eye(2))
    xs, ys = TC.raw_table('dir')
    for T, band in ((0., TC.BAND), (1000., (2e-6, 1e-6)), (1000., (1e-6, 1.0005e-6))):
        with pytest.raises(ValueError):
            sources.thermal_emitter_bundle(10, ok, xs, ys, T, band, **POSE)
    with pytest.raises(ValueError):
        sources.thermal_emitter_bundle(10, ok, xs, -0.5, TC.T_WALL, TC.BAND, **POSE)
    with pytest.raises(ValueError):
        sources.thermal_emitter_bundle(10, ok, [0., 2.], [1., 1.], TC.T_WALL, TC.BAND, **POSE)
    # the reference's node trapezoid of a two-point table over [0, pi/2] is no power (negative, with pi/2 to 8 decimals)
    with pytest.raises(ValueError):
        sources.thermal_emitter_bundle(10, ok, *TC.raw_table('gray2'), TC.T_WALL, TC.BAND, **POSE)
    assert sources.thermal_emitter_bundle(10, ok, *TC.raw_table('gray2'), TC.T_WALL, TC.BAND, quadrature='exact', **POSE)._src_desc.energy > 0.


def test_the_references_names_are_in_the_modules_compat_aliases():
    """tracer.sources and ray_trace_utils.sampling resolve to these modules under tracer_amd.compat"""
    from tracer_amd import sampling, sources
    for name in ('spectral_band_axisymmetrical_thermal_emission_source', 'gray_source', 'thermal_emitter_bundle', 'emittance_table'):
        assert callable(getattr(sources, name))
    for name in ('PW_lincossin_distribution', 'PW_lincos_distribution', 'frustum_sampling', 'triangle_sampling', 'rectangle_sampling'):
        assert callable(getattr(sampling, name))
