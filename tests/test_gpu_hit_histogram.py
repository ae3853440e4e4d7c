"""
GPU tests of the histogram of captured hits (trc_scene_histogram_hits, k_hist_hits), run with -m gpu on the MI355X box.

The scene is the receiver assembly of the flux-map chart tests (fluxmap_chart_scene.receivers(), 2e5 rays of its disc source): the
cylinder (2) and the frustum (5) capture everything, the floor (0), the wall (1), the sphere (3) and the dish (4) capture lean.  The
reference of every assertion is numpy.histogram2d of dev.get_hits(), read AFTER the histogram calls, with the NumPy formulas of the
charts (hit_histogram_cases.py): counts exact, sums and squares to rtol 1e-9, atol 1e-9 of the largest bin -- the tolerance
test_gpu_fluxmap.py applies to device maps; the order of float64 sums.  The device's atan2 and acos need not match NumPy's to the
bit, so every test first asserts that no selected hit lies within 1e-12 of a map's span from an edge (an input condition: a seed
that fails it is replaced, the tolerance is not widened).
"""
import numpy as N
import pytest

import hit_histogram_cases as hh

fc = hh.fc
pytestmark = pytest.mark.gpu

REPS, EMIN = 12, 1e-10
N_RAYS, SEED = 200000, 11
FULL, LEAN = (fc.CYLINDER, fc.FRUSTUM), (fc.FLOOR, fc.WALL, fc.SPHERE, fc.DISH)
TWO_PI = 2. * N.pi


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


@pytest.fixture(scope='module')
def receivers():
    from tracer_amd import _cabi
    from tracer_amd.scene import compile_scene
    asm, objs, T = fc.receivers()
    cs = compile_scene(asm)
    lean = [bool(cs.descs[s].flags & _cabi.SURF_CAPTURE_LEAN) for s in range(cs.n_surf)]
    assert all(cs.capture) and [s for s in range(cs.n_surf) if lean[s]] == sorted(LEAN)
    return cs, T, [N.array(s._temp_frame) for s in cs.surfaces]


@pytest.fixture(scope='module')
def lib():
    return hh.host_library()


def _traced(ctx, receivers, form='stream', maps=None, seeds=(SEED,), n=N_RAYS):
    """a device scene that holds the hits of one call per seed, none read yet"""
    from tracer_amd.scene import DeviceScene
    cs, T, frames = receivers
    dev = DeviceScene(cs, ctx)
    for s in sorted(maps or {}):
        chart, swap, ue, ve = maps[s]
        dev.set_fluxmap(s, ue, ve, proj=fc.projection(frames[s], True) if swap else None, chart=chart)
    dev.set_hit_capacity(len(seeds) * (2 * n + 65536))
    for seed in seeds:
        st, _ = dev.trace_fast(fc.source(n, T, seed), REPS, EMIN, seed, accel=True, stream=(form == 'stream'))
        assert st.hits_dropped == 0
    return dev


def _compare(got, ref, what):
    """a HitHistogram against hit_histogram_cases.reference"""
    assert ref['near'] == 0, ('INPUT CONDITION, not the histogram: %d hits within %g of the span of an edge -- choose another seed'
                              % (ref['near'], fc.EDGE_EPS), what)
    assert ref['n'] > 0 and ref['count'].sum() > 0, what
    print('%s: %d x %d, %d hits, %d outside, largest difference %.3g of %.3g' %
          ((what,) + got.sum.shape + (ref['n'], ref['outside'][1], N.abs(got.sum - ref['sum']).max(), ref['sum'].max())))
    assert N.array_equal(got.count, ref['count']), (what, N.abs(got.count - ref['count']).max())
    assert got.outside[1] == ref['outside'][1] and got.count.sum() + got.outside[1] == ref['n'], what
    for mine, want in ((got.sum, ref['sum']), (got.sum_sq, ref['sum_sq'])):
        assert N.allclose(mine, want, rtol=1e-9, atol=1e-9 * want.max()), (what, N.abs(mine - want).max(), want.max())
    assert N.isclose(got.outside[0], ref['outside'][0], rtol=1e-9, atol=1e-9 * ref['sum'].max()), what


# 1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['stream', 'megakernel'])
def test_position_charts_equal_the_host_histogram_and_the_device_flux_maps(ctx, receivers, form):
    """every position chart on its surface, the edges of the chart tests' maps, absorbed energy -- after the streaming form, whose
    buffer has unwritten entries, and after the megakernel; every surface has a device flux map set too, which the histogram equals"""
    cs, T, frames = receivers
    maps = fc.maps('lds')
    dev = _traced(ctx, receivers, form, maps)
    got = {}
    for s, (chart, swap, ue, ve) in sorted(maps.items()):
        got[s] = dev.histogram_hits(s, s, ue, ve, proj=fc.projection(frames[s], swap), chart=chart, moments=True)
        plain = dev.histogram_hits(s, s, ue, ve, proj=fc.projection(frames[s], True) if swap else None, chart=chart)
        assert N.array_equal(plain.shape, got[s].sum.shape) and N.allclose(plain, got[s].sum, rtol=1e-12, atol=1e-12 * plain.max())
    reserved = dev.hits_reserved()[0]
    hits = dev.get_hits()
    if form == 'stream':
        assert reserved > len(hits['surf']), 'the streaming form left no unwritten entry in the reserved range'
    assert set(m[0] for m in maps.values()) == set(fc.CHARTS)
    for s, (chart, swap, ue, ve) in sorted(maps.items()):
        ref = hh.reference(hits, s, s, chart, 'absorbed', fc.projection(frames[s], swap), ue, ve)
        _compare(got[s], ref, (form, s, chart))
        fm = dev.get_fluxmap(s)
        assert N.allclose(got[s].sum, fm, rtol=1e-9, atol=1e-9 * fm.max()), (form, s, N.abs(got[s].sum - fm).max())
    dev.close()


# 2 -------------------------------------------------------------------------------------------------------------------------------
DIRECTION_EDGES = {'dir_cosines': (N.linspace(-0.8, 0.8, 10), fc.fs.nonuniform(-0.7, 0.7, 7)),         # clipped both ways
                   'dir_angles': (N.linspace(0., 1.2, 9), N.linspace(0., TWO_PI, 12))}                  # clipped at 1.2 of pi / 2
FULL_CASES = [(s, chart, weight) for s in FULL for chart, weight in
              (('dir_cosines', 'incident'), ('dir_angles', 'count'), ('dir_angles', 'absorbed'), ('dir_cosines', 'count'), ('cylinder', 'incident'))]


def test_direction_charts_incident_energy_and_counts_on_the_full_captures(ctx, receivers):
    """both direction charts, the incident weight and the count on the cylinder and the frustum, all three planes and `outside`"""
    cs, T, frames = receivers
    dev = _traced(ctx, receivers)
    maps = fc.maps('lds')
    got = {}
    for s, chart, weight in FULL_CASES:
        ue, ve = DIRECTION_EDGES[chart] if chart in DIRECTION_EDGES else maps[s][2:]
        got[s, chart, weight] = dev.histogram_hits(s, s, ue, ve, chart=chart, weight=weight, moments=True)
    hits = dev.get_hits()
    assert hits['directions'] is not None
    for s, chart, weight in FULL_CASES:
        ue, ve = DIRECTION_EDGES[chart] if chart in DIRECTION_EDGES else maps[s][2:]
        ref = hh.reference(hits, s, s, chart, weight, fc.projection(frames[s]), ue, ve)
        _compare(got[s, chart, weight], ref, (s, chart, weight))
        if chart in DIRECTION_EDGES:
            assert 0.01 * ref['n'] < ref['outside'][1] < 0.9 * ref['n'] and (ref['count'] > 0).mean() > 0.3, (s, chart, ref['outside'])
        if weight == 'count':
            assert N.array_equal(got[s, chart, weight].sum, ref['count']) and N.array_equal(got[s, chart, weight].sum_sq, ref['count'])
    # the incident energy is not the absorbed energy on these surfaces
    k = N.asarray(hits['surf']) == fc.CYLINDER
    assert N.asarray(hits['e_in'])[k].sum() > 1.5 * N.asarray(hits['e_abs'])[k].sum()
    dev.close()


# 3 -------------------------------------------------------------------------------------------------------------------------------
def _first_beyond(lib, nv, planes):
    nu = 1
    while lib.hh_in_lds(nu, nv, planes):
        nu += 1
    return nu


def test_bins_in_lds_and_in_global_memory(ctx, receivers, lib):
    """the floor's map at 13 x 16, at the largest size whose planes fit the kernel's LDS budget and at the smallest beyond it, taken
    from the decision function, with and without the moment planes"""
    cs, T, frames = receivers
    dev = _traced(ctx, receivers)
    proj = fc.projection(frames[fc.FLOOR], True)
    sizes = {False: [13, _first_beyond(lib, 16, 0) - 1, _first_beyond(lib, 16, 0)],
             True: [13, _first_beyond(lib, 16, 3) - 1, _first_beyond(lib, 16, 3)]}
    assert sizes == {False: [13, 480, 481], True: [13, 166, 167]}
    got = {}
    for moments, nus in sizes.items():
        planes = 3 if moments else 0
        assert [bool(lib.hh_in_lds(nu, 16, planes)) for nu in nus] == [hh.in_lds(nu, 16, planes) for nu in nus] == [True, True, False]
        for nu in nus:
            got[moments, nu] = dev.histogram_hits(fc.FLOOR, fc.FLOOR, fc.fs.nonuniform(0., 2.6, nu), N.linspace(0., TWO_PI, 17), proj=proj,
                                                  chart='polar', moments=moments)
    hits = dev.get_hits()
    for (moments, nu), g in sorted(got.items()):
        ref = hh.reference(hits, fc.FLOOR, fc.FLOOR, 'polar', 'absorbed', proj, fc.fs.nonuniform(0., 2.6, nu), N.linspace(0., TWO_PI, 17))
        if moments:
            _compare(g, ref, ('floor', nu, 'moments'))
        else:
            assert ref['near'] == 0 and g.shape == (nu, 16)
            assert N.allclose(g, ref['sum'], rtol=1e-9, atol=1e-9 * ref['sum'].max()), (nu, N.abs(g - ref['sum']).max())
        assert ref['n'] > 0.2 * N_RAYS and ref['outside'][1] == 0
    dev.close()


# 4 -------------------------------------------------------------------------------------------------------------------------------
def test_a_range_of_surfaces_two_calls_in_one_buffer_and_an_empty_buffer(ctx, receivers):
    from tracer_amd.scene import DeviceScene
    cs, T, frames = receivers
    ue, ve = N.linspace(-2.5, 2.5, 12), fc.fs.nonuniform(-2.5, 2.5, 9)
    proj = fc.projection(frames[fc.CYLINDER])
    dev = _traced(ctx, receivers, seeds=(SEED,))
    first = dev.histogram_hits(fc.CYLINDER, fc.FRUSTUM, ue, ve, weight='count', moments=True)
    dev.close()
    # two calls, nothing read in between: surfaces 2..5 -- two of them captured lean -- in the frame of the cylinder, counted
    dev = _traced(ctx, receivers, seeds=(SEED, SEED + 1))
    both = dev.histogram_hits(fc.CYLINDER, fc.FRUSTUM, ue, ve, weight='count', moments=True)
    one = dev.histogram_hits(fc.SPHERE, fc.SPHERE, ue, ve, proj=proj, weight='count', moments=True)
    hits = dev.get_hits()
    _compare(both, hh.reference(hits, fc.CYLINDER, fc.FRUSTUM, 'xy', 'count', proj, ue, ve), 'surfaces 2..5, two calls')
    _compare(one, hh.reference(hits, fc.SPHERE, fc.SPHERE, 'xy', 'count', proj, ue, ve), 'the sphere in the cylinder\'s frame')
    assert both.count.sum() > 1.8 * first.count.sum() > 0 and both.count.sum() > 2 * one.count.sum() > 0
    # emptied, and never filled
    dev.lib.trc_scene_clear_hits(dev.handle)
    fresh = DeviceScene(cs, ctx)
    fresh.set_hit_capacity(4096)
    never = DeviceScene(cs, ctx)          # (no buffer at all)
    for d in (dev, fresh, never):
        z = d.histogram_hits(fc.CYLINDER, fc.FRUSTUM, ue, ve, weight='count', moments=True)
        assert z.sum.shape == (11, 9) and not z.sum.any() and not z.sum_sq.any() and not z.count.any() and not z.outside.any()
        assert not d.histogram_hits(fc.CYLINDER, fc.CYLINDER, ue, ve, chart='dir_angles', weight='incident').any()
        d.close()


# 5 -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffer_as_it_was(ctx, receivers):
    from tracer_amd import _cabi
    from tracer_amd.scene import DeviceScene, compile_scene
    cs, T, frames = receivers
    dev = _traced(ctx, receivers)
    ue, ve = N.linspace(-1., 1., 5), N.linspace(-1., 1., 4)
    before = dev.histogram_hits(fc.CYLINDER, fc.CYLINDER, ue, ve, moments=True)
    bad = _cabi.TracerAmdValueError
    # what a lean capture never wrote: the message names the surface
    for s in LEAN:
        for kw in (dict(chart='dir_cosines'), dict(chart='dir_angles', weight='count'), dict(weight='incident')):
            with pytest.raises(bad, match='surface %d is captured lean' % s):
                dev.histogram_hits(s, s, ue, ve, **kw)
    with pytest.raises(bad, match='surface %d is captured lean' % fc.SPHERE):
        dev.histogram_hits(fc.CYLINDER, fc.FRUSTUM, ue, ve, weight='incident')
    assert dev.histogram_hits(fc.CYLINDER, fc.FRUSTUM, ue, ve, weight='absorbed').sum() > 0.      # (what it wrote is served)
    # ranges
    for lo, hi in ((-1, 2), (4, 6), (6, 6), (3, 2)):
        with pytest.raises(bad, match='not a range of the scene'):
            dev.histogram_hits(lo, hi, ue, ve, proj=N.eye(4))
    cavity = DeviceScene(compile_scene(fc.fs.cavity()[0]), ctx)           # its surfaces 3 and 6 capture nothing
    for lo, hi in ((3, 3), (6, 6)):
        with pytest.raises(bad, match='captures its hits'):
            cavity.histogram_hits(lo, hi, ue, ve)
    cavity.close()
    # edges, charts, weights
    for u_bad in ([0., 1., 1., 2.], [0., 2., 1.], [0., N.nan, 1.], [0., 1., N.inf], [-N.inf, 0., 1.], [3.], []):
        with pytest.raises(ValueError):
            dev.histogram_hits(fc.CYLINDER, fc.CYLINDER, u_bad, ve)
        with pytest.raises(ValueError):
            dev.histogram_hits(fc.CYLINDER, fc.CYLINDER, ue, u_bad)
    p, u1, v1 = _cabi.f64(N.eye(4)[:3].ravel()), _cabi.f64([0.]), _cabi.f64(ve)
    out = N.empty(3)
    d = _cabi.HitHistDesc(fc.CYLINDER, fc.CYLINDER, 0, 0, 0, 3, _cabi.ptr(u1), _cabi.ptr(v1), _cabi.ptr(p))
    import ctypes as C
    assert dev.lib.trc_scene_histogram_hits(dev.handle, C.byref(d), _cabi.ptr(out), None, None, None) == _cabi.ERR_INVALID
    for kw, msg in ((dict(chart=6), 'unknown chart'), (dict(chart=-1), 'unknown chart'), (dict(weight=3), 'unknown weight')):
        with pytest.raises(bad, match=msg):
            dev.histogram_hits(fc.CYLINDER, fc.CYLINDER, ue, ve, **kw)
    with pytest.raises(ValueError, match='unknown histogram chart'):
        dev.histogram_hits(fc.CYLINDER, fc.CYLINDER, ue, ve, chart='conical')
    with pytest.raises(ValueError, match='unknown histogram weight'):
        dev.histogram_hits(fc.CYLINDER, fc.CYLINDER, ue, ve, weight='emitted')
    # the buffer is as it was: the same histogram, and the hits read back
    after = dev.histogram_hits(fc.CYLINDER, fc.CYLINDER, ue, ve, moments=True)
    assert N.array_equal(after.count, before.count) and N.array_equal(after.outside, before.outside)
    hits = dev.get_hits()
    _compare(after, hh.reference(hits, fc.CYLINDER, fc.CYLINDER, 'xy', 'absorbed', fc.projection(frames[fc.CYLINDER]), ue, ve), 'after the refusals')
    assert len(hits['surf']) == dev.get_tallies()[2].sum()
    dev.close()


# 6 -------------------------------------------------------------------------------------------------------------------------------
def test_engine_and_receiver_model_histograms(ctx):
    """TracerEngine.histogram_hits after ray_tracer(tree=False): a surface, an index, a pair, swap_xy; decided after the trace, twice on
    the same surface, beside a flux map declared before it"""
    from tracer_amd.tracer_engine import TracerEngine
    asm, objs, T = fc.receivers()
    surfs = asm.get_surfaces()
    eng = TracerEngine(asm)
    maps = fc.maps('lds')
    chart, swap, ue, ve = maps[fc.FLOOR]
    eng.set_fluxmap(surfs[fc.CYLINDER], *maps[fc.CYLINDER][2:], chart='cylinder')
    eng.ray_tracer(fc.source(N_RAYS, T, SEED), REPS, EMIN, tree=False, seed=SEED)
    floor = eng.histogram_hits(surfs[fc.FLOOR], ue, ve, chart=chart, swap_xy=swap, moments=True)
    cyl = eng.histogram_hits(fc.CYLINDER, *maps[fc.CYLINDER][2:], chart='cylinder')
    ang = eng.histogram_hits(surfs[fc.CYLINDER], *DIRECTION_EDGES['dir_angles'], chart='dir_angles', weight='incident', moments=True)
    pair = eng.histogram_hits((fc.CYLINDER, fc.FRUSTUM), N.linspace(-2.5, 2.5, 12), N.linspace(-2.5, 2.5, 9), weight='count', moments=True)
    hits = eng._dev.get_hits()
    frames = [N.array(s._temp_frame) for s in eng._dev.compiled.surfaces]
    _compare(floor, hh.reference(hits, fc.FLOOR, fc.FLOOR, chart, 'absorbed', fc.projection(frames[fc.FLOOR], swap), ue, ve), 'engine, floor')
    _compare(ang, hh.reference(hits, fc.CYLINDER, fc.CYLINDER, 'dir_angles', 'incident', fc.projection(frames[fc.CYLINDER]),
                               *DIRECTION_EDGES['dir_angles']), 'engine, angles on the cylinder')
    _compare(pair, hh.reference(hits, fc.CYLINDER, fc.FRUSTUM, 'xy', 'count', fc.projection(frames[fc.CYLINDER]), N.linspace(-2.5, 2.5, 12),
                                N.linspace(-2.5, 2.5, 9)), 'engine, a pair')
    fm = eng.get_fluxmap(fc.CYLINDER)
    assert N.allclose(cyl, fm, rtol=1e-9, atol=1e-9 * fm.max()) and fm.sum() > 0.
    # the accountants read afterwards hold the same hits
    e_abs = surfs[fc.FLOOR].get_optics_manager().get_all_hits()[0]
    assert len(e_abs) == floor.count.sum() + floor.outside[1]


def test_homogenized_receiver_histogram_from_the_device(ctx):
    """HomogenizedLocalReceiver.histogram_hits(engine=...) is the triple the accountants give, without reading them"""
    from tracer_amd.models.tau_minidish import MiniDish
    from tracer_amd.tracer_engine import TracerEngine
    from tracer_amd.sources import solar_disk_bundle
    from tracer_amd.spatial_geometry import rotx
    dish = MiniDish(5., 6.25, 0.9, 6.95, 0.4, 0.7, 0.9)         # (the dish of the reference's example, as test_gpu_parity.py poses it)
    dish.set_transform(rotx(-N.pi / 4))
    eng = TracerEngine(dish)
    n, x = 200000, -1. / N.sqrt(2.)
    eng.ray_tracer(solar_disk_bundle(n, N.c_[[0, 7., 7.]], N.array([0, x, x]), 3., 0.005, flux=1000., seed=41), 100, 1e-6, tree=False, seed=41)
    H, xe, ye = dish.histogram_hits(bins=20, engine=eng)
    Hh, xh, yh = dish.histogram_hits(bins=20)
    assert N.array_equal(xe, xh) and N.array_equal(ye, yh) and H.shape == Hh.shape == (20, 20)
    plate, = dish.get_receiver_surf().get_surfaces()
    local = plate.global_to_local(plate.get_optics_manager().get_all_hits()[1])
    assert not (fc.near_edge(local[0], xe) | fc.near_edge(local[1], ye)).any(), 'INPUT CONDITION: a hit within 1e-12 of an edge'
    assert Hh.sum() > 0. and (Hh > 0).mean() > 0.1
    assert N.allclose(H, Hh, rtol=1e-9, atol=1e-9 * Hh.max()), N.abs(H - Hh).max()


# 7 -------------------------------------------------------------------------------------------------------------------------------
def _two_targets(transmitting):
    from tracer_amd.models.solar_simulator import SolarSimulator, Target
    A, C_ = 0.3, 0.5
    F = N.sqrt(C_ ** 2 - A ** 2)
    cdf = N.array([N.linspace(0., N.pi, 13), 0.5 * (1. - N.cos(N.linspace(0., N.pi, 13)))]).T      # an isotropic lamp's
    edges = N.linspace(-0.1, 0.1, 11)
    down = N.array([0., 0., -1.])
    first = Target(0.2, 0.2, N.array([0., 0., 2. * F - 0.02]), down, edges, edges[::2], transmitting=transmitting)
    second = Target(0.2, 0.2, N.array([0., 0., 2. * F]), down, edges, edges[::2])
    sim = SolarSimulator([N.zeros(3)], [N.array([0., 0., 1.])], [dict(a=A, b=A, c=C_, zlim=[-C_, 0.], lampdict=dict(model='Bader', theta_CDF=cdf))],
                         [first, second])
    return sim, first, second


def test_a_transmitting_target_in_front_of_an_absorbing_one(ctx):
    """one lamp, one batch of 2e4 rays: the transmitting plate maps the energy that arrives and lets it pass -- its map is the host
    histogram of its hits' incident energy -- and the plate 2 cm behind it, which an absorbing plate in front shadows completely, is
    lit through it"""
    n = 20000
    sim, first, second = _two_targets(True)
    assert first.transmitting and not second.transmitting
    est = sim.simulate(nrays=n, ray_batch=n, seed=5)
    i1, i2 = [sim.get_surfaces().index(t.get_surfaces()[0]) for t in (first, second)]
    m1, m2 = est[0].mean * first.areas, est[1].mean * second.areas
    hits = sim.engine._dev.get_hits()               # (the batch's hits are still on the device)
    absorbed, received, count = sim.engine.get_tallies()
    k = N.nonzero(N.asarray(hits['surf']) == i1)[0]
    assert len(k) == count[i1] > 0.05 * n and not N.asarray(hits['e_abs'])[k].any()
    u, v = fc.chart_uv('xy', fc.projection(sim.engine._dev.compiled.surfaces[i1]._temp_frame), N.asarray(hits['points'])[:, k])
    assert not (fc.near_edge(u, first.binx) | fc.near_edge(v, first.biny)).any(), 'INPUT CONDITION: a hit within 1e-12 of an edge'
    want = N.histogram2d(u, v, bins=[first.binx, first.biny], weights=N.asarray(hits['e_in'])[k])[0]
    assert m1.shape == want.shape == (10, 5) and want.sum() > 0.
    assert N.allclose(m1, want, rtol=1e-9, atol=1e-9 * want.max()), N.abs(m1 - want).max()
    assert absorbed[i1] == 0.
    # behind it: lit, by rays that all crossed the first plate
    assert m2.sum() > 0. and N.isclose(m2.sum(), absorbed[i2], rtol=1e-9) and 0 < count[i2] <= count[i1]
    assert absorbed[i2] > 0.5 * want.sum()
    # ... for an absorbing plate in the same place leaves it dark
    dark, f0, s0 = _two_targets(False)
    e0 = dark.simulate(nrays=n, ray_batch=n, seed=5)
    c0 = dark.engine.get_tallies()[2]
    j1, j2 = [dark.get_surfaces().index(t.get_surfaces()[0]) for t in (f0, s0)]
    assert c0[j1] == count[i1] and c0[j2] == 0 and not e0[1].mean.any()
    assert N.allclose(e0[0].mean * f0.areas, m1, rtol=1e-9, atol=1e-9 * want.max())       # what it absorbs is what the other lets pass
