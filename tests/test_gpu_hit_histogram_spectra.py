"""
GPU tests of the spectral histogram of captured hits (trc_scene_histogram_hits_x, k_hist_hits_x), run with -m gpu on the MI355X box.

The scenes and the source are those of test_gpu_poly_source.py -- the polychromatic box, whose floor is the capturing polychromatic
wall, alone and with the slab that splits rays -- at 20 000 rays through DeviceScene.trace_fast in its streaming form: many
workgroups, the grid-stride loop, unwritten entries in the reserved range.  The reference of every assertion is NumPy on
dev.get_hits(), read AFTER the histogram calls, with the NumPy formulas of the charts (hit_histogram_cases.hit_uv): counts and
outside_n exact, sums to rtol 1e-9, atol 1e-9 of the largest bin -- the tolerances of test_gpu_hit_histogram.py, and its input
condition: no selected hit within 1e-12 of a map's span from an edge (a seed that fails it is replaced, the tolerance is not
widened).  The oracle is not involved.
"""
import ctypes as C

import numpy as N
import pytest

import hit_histogram_spectra_cases as hx
from test_gpu_poly_source import scene, source, spectrum, CYL_EDGES, MIN_ENERGY

hh, fc = hx.hh, hx.fc
pytestmark = pytest.mark.gpu

N_RAYS, SEED, REPS = 20000, 77, 3
FLOOR = 0
WEIGHTS = ('absorbed', 'incident')


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


@pytest.fixture(scope='module')
def lib():
    return hx.host_library()


def _traced(ctx, kind, specs, reps=REPS, fluxmap=None):
    """a device scene that holds the hits of one streaming call per spectrum (seeds SEED, SEED + 1 ..), none read yet; the hits each
    call captured on the floor"""
    from tracer_amd.scene import DeviceScene
    cs = scene(kind)[1]
    assert cs.capture[FLOOR]
    dev = DeviceScene(cs, ctx)
    if fluxmap is not None:
        dev.set_fluxmap(FLOOR, *fluxmap)
    room = 4 * reps * N_RAYS + 65536
    dev.set_hit_capacity(room)
    made = []
    for j, sp in enumerate(specs):
        if j:
            dev.reserve_hits((j + 1) * room)
        before = dev.get_tallies()[2][FLOOR]
        st, _ = dev.trace_fast(source(N_RAYS, sp, seed=SEED + j), reps, MIN_ENERGY, SEED + j, stream=True)
        assert st.hits_dropped == 0 and st.launches > 1
        made.append(int(dev.get_tallies()[2][FLOOR] - before))
    return dev, made


def _frame(kind, s=FLOOR):
    return N.array(scene(kind)[1].surfaces[s]._temp_frame)


def _edges(nu, nv):
    """a map clipped to a part of the floor (the hits spread over about -1.6 .. 1.6 either way), uneven in v"""
    return N.linspace(-1.1, 0.9, nu + 1), fc.fs.nonuniform(-0.8, 1.2, nv)


def _compare(got, ref, what, wl=None, off_grid=0):
    """a SpectralHistogram against hit_histogram_spectra_cases.reference"""
    assert ref['near'] == 0, ('INPUT CONDITION, not the histogram: %d hits within %g of the span of an edge -- choose another seed'
                              % (ref['near'], fc.EDGE_EPS), what)
    assert ref['n'] > 0 and ref['count'].sum() > 0 and got.sum.shape == ref['sum'].shape, what
    big = N.abs(ref['sum']).max()
    print('%s: %s, %d hits, %d outside, largest difference %.3g of %.3g' % (what, got.sum.shape, ref['n'], ref['outside_n'],
                                                                          N.abs(got.sum - ref['sum']).max(), big))
    if got.count is not None:
        assert N.array_equal(got.count, ref['count']), (what, N.abs(got.count - ref['count']).max())
    assert got.outside_n == ref['outside_n'] and got.off_grid == off_grid, (what, got.outside_n, got.off_grid)
    assert N.allclose(got.sum, ref['sum'], rtol=1e-9, atol=1e-9 * big), (what, N.abs(got.sum - ref['sum']).max(), big)
    assert N.allclose(got.outside, ref['outside'], rtol=1e-9, atol=1e-9 * big), (what, N.abs(got.outside - ref['outside']).max())
    assert (got.wavelengths is None) if wl is None else N.array_equal(got.wavelengths, wl)


# 1 -------------------------------------------------------------------------------------------------------------------------------
SHAPES = {2: [(1, 1, False), (4, 5, True)],
          3: [(1, 1, True), (4, 5, False), (100, 100, False), (100, 100, True)],
          7: [(1, 1, False), (4, 5, True), (40, 40, False), (40, 40, True)]}
FORM = {(1, 1): 'whole', (4, 5): 'whole', (40, 40): 'sliced', (100, 100): 'global'}


@pytest.mark.parametrize('W', sorted(SHAPES))
def test_maps_of_the_floor_whole_in_lds_sliced_and_in_global_memory(ctx, lib, W):
    """the 'xy' chart on the floor, clipped so that hits are outside, both weights: 1 x 1 and 4 x 5 fit LDS whole, 40 x 40 at 7 samples
    is sliced 5 + 2 without the count plane and 4 + 3 with it, 100 x 100 has its bins in global memory -- as the plan function says"""
    sp = spectrum(W)
    wl = sp.table()[0]
    dev, _ = _traced(ctx, 'box', [sp])
    got = {}
    for nu, nv, counts in SHAPES[W]:
        in_lds, ks, slices, nbytes = hx.library_plan(lib, nu, nv, W, counts)
        form = 'global' if not in_lds else 'whole' if slices == 1 else 'sliced'
        assert form == FORM[nu, nv] and (in_lds, ks, slices, nbytes) == hx.plan(nu, nv, W, counts), (nu, nv, W, counts, in_lds, ks, slices)
        if form == 'sliced':
            assert (ks, slices, W % ks) == ((4, 2, 3) if counts else (5, 2, 2))          # a partial last slice
        for weight in WEIGHTS:
            got[nu, nv, counts, weight] = dev.histogram_spectra(FLOOR, FLOOR, *_edges(nu, nv), weight=weight, wavelengths=wl, counts=counts)
    loose = dev.histogram_spectra(FLOOR, FLOOR, *_edges(4, 5), counts=True)          # (no grid: the wavelength columns are not read)
    reserved = dev.hits_reserved()[0]
    hits = dev.get_hits()
    assert reserved > len(hits['surf']) > N_RAYS // 2, 'the streaming form left no unwritten entry in the reserved range'
    assert N.array_equal(hits['spectra'][2], N.tile(wl[:, None], (1, len(hits['surf']))))
    proj = fc.projection(_frame('box'))
    for (nu, nv, counts, weight), g in sorted(got.items()):
        ref = hx.reference(hits, FLOOR, FLOOR, 'xy', weight, proj, *_edges(nu, nv))
        _compare(g, ref, (W, nu, nv, counts, weight), wl)
        assert (g.count is not None) == counts and 0.02 * ref['n'] < ref['outside_n'] < 0.9 * ref['n']
    _compare(loose, hx.reference(hits, FLOOR, FLOOR, 'xy', 'absorbed', proj, *_edges(4, 5)), (W, 'no grid'))
    if (4, 5, True, 'absorbed') in got:
        assert N.array_equal(loose.count, got[4, 5, True, 'absorbed'].count)
    # the wall absorbs a part of what arrives
    a, i = got[1, 1, SHAPES[W][0][2], 'absorbed'], got[1, 1, SHAPES[W][0][2], 'incident']
    assert (0. < a.sum).all() and (a.sum < i.sum).all()
    dev.close()


# 2 -------------------------------------------------------------------------------------------------------------------------------
def test_cylinder_chart_and_direction_angles(ctx):
    """the floor in the cylinder chart of the poly-source tests (1 x 6), and by the angles of the incident direction where the floor
    is captured in full; a lean capture refuses the direction chart and the incident weight, naming the surface"""
    from tracer_amd import _cabi
    W = 3
    sp = spectrum(W)
    wl = sp.table()[0]
    dev, _ = _traced(ctx, 'box', [sp])
    lean = bool(scene('box')[1].descs[FLOOR].flags & _cabi.SURF_CAPTURE_LEAN)
    ang = (N.linspace(0., 0.3, 9), N.linspace(0., 2. * N.pi, 12))        # clipped at 0.3 of pi / 2
    cyl = dev.histogram_spectra(FLOOR, FLOOR, *CYL_EDGES, chart='cylinder', wavelengths=wl, counts=True)
    if lean:
        for kw in (dict(chart='dir_angles'), dict(weight='incident')):
            with pytest.raises(_cabi.TracerAmdValueError, match='surface %d is captured lean' % FLOOR):
                dev.histogram_spectra(FLOOR, FLOOR, *ang, wavelengths=wl, **kw)
    else:
        dirs = [dev.histogram_spectra(FLOOR, FLOOR, *ang, chart='dir_angles', weight=w, wavelengths=wl, counts=True) for w in WEIGHTS]
    hits = dev.get_hits()
    proj = fc.projection(_frame('box'))
    ref = hx.reference(hits, FLOOR, FLOOR, 'cylinder', 'absorbed', proj, *CYL_EDGES)
    _compare(cyl, ref, 'cylinder chart', wl)
    assert cyl.sum.shape == (1, 6, W) and (ref['count'] > 0).all() and ref['outside_n'] == 0
    if not lean:
        assert hits['directions'] is not None
        for w, g in zip(WEIGHTS, dirs):
            ref = hx.reference(hits, FLOOR, FLOOR, 'dir_angles', w, proj, *ang)
            _compare(g, ref, ('dir_angles', w), wl)
            assert 0 < ref['outside_n'] < ref['n'] and (ref['count'] > 0).mean() > 0.3
    dev.close()


# 3 -------------------------------------------------------------------------------------------------------------------------------
def test_spectra_per_surface_of_the_split_scene(ctx):
    """surface_spectra over the whole scene with the slab that splits rays: a row per surface, zero rows for those that capture
    nothing, the sums per surface of the hit list; integrate() is the trapezoid rule over the rows"""
    from tracer_amd import _cabi
    W = 3
    sp = spectrum(W)
    wl = sp.table()[0]
    cs = scene('split')[1]
    dev, _ = _traced(ctx, 'split', [sp], reps=4)
    hi = cs.n_surf - 1
    got = dev.surface_spectra(0, hi, wavelengths=wl)
    floor = dev.surface_spectra(FLOOR, FLOOR)
    lean = [bool(cs.descs[s].flags & _cabi.SURF_CAPTURE_LEAN) for s in range(cs.n_surf)]
    full = [s for s in range(cs.n_surf) if cs.capture[s] and not lean[s]]
    arrived = dict((s, dev.surface_spectra(s, s, weight='incident', wavelengths=wl)) for s in full)
    dark = [s for s in range(cs.n_surf) if not cs.capture[s]]
    assert dark, 'every surface of the split scene captures: no zero row to look at'
    with pytest.raises(_cabi.TracerAmdValueError, match='captures its hits'):
        dev.surface_spectra(dark[0], dark[0])
    hits = dev.get_hits()
    ref = hx.reference_by_surface(hits, 0, hi, 'absorbed')
    big = N.abs(ref['sum']).max()
    assert got.sum.shape == (cs.n_surf, W) and N.array_equal(got.count, ref['count']) and got.off_grid == 0 and got.outside_n == 0
    assert N.allclose(got.sum, ref['sum'], rtol=1e-9, atol=1e-9 * big), N.abs(got.sum - ref['sum']).max()
    assert not got.sum[dark].any() and not got.count[dark].any() and got.count[FLOOR] > N_RAYS // 2 and not got.outside.any()
    assert N.allclose(floor.sum[0], got.sum[FLOOR], rtol=1e-9, atol=0.)
    assert floor.wavelengths is None and floor.count[0] == got.count[FLOOR]
    for s, g in arrived.items():
        want = hx.reference_by_surface(hits, s, s, 'incident')
        assert N.array_equal(g.count, want['count']) and N.allclose(g.sum, want['sum'], rtol=1e-9, atol=1e-9 * N.abs(want['sum']).max())
    trapz = getattr(N, 'trapezoid', None) or N.trapz
    assert N.allclose(got.integrate(), trapz(ref['sum'], wl, axis=-1), rtol=1e-9, atol=1e-9 * trapz(ref['sum'], wl, axis=-1).max())
    assert N.array_equal(got.integrate(), trapz(got.sum, wl, axis=-1)) and got.integrate()[FLOOR] > 0.
    with pytest.raises(ValueError, match='without wavelengths'):
        floor.integrate()
    dev.close()


# 4 -------------------------------------------------------------------------------------------------------------------------------
def _other_grid():
    from tracer_amd.source_spectrum import SourceSpectrum
    wl = N.array([0.3e-6, 1.0e-6, 2.5e-6])
    assert not N.isin(wl, spectrum(3).table()[0]).any()
    return SourceSpectrum.polychromatic(wl, 1.5 + N.sin(4e6 * wl))


def test_two_sample_grids_in_one_buffer(ctx):
    """two calls of 3 samples on different grids, the second behind the first (reserve_hits): held to the first grid every sample of
    the second call's hits is off it and left out, the other way round the first call's; without a grid both are binned"""
    first, second = spectrum(3), _other_grid()
    dev, made = _traced(ctx, 'box', [first, second])
    ue, ve = _edges(4, 5)
    on = [dev.histogram_spectra(FLOOR, FLOOR, ue, ve, wavelengths=sp.table()[0], counts=True) for sp in (first, second)]
    by = dev.surface_spectra(FLOOR, FLOOR, weight='incident', wavelengths=first.table()[0])
    both = dev.histogram_spectra(FLOOR, FLOOR, ue, ve, counts=True)
    hits = dev.get_hits()
    assert len(hits['surf']) >= sum(made) and min(made) > N_RAYS // 2
    assert on[0].off_grid == 3 * made[1] and on[1].off_grid == 3 * made[0] and by.off_grid == 3 * made[1] and both.off_grid == 0
    proj = fc.projection(_frame('box'))
    _compare(both, hx.reference(hits, FLOOR, FLOOR, 'xy', 'absorbed', proj, ue, ve), 'both grids, none given')
    for g, sp in zip(on, (first, second)):
        skip = hits['spectra'][2] != sp.table()[0][:, None]
        assert skip.sum() == g.off_grid and skip.all(axis=0).sum() * 3 == g.off_grid
        ref = hx.reference(hits, FLOOR, FLOOR, 'xy', 'absorbed', proj, ue, ve, skip=skip)
        _compare(g, ref, 'one grid of two', sp.table()[0], off_grid=g.off_grid)
        assert N.array_equal(g.count, both.count)       # the hits are counted all the same
    want = hx.reference_by_surface(hits, FLOOR, FLOOR, 'incident', skip=hits['spectra'][2] != first.table()[0][:, None])
    assert N.allclose(by.sum, want['sum'], rtol=1e-9, atol=1e-9 * want['sum'].max()) and by.count[0] == sum(made)
    dev.close()


def test_engine_methods_take_the_grid_of_the_last_call_and_refuse_another(ctx):
    """TracerEngine.histogram_spectra and surface_spectra after ray_tracer(tree=False): the grid of the carried spectrum, a surface or
    an index, the whole scene; hits of another grid behind them in the buffer are a ValueError that states the count"""
    from tracer_amd.tracer_engine import TracerEngine
    from test_gpu_media import _poly_scene
    asm = _poly_scene()[0]              # (the box, an assembly of this test's own: its accountants are promised the hits)
    sp = spectrum(3)
    wl = sp.table()[0]
    eng = TracerEngine(asm)
    eng.ray_tracer(source(N_RAYS, sp), reps=REPS, min_energy=MIN_ENERGY, tree=False, seed=SEED)
    assert eng.stats['engine'] == 'fast' and eng.stats['form'] == 'stream'
    ue, ve = _edges(4, 5)
    floor = eng.histogram_spectra(asm.get_surfaces()[FLOOR], ue, ve, counts=True)
    swapped = eng.histogram_spectra(FLOOR, ve, ue, swap_xy=True, wavelengths=wl)
    rows = eng.surface_spectra()
    one = eng.surface_spectra(FLOOR)
    dev = eng._dev
    hits = dev.get_hits()
    frame = N.array(dev.compiled.surfaces[FLOOR]._temp_frame)
    _compare(floor, hx.reference(hits, FLOOR, FLOOR, 'xy', 'absorbed', fc.projection(frame), ue, ve), 'engine, floor', wl)
    _compare(swapped, hx.reference(hits, FLOOR, FLOOR, 'xy', 'absorbed', fc.projection(frame, True), ve, ue), 'engine, swap_xy', wl)
    ref = hx.reference_by_surface(hits, 0, dev.n_surf - 1, 'absorbed')
    assert rows.sum.shape == (dev.n_surf, 3) and N.array_equal(rows.count, ref['count']) and N.array_equal(rows.wavelengths, wl)
    assert N.allclose(rows.sum, ref['sum'], rtol=1e-9, atol=1e-9 * ref['sum'].max()) and N.array_equal(one.count, rows.count[:1])
    assert N.allclose(one.sum[0], rows.sum[FLOOR], rtol=1e-9, atol=0.)
    # hits of another grid, left behind the first call's
    used = dev.hits_reserved()[0]
    dev.reserve_hits(used + 4 * REPS * N_RAYS + 65536)
    before = dev.get_tallies()[2][FLOOR]
    st, _ = dev.trace_fast(source(N_RAYS, _other_grid(), seed=SEED + 1), REPS, MIN_ENERGY, SEED + 1, stream=True)
    n_other = int(dev.get_tallies()[2][FLOOR] - before)
    assert st.hits_dropped == 0 and n_other > N_RAYS // 2
    for call in (lambda: eng.histogram_spectra(FLOOR, ue, ve), lambda: eng.surface_spectra(FLOOR), lambda: eng.surface_spectra()):
        with pytest.raises(ValueError, match='%d samples' % (3 * n_other)):
            call()
    assert eng._dev.surface_spectra(FLOOR, FLOOR).count[0] == one.count[0] + n_other
    # a call whose source carries no spectrum leaves no grid: the engine asks for one
    asm2, objs, T = fc.receivers()
    eng2 = TracerEngine(asm2)
    eng2.ray_tracer(fc.source(N_RAYS, T, 11), 12, 1e-10, tree=False, seed=11)
    with pytest.raises(ValueError, match='give the wavelengths'):
        eng2.surface_spectra(fc.CYLINDER)


# 5 -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_buffers(ctx):
    from tracer_amd import _cabi
    from tracer_amd.scene import DeviceScene, compile_scene
    bad = _cabi.TracerAmdValueError
    ue, ve = _edges(4, 5)
    # hits of rays that carry no spectrum: no spectral columns
    asm, objs, T = fc.receivers()
    plain = DeviceScene(compile_scene(asm), ctx)
    plain.set_hit_capacity(2 * N_RAYS + 65536)
    st, _ = plain.trace_fast(fc.source(N_RAYS, T, 11), 12, 1e-10, 11, accel=True, stream=True)
    assert plain.hit_spectral_columns() == 0 and plain.hits_reserved()[0] > 0
    for call in (lambda: plain.histogram_spectra(fc.CYLINDER, fc.CYLINDER, ue, ve), lambda: plain.surface_spectra(fc.CYLINDER, fc.FRUSTUM),
                 lambda: plain.histogram_spectra(fc.CYLINDER, fc.CYLINDER, ue, ve, wavelengths=[1e-6, 2e-6])):
        with pytest.raises(bad, match='no spectral columns'):
            call()
    assert plain.histogram_hits(fc.CYLINDER, fc.CYLINDER, N.linspace(-2.5, 2.5, 5), N.linspace(-2.5, 2.5, 4)).sum() > 0.   # (still served)
    plain.close()
    W = 3
    sp = spectrum(W)
    wl = sp.table()[0]
    dev, _ = _traced(ctx, 'box', [sp])
    before = dev.histogram_spectra(FLOOR, FLOOR, ue, ve, wavelengths=wl, counts=True)
    # another number of samples than the buffer's
    with pytest.raises(ValueError, match='4 wavelengths for hits of 3 samples'):
        dev.histogram_spectra(FLOOR, FLOOR, ue, ve, wavelengths=N.linspace(1e-6, 2e-6, 4))
    u, v, p = _cabi.f64(ue), _cabi.f64(ve), _cabi.f64(N.eye(4)[:3].ravel())
    out, outside = N.empty(4 * 5 * 4), N.empty(5)
    for n_samples, msg in ((2, 'holds 9 spectral columns'), (4, 'holds 9 spectral columns'), (0, '0 samples'), (-1, '-1 samples')):
        d = _cabi.HitHistXDesc(_cabi.HitHistDesc(FLOOR, FLOOR, 0, 0, 4, 5, _cabi.ptr(u), _cabi.ptr(v), _cabi.ptr(p)), n_samples, 0, None)
        assert dev.lib.trc_scene_histogram_hits_x(dev.handle, C.byref(d), _cabi.ptr(out), None, _cabi.ptr(outside), None) == _cabi.ERR_INVALID
        assert msg in dev.lib.trc_last_error().decode(), (n_samples, dev.lib.trc_last_error())
    # the weight, a grid that is not finite, and what trc_scene_histogram_hits refuses
    with pytest.raises(bad, match='the weight is the absorbed or the incident spectrum'):
        dev.histogram_spectra(FLOOR, FLOOR, ue, ve, weight='count')
    with pytest.raises(bad, match='the weight is the absorbed or the incident spectrum'):
        dev.surface_spectra(FLOOR, FLOOR, weight='count')
    with pytest.raises(ValueError, match='unknown histogram weight'):
        dev.surface_spectra(FLOOR, FLOOR, weight='emitted')
    for w_bad in ([N.nan, 1e-6, 2e-6], [1e-6, N.inf, 2e-6]):
        with pytest.raises(bad, match='wl holds a value that is not finite'):
            dev.surface_spectra(FLOOR, FLOOR, wavelengths=w_bad)
    n_surf = dev.n_surf
    for lo, hi in ((-1, 0), (0, n_surf), (n_surf, n_surf), (1, 0)):
        with pytest.raises(bad, match='not a range of the scene'):
            dev.surface_spectra(lo, hi)
        with pytest.raises(bad, match='not a range of the scene'):
            dev.histogram_spectra(lo, hi, ue, ve, proj=N.eye(4))
    for kw, msg in ((dict(chart=6), 'unknown chart'), (dict(chart=-1), 'unknown chart')):
        with pytest.raises(bad, match=msg):
            dev.histogram_spectra(FLOOR, FLOOR, ue, ve, **kw)
    for u_bad in ([0., 1., 1., 2.], [0., N.nan, 1.], [3.]):
        with pytest.raises(ValueError):
            dev.histogram_spectra(FLOOR, FLOOR, u_bad, ve)
    # the buffer is as it was; emptied, and never filled, it gives zeros
    after = dev.histogram_spectra(FLOOR, FLOOR, ue, ve, wavelengths=wl, counts=True)
    assert N.array_equal(after.count, before.count) and after.outside_n == before.outside_n and after.count.sum() > N_RAYS // 4
    dev.lib.trc_scene_clear_hits(dev.handle)
    never = DeviceScene(scene('box')[1], ctx)
    for d, shape in ((dev, W), (never, 1)):
        z = d.histogram_spectra(FLOOR, FLOOR, ue, ve, counts=True)
        assert z.sum.shape == (4, 5, shape) and not z.sum.any() and not z.count.any() and not z.outside.any() and (z.outside_n, z.off_grid) == (0, 0)
        s = d.surface_spectra(0, n_surf - 1)
        assert s.sum.shape == (n_surf, shape) and not s.sum.any() and not s.count.any()
    z = never.histogram_spectra(FLOOR, FLOOR, ue, ve, wavelengths=N.linspace(1e-6, 2e-6, 4))
    assert z.sum.shape == (4, 5, 4) and not z.sum.any() and z.count is None
    dev.close()
    never.close()


# 6 -------------------------------------------------------------------------------------------------------------------------------
def _sorted_hits(hits):
    cols = N.vstack([hits['surf'].astype(float), hits['e_abs'], hits['e_in'], hits['points']] +
                    ([hits['directions']] if hits['directions'] is not None else []) + list(hits['spectra']))
    return cols[:, N.lexsort(cols[::-1])]


def test_the_buffer_the_tallies_and_a_flux_map_stay_as_they_are(ctx, lib):
    """after histograms of every form, get_hits, get_tallies and a flux map set on the floor are those of a second identical scene that
    was traced and never histogrammed: the hits the same multiset to the bit, the tallies and the map to the order of their sums"""
    W = 7
    sp = spectrum(W)
    wl = sp.table()[0]
    fm = _edges(13, 16)
    dev, _ = _traced(ctx, 'box', [sp], fluxmap=fm)
    twin, _ = _traced(ctx, 'box', [sp], fluxmap=fm)
    for nu, nv, counts in ((4, 5, True), (40, 40, False), (100, 100, True)):
        for weight in WEIGHTS:
            dev.histogram_spectra(FLOOR, FLOOR, *_edges(nu, nv), weight=weight, wavelengths=wl, counts=counts)
    dev.histogram_spectra(FLOOR, FLOOR, *CYL_EDGES, chart='cylinder')
    dev.surface_spectra(0, dev.n_surf - 1, wavelengths=wl)
    with pytest.raises(ValueError):
        dev.histogram_spectra(FLOOR, FLOOR, *_edges(4, 5), weight='count')
    mine, theirs = dev.get_hits(), twin.get_hits()
    a, b = _sorted_hits(mine), _sorted_hits(theirs)
    assert a.shape == b.shape and a.shape[1] > N_RAYS and N.array_equal(a, b)
    for x, y, exact in zip(dev.get_tallies(), twin.get_tallies(), (False, False, True)):
        assert N.array_equal(x, y) if exact else N.allclose(x, y, rtol=1e-9, atol=1e-12), (x, y)
    m1, m2 = dev.get_fluxmap(FLOOR), twin.get_fluxmap(FLOOR)
    assert m2.sum() > 0. and N.allclose(m1, m2, rtol=1e-9, atol=1e-9 * m2.max())
    dev.close()
    twin.close()
