"""
GPU tests of polychromatic sources (SourceSpectrum.polychromatic: every source ray carries the whole table), run with -m gpu on the
MI355X box.

A pending source bundle with a carried spectrum is traced by the streaming form of the fast engine (k_s_shade_p: sample grid and
birth spectrum per workgroup, nothing of size W x n uploaded) and by the ordered engine (level 0 gets its (W, n) columns on the
device).  The reference of every trace is oracle.engine.trace_bundle on the rays oracle.sources.generate makes for the descriptor,
with the tiled table()[0] as sample wavelengths and e * table()[1] as spectra, on the same Philox streams.  Hits per surface,
segments and events are exact; absorbed and received energy and flux maps hold to rtol 1e-9; captured hits are matched after
sorting, points to 1e-12, sample wavelengths exactly, spectra in and out to rtol 1e-12; survivors to 1e-9, their spectra to rtol
1e-12.  No ray or hit is left out.

The scenes: the polychromatic box of test_gpu_media.py (a capturing polychromatic wall for a floor, a mirror for a roof, a diffuse
side wall) -- alone (the LDS instance, the walls' lambda cells staged), with a surface whose optics table is beyond LDS (the global
instance, as split_cases.py makes one), and with a slab that splits rays in front of the wall.  The sample grids have points below,
on and beyond the nodes of the wall's lambda table (0.25e-6 .. 2.6e-6, 5 nodes).
"""
import ctypes as C
import functools
import os
import types

import numpy as N
import pytest

import fluxmap_chart_scene as fcs
import split_cases
from test_gpu_media import _poly_scene

pytestmark = pytest.mark.gpu

N_RAYS = 293            # not a multiple of 64
SEED, OFFSET = 77, 500
MIN_ENERGY = 1e-9
NODES = N.linspace(0.25e-6, 2.6e-6, 5)          # the lambda nodes of the wall's table (_poly_scene)
CYL_EDGES = (N.array([-0.5, 0.5]), N.linspace(0., 2. * N.pi, 7))        # the floor in the cylinder chart: (local z, azimuth), 1 x 6


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


def spectrum(W, ref_index=1.):
    """W points from below the wall's first node to beyond its last, some of them on nodes; an uneven density"""
    from tracer_amd.source_spectrum import SourceSpectrum
    if W == 2:
        wl = N.array([NODES[0], NODES[-1]])
    elif W == 3:
        wl = N.array([0.2e-6, NODES[2], 2.8e-6])
    else:
        wl = N.linspace(0.2e-6, 2.8e-6, W)
        for node in (NODES[0], NODES[2], NODES[-1]):        # the grid point next to a node moves onto it
            wl[N.abs(wl - node).argmin()] = node
    assert (wl[1:] > wl[:-1]).all()
    return SourceSpectrum.polychromatic(wl, 1.5 + N.sin(4e6 * wl), ref_index=ref_index)


def source(n, spec, seed=SEED, offset=OFFSET):
    from tracer_amd import sources
    return sources.rect_bundle(n, N.c_[[0., 0., 1.]], N.r_[0., 0., -1.], 2., 2., 0.4, flux=1000., seed=seed, ray_offset=offset, spectrum=spec)


@functools.lru_cache(maxsize=None)
def scene(kind):
    """(assembly, compiled scene) of the box: 'box', 'table' (with a surface out of the way whose optics table is beyond LDS) or
    'split' (with a slab of two faces that send two rays on, between the source and the wall)"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM, RoundPlateGM
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate
    from tracer_amd.scene import compile_scene
    asm, _ = _poly_scene()
    objs = list(asm.get_objects())
    if kind == 'table':
        lam = N.linspace(0.2e-6, 2.6e-6, split_cases.TABLE_LEN)
        objs.append(AssembledObject(surfs=[Surface(RoundPlateGM(0.5), opt.Reflective_spectral(0.2 + 0.5 * N.sin(3e6 * lam) ** 2, lam))],
                                    transform=translate(40., 40., 0.25)))
    if kind == 'split':
        face = lambda: opt.RefractiveHomogenous(1., 1.5, single_ray=False)
        objs += [AssembledObject(surfs=[Surface(RectPlateGM(3.6, 3.6), face())], transform=translate(0., 0., z)) for z in (0.8, 0.6)]
    asm = Assembly(objects=objs)
    return asm, compile_scene(asm)


_REF = {}


def reference(kind, W, n, reps):
    """the oracle's trace, computed once and shared (nobody changes it), with its hit list (split_cases.hit_list: one entry per hit,
    whatever it sent on, with the 3 W spectral columns)"""
    key = (kind, W, n, reps)
    if key not in _REF:
        from oracle import engine, sources
        cs = scene(kind)[1]
        sp = spectrum(W)
        desc, n_, seed, off = source(n, sp).source_args()
        v, d, e, rid = sources.generate(engine.source_from_desc(desc), n, seed, off)
        wl, val, _ = sp.table()
        swl = N.tile(wl[:, None], (1, n))
        spec = e * val[:, None]
        with N.errstate(all='ignore'):
            o = engine.trace_bundle(cs, v, d, e, reps, MIN_ENERGY, seed, ref_index=N.full(n, sp.ref_index), wavelengths=swl, spectra=spec, offset=off)
        c = types.SimpleNamespace(W=W, columns=lambda: dict(spec=spec))
        o['hit_list'] = split_cases.hit_list(o['levels'], c)
        o['first'] = (v, d, e, swl, spec)
        _REF[key] = o
    return _REF[key]


def _order(*keys):
    return N.lexsort([N.round(k, 7) for k in reversed(keys)])


class env(object):
    """environment knobs of the library for the duration of a block (read at every call)"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = dict((k, os.environ.get(k)) for k in self.kw)
        for k, v in self.kw.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check(ctx, kind, W, n, reps, what, chart=False, bundle=None, **knobs):
    """trace the pending carried source (or `bundle`) through DeviceScene.trace_fast and hold everything to the oracle"""
    from tracer_amd.scene import DeviceScene
    cs = scene(kind)[1]
    o = reference(kind, W, n, reps)
    captured = [i for i in range(cs.n_surf) if cs.capture[i]]
    assert 0 in captured            # the polychromatic wall
    dev = DeviceScene(cs, ctx)
    if chart:
        dev.set_fluxmap(0, *CYL_EDGES, chart='cylinder')
    dev.set_hit_capacity(o['events'] + 1024)
    b = source(n, spectrum(W)) if bundle is None else bundle
    try:
        with env(**knobs):
            st, last = dev.trace_fast(b, reps, MIN_ENERGY, SEED, keep_last=True, last_capacity=o['last_energy'].size + 64)
    except Exception:
        dev.close()
        raise
    if bundle is None:
        assert b.is_pending(), what             # never made on the way
    a, r, h = dev.get_tallies()
    hits = dev.get_hits()
    nx = dev.hit_spectral_columns()
    fm = dev.get_fluxmap(0) if chart else None
    dev.close()
    print('%s: %d segments, %d hits, %d left, %d launches; largest differences: absorbed %.3g, received %.3g of %.3g' %
          (what, st.segments, st.hits, st.rays_left, st.launches, N.abs(a - o['absorbed']).max(), N.abs(r - o['received']).max(), o['received'].max()))
    assert st.launches > 1 and st.hits_dropped == 0, what
    assert N.array_equal(h, o['hits']), (what, h, o['hits'])
    assert (st.segments, st.hits, st.rays_left) == (o['segments'], o['events'], o['last_energy'].size), what
    # (the project's tolerances for tallies, test_gpu_media.py and test_gpu_shade_instances.py: rtol 1e-9 with atol 1e-12 -- a surface
    # that absorbs nothing, a face of the slab, shows the roundings of `incident - (reflected + refracted)`, 1e-14 of either sign)
    assert N.allclose(a, o['absorbed'], rtol=1e-9, atol=1e-12), (what, a, o['absorbed'])
    assert N.allclose(r, o['received'], rtol=1e-9, atol=0.), (what, r, o['received'])
    assert N.isclose(st.energy_left, o['last_energy'].sum(), rtol=1e-9, atol=0.), what
    # survivors, as multisets, with their spectra
    assert o['last_energy'].size > 20, what            # (reps is cut so that rays survive)
    mine = N.vstack(last[:7])
    theirs = N.vstack((o['last_vertices'], o['last_directions'], o['last_energy'][None, :]))
    assert mine.shape == theirs.shape, (what, mine.shape, theirs.shape)
    km, kt = _order(*mine[:6]), _order(*theirs[:6])
    assert N.allclose(mine[:6, km], theirs[:6, kt], rtol=1e-9, atol=1e-9), (what, 'survivors')
    assert N.allclose(mine[6, km], theirs[6, kt], rtol=1e-9, atol=0.), (what, 'energies of the survivors')
    if bundle is None:          # (survivors' spectra come back for a carried source only)
        L = o['levels'][-1]
        assert len(last) == 9 and last[7].shape == (W, theirs.shape[1]), what
        assert N.allclose(last[7][:, km], L['spectra'][:, :L['n_live']][:, kt], rtol=1e-12, atol=0.), (what, 'spectra of the survivors')
        assert N.array_equal(last[8][:, km], L['swl'][:, :L['n_live']][:, kt]), what
    # captured hits, per capturing surface, matched after sorting
    H = o['hit_list']
    assert len(hits['surf']) == h[captured].sum() and nx == 3 * W, (what, nx)
    for s in captured:
        km, kt = N.nonzero(hits['surf'] == s)[0], N.nonzero(H['surf'] == s)[0]
        assert len(km) == len(kt) == h[s] and h[s] > 0, (what, s)
        km = km[_order(*N.vstack((hits['points'][:, km], hits['e_abs'][km])))]
        kt = kt[_order(*N.vstack((H['points'][:, kt], H['e_abs'][kt])))]
        assert N.allclose(hits['points'][:, km], H['points'][:, kt], rtol=1e-12, atol=1e-12), (what, s)
        assert N.allclose(hits['e_abs'][km], H['e_abs'][kt], rtol=1e-9, atol=0.), (what, s)
        if hits['directions'] is not None:          # (a full capture)
            assert N.allclose(hits['e_in'][km], H['e_in'][kt], rtol=1e-9, atol=0.), (what, s)
        got = N.vstack((hits['spectra'][2], hits['spectra'][0], hits['spectra'][1]))[:, km]        # wavelengths, arrived, left
        assert N.array_equal(got[:W], H['x'][:W, kt]), (what, s)
        assert N.allclose(got[W:], H['x'][W:, kt], rtol=1e-12, atol=0.), (what, s, N.abs(got[W:] - H['x'][W:, kt]).max())
    if chart:
        frames = [N.array(sf._temp_frame) for sf in cs.surfaces]
        Hm = fcs.host_maps(H, frames, {0: ('cylinder', False) + CYL_EDGES})[0][0]
        assert fm.shape == Hm.shape and (Hm > 0).all(), what
        assert N.allclose(fm, Hm, rtol=1e-9, atol=1e-9 * Hm.max()), (what, N.abs(fm - Hm).max())
    return dict(tallies=(a, r, h), hits=hits, stats=st)


@pytest.mark.parametrize('W', [3, 17])
def test_streaming_form_lds_route(ctx, W):
    """the box alone: tables, grid, birth vector and the wall's lambda cells in LDS (k_s_shade_p<true, false, false>)"""
    _check(ctx, 'box', W, N_RAYS, 3, 'box W=%d' % W)


def test_streaming_form_global_route(ctx):
    """an optics table beyond LDS: tables, grid and birth vector are read from global memory, every hit searches its cells"""
    _check(ctx, 'table', 17, N_RAYS, 3, 'table W=17')


def test_longest_grid_at_the_fewest_rays(ctx):
    """W = 4096 at 64 rays: 64 KiB of grid and birth vector beside the long table -- the global instance.  (The table of the spectra
    under way has W rows of as many entries as the ray table has slots, 2^24 and more by default whatever the call's size: the room
    of the lists is set to 65536 entries for this call, 2 GiB of spectra, as the tests of small lists set it.)"""
    _check(ctx, 'table', 4096, 64, 2, 'table W=4096', TRC_STREAM_ROOM=65536)


def test_split_scene(ctx):
    """a splitting slab in front of the wall: a hit is recorded once, with the sum of both rays' spectra; both survivors come back"""
    out = _check(ctx, 'split', 3, N_RAYS, 4, 'split W=3')
    assert out['stats'].rays_left > N_RAYS          # more rays left than were given


def test_chart_flux_map(ctx):
    """a cylinder-chart flux map on the wall against the host histogram of the oracle's hits"""
    _check(ctx, 'box', 3, N_RAYS, 3, 'chart W=3', chart=True)


def test_same_rays_two_routes(ctx):
    """the pending source against its own materialisation, traced as a given polychromatic bundle with seed and offset handed over"""
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.scene import DeviceScene
    W, reps = 17, 3
    pending = _check(ctx, 'box', W, N_RAYS, reps, 'pending')
    made = source(N_RAYS, spectrum(W))
    assert made.is_polychromatic() and not made.is_pending() and made.get_spectra().shape == (W, N_RAYS)
    cs = scene('box')[1]
    dev = DeviceScene(cs, ctx)
    dev.set_hit_capacity(8 * N_RAYS)
    cols = made.columns_soa()
    from tracer_amd import _cabi
    rid = N.arange(N_RAYS, dtype=N.uint64) + N.uint64(OFFSET)
    rays = _cabi.make_rays(N_RAYS, cols['x'], cols['y'], cols['z'], cols['dx'], cols['dy'], cols['dz'], cols['e'], ref_index=cols['ref_index'],
                           rid=rid, spec_wl=cols['spec_wl'], spectra=cols['spectra'])
    stats = _cabi.TraceStats()
    _cabi.check(dev.lib.trc_trace_fast_x(dev.handle, C.byref(rays), None, None, N_RAYS, reps, MIN_ENERGY, SEED, 0, _cabi.TRACE_STREAM, None,
                                         C.byref(stats)))
    a, r, h = dev.get_tallies()
    hits = dev.get_hits()
    dev.close()
    pa, pr, ph = pending['tallies']
    assert N.array_equal(h, ph) and stats.segments == pending['stats'].segments
    assert N.allclose(a, pa, rtol=1e-9, atol=0.) and N.allclose(r, pr, rtol=1e-9, atol=0.)
    P = pending['hits']
    km = _order(*N.vstack((hits['points'], hits['e_abs'])))
    kp = _order(*N.vstack((P['points'], P['e_abs'])))
    assert len(km) == len(kp)
    for x, y in zip(hits['spectra'], P['spectra']):
        assert N.allclose(x[:, km], y[:, kp], rtol=1e-12, atol=0.)


@pytest.mark.parametrize('n,tree', [(N_RAYS, True), (63, False)])
def test_ordered_engine(ctx, n, tree):
    """tree=True, and 63 rays under engine='auto': every level against the oracle; level 0 carries (W, n) columns made on the device"""
    from tracer_amd.tracer_engine import TracerEngine
    W, reps = 3, 3
    asm = scene('box')[0]
    o = reference('box', W, n, reps)
    eng = TracerEngine(asm)
    b = source(n, spectrum(W))
    eng.ray_tracer(b, reps=reps, min_energy=MIN_ENERGY, tree=tree, seed=SEED)
    assert eng.stats['engine'] == 'ordered' and b.is_pending()
    a, r, h = eng.get_tallies()
    assert N.array_equal(h, o['hits']) and eng.stats['segments'] == o['segments']
    assert N.allclose(a, o['absorbed'], rtol=1e-9, atol=0.) and N.allclose(r, o['received'], rtol=1e-9, atol=0.)
    levels = eng._ordered_pending[-1]().levels
    v, d, e, swl, spec = o['first']
    L0 = levels.level(0)
    assert L0['spectra'].shape == (W, n) and N.array_equal(L0['spectra'], spec) and N.array_equal(L0['wavelengths'], swl)
    assert N.array_equal(L0['energy'], e)
    for lv in range(1, len(o['levels'])):
        L, R = levels.level(lv), o['levels'][lv]
        assert L['n_live'] == R['n_live'] and N.array_equal(L['parents'], R['parents']) and N.array_equal(L['surf'], R['surf']), lv
        assert N.allclose(L['vertices'], R['vertices'], rtol=1e-9, atol=1e-9) and N.allclose(L['energy'], R['energy'], rtol=1e-9, atol=0.), lv
        assert N.array_equal(L['wavelengths'], R['swl']) and N.allclose(L['spectra'], R['spectra'], rtol=1e-12, atol=0.), lv


def test_source_generate_columns(ctx):
    """trc_source_generate_x under a carried spectrum: the columns are table() x energy, bit for bit"""
    for W in (2, 3, 17):
        sp = spectrum(W, ref_index=1.25)
        b = source(N_RAYS, sp)
        wl, val, _ = sp.table()
        e = b.get_energy()
        assert b.is_polychromatic() and b.get_spectra().shape == (W, N_RAYS)
        assert N.array_equal(b.get_spectra(), e * val[:, None])
        assert N.array_equal(b.get_wavelengths(), N.tile(wl[:, None], (1, N_RAYS)))
        assert N.array_equal(b.get_ref_index(), N.full(N_RAYS, 1.25))
        assert N.allclose(N.trapezoid(b.get_spectra(), b.get_wavelengths(), axis=0), e, rtol=1e-12)
        # the same rays as without a spectrum
        plain = source(N_RAYS, None)
        assert N.array_equal(plain.get_vertices(), b.get_vertices()) and N.array_equal(plain.get_energy(), e)


def test_refusals(ctx):
    from tracer_amd import _cabi
    from tracer_amd.scene import DeviceScene, compile_scene
    import shade_cases
    cs = scene('box')[1]
    dev = DeviceScene(cs, ctx)
    sp = spectrum(3)
    # the megakernel, and fewer than 64 rays: unsupported, naming the ordered engine
    for n, stream in ((N_RAYS, False), (63, None)):
        with pytest.raises(_cabi.TracerAmdError) as err:
            dev.trace_fast(source(n, sp), 3, MIN_ENERGY, SEED, stream=stream)
        assert err.value.status == _cabi.ERR_UNSUPPORTED and 'trc_trace_ordered' in str(err.value)
    # a given bundle with a spectrum
    made = source(64, None)
    cols = made.columns_soa()
    rays = _cabi.make_rays(64, cols['x'], cols['y'], cols['z'], cols['dx'], cols['dy'], cols['dz'], cols['e'])
    stats = _cabi.TraceStats()
    st = dev.lib.trc_trace_fast_x(dev.handle, C.byref(rays), None, C.byref(sp.desc()), 64, 3, MIN_ENERGY, SEED, 0, 0, None, C.byref(stats))
    assert st == _cabi.ERR_INVALID
    dev.close()
    # a scene between tabulated materials
    asm, T = shade_cases.room('carry-mat')
    dev = DeviceScene(compile_scene(asm), ctx)
    desc, n, seed, off = source(N_RAYS, sp).source_args()
    for fn, extra in ((dev.lib.trc_trace_fast_x, (None,)), (dev.lib.trc_trace_ordered_x, (C.byref(C.c_void_p()),))):
        st = fn(dev.handle, None, C.byref(desc), C.byref(sp.desc()), n, 3, MIN_ENERGY, seed, off, 0, *(extra + (C.byref(stats),)))
        assert st == _cabi.ERR_UNSUPPORTED
    dev.close()
    # room for another number of samples than the spectrum has
    c = _cabi.get_context()
    n = 64
    cols = [N.empty(n) for _ in range(7)]
    wl, spec = N.empty((4, n)), N.empty((4, n))
    out = _cabi.make_rays(n, *cols, spec_wl=wl, spectra=spec)
    st = c.lib.trc_source_generate_x(c.handle, C.byref(desc), C.byref(sp.desc()), n, seed, off, C.byref(out))
    assert st == _cabi.ERR_INVALID
    out = _cabi.make_rays(n, *cols)
    st = c.lib.trc_source_generate_x(c.handle, C.byref(desc), C.byref(sp.desc()), n, seed, off, C.byref(out))
    assert st == _cabi.ERR_INVALID


def test_tracer_engine_end_to_end(ctx):
    """engine='auto': the fast engine's streaming form for tree=False, the bundle still pending afterwards, the returned bundle with
    spectra; the wall's PolychromaticAccountant holds the hits of an ordered trace, hit by hit"""
    from tracer_amd.tracer_engine import TracerEngine
    W, reps = 17, 3
    o = reference('box', W, N_RAYS, reps)
    got = []
    for engine in ('auto', 'ordered'):
        asm, _ = _poly_scene()
        eng = TracerEngine(asm)
        b = source(N_RAYS, spectrum(W))
        eng.ray_tracer(b, reps=reps, min_energy=MIN_ENERGY, tree=False, seed=SEED, engine=engine)
        assert b.is_pending()
        if engine == 'auto':
            assert eng.stats['engine'] == 'fast' and eng.stats['form'] == 'stream'
            last = eng.tree[-1]
            assert last.is_polychromatic() and last.get_spectra().shape == (W, o['last_energy'].size)
            assert N.allclose(N.sort(N.trapezoid(last.get_spectra(), last.get_wavelengths(), axis=0)), N.sort(last.get_energy()), rtol=1e-9)
        else:
            assert eng.stats['engine'] == 'ordered'
        e, (w, s) = asm.get_surfaces()[0].get_optics_manager().get_all_hits()[:2]
        assert len(e) == o['hits'][0] and s.shape == (W, len(e))
        k = N.lexsort((s[1], s[0], e))
        got.append((e[k], w[:, k], s[:, k]))
    (e1, w1, s1), (e2, w2, s2) = got
    assert N.allclose(e1, e2, rtol=1e-9, atol=0.) and N.array_equal(w1, w2)
    assert N.allclose(s1, s2, rtol=1e-9, atol=1e-12 * N.abs(s2).max())
    # engine='protocol' makes the bundle
    b = source(N_RAYS, spectrum(3))
    eng = TracerEngine(_poly_scene()[0])
    eng.ray_tracer(b, reps=1, min_energy=MIN_ENERGY, tree=True, engine='protocol')
    assert not b.is_pending() and b.is_polychromatic()
