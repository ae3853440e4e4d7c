"""
GPU tests of the flux maps binned in cylinder, polar and sphere coordinates (trc_scene_set_fluxmap_chart), run with -m gpu on the
MI355X box.

As in test_gpu_fluxmap.py every map is compared with an independent reference, never with another device form: the hits captured
on the mapped surfaces (the buffer holds all of them: nothing dropped) are read back, projected on the host with the same
round(inv(frame), 9), taken to the chart's coordinates by the NumPy formulas of the reference's get_fluxmap bodies
(fluxmap_chart_scene.chart_uv) and binned by numpy.histogram2d with the absorbed energies as weights.  Map and histogram differ by
the order of float64 sums only (rtol 1e-9, atol 1e-9 of the largest bin) -- as long as no hit lies within 1e-12 of a map's span
from an edge, where the last bit of atan2 / acos would decide the bin: check_inputs says so if a seed ever gives such a hit.

The scene (fluxmap_chart_scene.py) holds every chart, a chart map on a surface of every shading class and on one that ends every
ray, a plain XY map in front of them, a map with x and y exchanged, a frustum on edges of the caller's, a clipped map and
full-azimuth maps whose seam bins are populated; it reaches record_hit's chart instances in the megakernel, in k_s_shade, in the lean
shading kernels of both classes and in the spectral k_s_shade_x, and the ordered engine's own copy.
"""
import os

import numpy as N
import pytest

import fluxmap_chart_scene as fc

pytestmark = pytest.mark.gpu

REPS, EMIN = 12, 1e-10

# form: (engine, stream, accel, environment knobs)
FORMS = {'megakernel': ('fast', False, True, {}),
         'stream': ('fast', True, True, {}),
         'stream-absorb-list': ('fast', True, True, {'TRC_STREAM_ABSORB': 1}),  # (a scene with a chart map keeps its terminal hits in the shading kernels)
         'stream-no-accel': ('fast', True, False, {}),
         'ordered': ('ordered', None, False, {})}


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


@pytest.fixture(scope='module')
def receivers():
    from tracer_amd.scene import compile_scene
    asm, objs, T = fc.receivers()
    cs = compile_scene(asm)
    return cs, T, [N.array(s._temp_frame) for s in cs.surfaces]


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


def _device(ctx, cs, maps, capacity):
    from tracer_amd.scene import DeviceScene
    dev = DeviceScene(cs, ctx)
    for s in sorted(maps):
        chart, swap, ue, ve = maps[s]
        proj = fc.projection(cs.surfaces[s]._temp_frame, True) if swap else None     # (None: the library's own default)
        dev.set_fluxmap(s, ue, ve, proj=proj, chart=chart)
    if capacity:
        dev.set_hit_capacity(capacity)
    return dev


def _capacity(n):
    return 2 * n + 65536


def _given(bundle):
    """the rays of a source bundle handed over as a plain RayBundle"""
    from tracer_amd.ray_bundle import RayBundle
    return RayBundle(vertices=N.array(bundle.get_vertices()), directions=N.array(bundle.get_directions()),
                     energy=N.array(bundle.get_energy()))


def _trace(dev, bundle, form, seed):
    """one call; returns (the hit list of this call for the host reference, stats)"""
    engine, stream, accel, knobs = FORMS[form]
    with env(**knobs):
        if engine == 'ordered':
            res, st = dev.trace_ordered(bundle, REPS, EMIN, seed, accel=False)
            levels = [dict(energy=N.asarray(bundle.get_energy()))] + [res.level(k) for k in range(1, res.num_levels())]
            res.close()
            return fc.fs.hits_of_levels(levels), st
        st, _ = dev.trace_fast(bundle, REPS, EMIN, seed, accel=accel, stream=stream)
    assert st.hits_dropped == 0
    return None, st


def _check(dev, ref, what):
    """every map against its host histogram, the energy outside against the surface's absorbed energy"""
    a, _, h = dev.get_tallies()
    for s, (H, e_out, n_out, n_hits, n_near) in ref.items():
        got = dev.get_fluxmap(s)
        assert got.shape == H.shape and n_hits == h[s], (what, s, n_hits, h[s])       # (the hit list holds every hit the surface counted)
        tol = 1e-9 * H.max()
        print('%s surface %d: %d x %d, %d hits, %d outside, largest difference %.3g of %.3g' %
              (what, s, H.shape[0], H.shape[1], n_hits, n_out, N.abs(got - H).max(), H.max()))
        assert N.allclose(got, H, rtol=1e-9, atol=tol), (what, s, N.abs(got - H).max(), H.max())
        assert N.isclose(a[s] - got.sum(), e_out, rtol=1e-9, atol=tol), (what, s, a[s] - got.sum(), e_out)


def _captured(dev, frames, maps):
    hits = dev.get_hits()
    h = dev.get_tallies()[2]
    captured = [i for i in range(dev.n_surf) if dev.compiled.capture[i]]
    assert len(hits['surf']) == h[captured].sum()
    return fc.host_maps(hits, frames, maps)


@pytest.mark.parametrize('given', [False, True], ids=['source', 'given-bundle'])
@pytest.mark.parametrize('regime', sorted(fc.FLOOR_BINS))
@pytest.mark.parametrize('form', sorted(FORMS))
def test_chart_maps_equal_the_host_histogram_of_the_hits(ctx, receivers, form, regime, given):
    """2e5 rays (one batch) from the disc source -- fresh rays through the footprint map -- or the same rays as a given bundle --
    through the general queue path -- by every form, with the bins in LDS and on global atomics."""
    cs, T, frames = receivers
    n, seed = 200000, 11
    maps = fc.maps(regime)
    bundle = fc.source(n, T, seed)
    if given:
        bundle = _given(bundle)
    dev = _device(ctx, cs, maps, 0 if form == 'ordered' else _capacity(n))
    hits, st = _trace(dev, bundle, form, seed)
    ref = fc.host_maps(hits, frames, maps) if hits is not None else _captured(dev, frames, maps)
    fc.check_inputs(ref, maps)
    assert st.segments > 1.2 * n and sum(r[3] for r in ref.values()) > 0.8 * n
    _check(dev, ref, (form, regime, given))
    dev.close()


@pytest.mark.parametrize('kind', ['source-spectrum', 'polychromatic'])
def test_chart_maps_of_the_spectral_paths(ctx, receivers, kind):
    """A source with a spectrum -- the SPEC shading instances -- and a polychromatic given bundle -- k_s_shade_x, which serves every
    hit when rays carry spectra -- against the same host histogram, the bins in LDS."""
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.source_spectrum import SourceSpectrum
    cs, T, frames = receivers
    maps = fc.maps('lds')
    n, seed = 200000, 41
    if kind == 'source-spectrum':
        wl = N.linspace(0.3e-6, 2.5e-6, 23)
        bundle = fc.source(n, T, seed, spectrum=SourceSpectrum.tabulated(wl, 1. + N.sin(4e6 * wl) ** 2))
    else:
        b = fc.source(n, T, seed)
        W = 5
        rng = N.random.RandomState(6)
        swl = N.sort(rng.uniform(0.3e-6, 2.5e-6, size=(W, n)), axis=0)
        spec = rng.uniform(0.5, 2., size=(W, n))
        spec *= N.asarray(b.get_energy()) / N.trapezoid(spec, swl, axis=0)
        bundle = RayBundle(vertices=N.array(b.get_vertices()), directions=N.array(b.get_directions()),
                           energy=N.trapezoid(spec, swl, axis=0), spectra=spec, wavelengths=swl)
    dev = _device(ctx, cs, maps, _capacity(n))
    _, st = _trace(dev, bundle, 'stream', seed)
    ref = _captured(dev, frames, maps)
    fc.check_inputs(ref, maps)
    assert st.segments > 1.2 * n
    _check(dev, ref, kind)
    dev.close()


@pytest.mark.parametrize('chart', ['cylinder', 'polar', 'sphere'])
@pytest.mark.parametrize('form', ['megakernel', 'stream', 'ordered'])
def test_hits_exactly_on_chart_edges(ctx, form, chart):
    """Rays fired straight down on an axis-aligned plate land exactly where the chart's coordinates are exact on any library: u on
    interior, first and last edges and one ulp either side of them, phi = 0 and the seam, theta = 0 at the pole
    (fluxmap_chart_scene.edge_cases: the expected map is written out by hand from numpy's rule).  Equality is exact."""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd import optics_callables as opt
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.scene import compile_scene, DeviceScene
    x, y, e, want, outside = fc.edge_cases(chart)
    cs = compile_scene(Assembly(objects=[AssembledObject(surfs=[Surface(RectPlateGM(64., 64.), opt.LambertianReceiver(1.))])]))
    assert N.array_equal(fc.projection(cs.surfaces[0]._temp_frame), N.eye(4))
    k = len(x)
    # (64 rays more that pass beside the plate: from 64 rays on a forced streaming call is one -- below, the megakernel serves it)
    miss = 64
    vx, vy = N.r_[x, 100. + N.arange(miss)], N.r_[y, N.zeros(miss)]
    bundle = RayBundle(vertices=N.vstack((vx, vy, N.ones(k + miss))), directions=N.vstack((N.zeros(k + miss), N.zeros(k + miss), -N.ones(k + miss))),
                       energy=N.r_[e, N.ones(miss)])
    dev = DeviceScene(cs, ctx)
    dev.set_fluxmap(0, *fc.EDGE_EDGES[chart], proj=fc.EDGE_PROJ[chart], chart=chart)
    if form != 'ordered':
        dev.set_hit_capacity(4096)
    hits, st = _trace(dev, bundle, form, 3)
    a, r, h = dev.get_tallies()
    got = dev.get_fluxmap(0)
    assert h[0] == k and a[0] == e.sum()
    if hits is None:
        hits = dev.get_hits()
    assert sorted(zip(hits['points'][0], hits['points'][1])) == sorted(zip(x, y))         # every ray landed where it was aimed
    assert not N.asarray(hits['points'][2]).any()
    assert N.array_equal(got, want), (form, chart, N.argwhere(got != want))
    assert a[0] - got.sum() == outside
    dev.close()


def test_engine_maps_of_the_surfaces_own_shapes(ctx):
    """TracerEngine.set_surface_fluxmap for the cylinder, the dish, the sphere and the round plate, then ray_tracer(tree=False):
    get_surface_flux is that geometry's get_fluxmap of the hits its accountants hold, taken through global_to_local (rtol 1e-9:
    the order of sums; no hit within 1e-12 of an edge)."""
    from tracer_amd.tracer_engine import TracerEngine
    asm, objs, T = fc.receivers()
    surfs = asm.get_surfaces()
    eng = TracerEngine(asm)
    resolution = {fc.CYLINDER: 9, fc.DISH: 7, fc.SPHERE: 5, fc.FLOOR: None}        # (None: the round plate's default of 40)
    for s in sorted(resolution):
        eng.set_surface_fluxmap(surfs[s], resolution[s])
    n = 200000
    eng.ray_tracer(fc.source(n, T, 61), REPS, EMIN, tree=False, seed=61)
    for s in sorted(resolution):
        e_abs, pts = surfs[s].get_optics_manager().get_all_hits()[:2]
        local = surfs[s].global_to_local(pts)
        gm = surfs[s].get_geometry_manager()
        chart, swap, ue, ve, areas = gm.fluxmap_grid(resolution[s])
        u, v = fc.chart_uv(chart, N.eye(4)[[1, 0, 2, 3]] if swap else N.eye(4), local[:3])
        assert not (fc.near_edge(u, ue) | fc.near_edge(v, ve)).any(), 'INPUT CONDITION, not the map: a hit of surface %d within 1e-12 of an edge' % s
        want = gm.get_fluxmap(N.array(e_abs), N.array(local), resolution[s])
        got = eng.get_surface_flux(surfs[s])
        print('surface %d: %d hits, %d bins, %.0f %% filled' % (s, len(e_abs), want.size, 100. * (want > 0).mean()))
        assert len(e_abs) > 0.01 * n and got.shape == want.shape and (want > 0).mean() >= 0.10
        assert N.allclose(got, want, rtol=1e-9, atol=1e-9 * want.max()), (s, N.abs(got - want).max(), want.max())
    with pytest.raises(NotImplementedError):
        eng.set_surface_fluxmap(surfs[fc.FRUSTUM], 5)


def _call(dev, receivers, maps, n, seed, form='stream'):
    """one more call on `dev`; the host maps of that call's hits alone (the hit buffer is emptied first)"""
    cs, T, frames = receivers
    dev.set_hit_capacity(_capacity(n))
    dev.lib.trc_scene_clear_hits(dev.handle)
    _trace(dev, fc.source(n, T, seed), form, seed)
    return fc.host_maps(dev.get_hits(), frames, maps)


def test_chart_bins_accumulate_reset_and_travel(ctx, receivers):
    """Two calls -- the streaming form, then the megakernel -- accumulate to the sum of the two host histograms; export_tallies /
    import_tallies carries all six maps to another scene; reset_tallies zeroes every one, and the next call starts from zero."""
    cs, T, frames = receivers
    maps = fc.maps('lds')
    n = 200000
    dev = _device(ctx, cs, maps, _capacity(n))
    r1 = _call(dev, receivers, maps, n, 21, 'stream')
    _check(dev, r1, 'first call')
    r2 = _call(dev, receivers, maps, n, 22, 'megakernel')
    both = dict((s, tuple(r1[s][k] + r2[s][k] for k in range(5))) for s in r1)
    fc.check_inputs(both, maps)
    _check(dev, both, 'two calls')
    assert all(both[s][0].sum() > 1.5 * r1[s][0].sum() for s in both)
    other = _device(ctx, cs, maps, 0)
    other.import_tallies(dev.export_tallies())
    for s in maps:
        assert N.array_equal(other.get_fluxmap(s), dev.get_fluxmap(s)), s
    assert all(N.array_equal(x, y) for x, y in zip(other.get_tallies(), dev.get_tallies()))
    other.close()
    dev.reset_tallies()
    for s in maps:
        assert not dev.get_fluxmap(s).any(), s
    r3 = _call(dev, receivers, maps, n, 23, 'stream')
    _check(dev, r3, 'after the reset')
    dev.close()


def test_unknown_charts_and_second_maps_are_refused(ctx, receivers):
    from tracer_amd import _cabi
    from tracer_amd.scene import DeviceScene
    cs, T, frames = receivers
    dev = DeviceScene(cs, ctx)
    u, v = N.linspace(0., 1., 4), N.linspace(0., 6., 6)
    for bad in (4, -1, 17):
        with pytest.raises(_cabi.TracerAmdError, match='unknown chart'):
            dev.set_fluxmap(fc.CYLINDER, u, v, chart=bad)
    with pytest.raises(ValueError, match='unknown flux-map chart'):
        dev.set_fluxmap(fc.CYLINDER, u, v, chart='conical')
    assert fc.CYLINDER not in dev.fluxmaps
    dev.set_fluxmap(fc.CYLINDER, u, v, chart='cylinder')
    dev.set_fluxmap(fc.WALL, u, v)
    # one map per surface, whichever entry point set it and whichever asks again
    for s, kw in ((fc.CYLINDER, {}), (fc.CYLINDER, {'chart': 'polar'}), (fc.WALL, {'chart': 'sphere'}), (fc.WALL, {})):
        with pytest.raises(_cabi.TracerAmdError, match='surface %d already has a flux map' % s):
            dev.set_fluxmap(s, N.linspace(-1., 1., 3), N.linspace(-1., 1., 5), **kw)
    p = _cabi.f64(N.eye(4)[:3].ravel())
    uu, vv = _cabi.f64(u), _cabi.f64(v)
    rc = dev.lib.trc_scene_set_fluxmap(dev.handle, fc.CYLINDER, 3, 5, _cabi.ptr(uu), _cabi.ptr(vv), _cabi.ptr(p))
    assert rc == _cabi.ERR_INVALID
    assert dev.get_fluxmap(fc.CYLINDER).shape == (3, 5) and dev.get_fluxmap(fc.WALL).shape == (3, 5)
    dev.close()
