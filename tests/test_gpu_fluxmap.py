"""
GPU tests of the flux maps (trc_scene_set_fluxmap / trc_scene_get_fluxmap), run with -m gpu on the MI355X box.

Every map is compared with the same independent reference, never with another device form: the hits captured on the mapped
surfaces (the buffer holds all of them: nothing dropped) are read back, projected on the host with the same round(inv(frame), 9)
and binned by numpy.histogram2d with the absorbed energies as weights.  Map and histogram differ by the order of float64 sums
only (rtol 1e-9, atol 1e-9 of the largest bin); the energy of the hits outside a map is what the surface absorbed less the map.

The scene (fluxmap_scene.py) reaches every site that bins: record_hit in the megakernel and in the streaming engine's shading
kernels of all three classes, k_s_absorb's and k_s_bounce's finish of terminal hits, the spectral k_s_shade_x and the ordered
engine's own copy -- with five maps of different shapes at once, so that every map but the first sits at an offset in the
tally buffer and in its LDS copy, and in the three storage regimes of the bins (fluxmap_scene.FLOOR_BINS has the arithmetic).
"""
import os

import numpy as N
import pytest

import fluxmap_scene as fs

pytestmark = pytest.mark.gpu

REPS, EMIN = 12, 1e-10

# form: (engine, stream, accel, environment knobs)
FORMS = {'megakernel': ('fast', False, True, {}),
         'stream': ('fast', True, True, {}),                                    # terminal hits finished inside k_s_bounce
         'stream-absorb-list': ('fast', True, True, {'TRC_STREAM_ABSORB': 1}),  # ... behind a list, by k_s_absorb
         'stream-no-accel': ('fast', True, False, {}),
         'ordered': ('ordered', None, False, {})}


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


@pytest.fixture(scope='module')
def cavity():
    from tracer_amd.scene import compile_scene
    asm, objs, T = fs.cavity()
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


def _device(ctx, cs, edges, capacity):
    from tracer_amd.scene import DeviceScene
    dev = DeviceScene(cs, ctx)
    for s in sorted(edges):
        dev.set_fluxmap(s, *edges[s])
    if capacity:
        dev.set_hit_capacity(capacity)
    return dev


def _capacity(n):
    return 2 * n + 65536        # (1.1 captured hits per ray in this cavity)


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
            return fs.hits_of_levels(levels), st
        st, _ = dev.trace_fast(bundle, REPS, EMIN, seed, accel=accel, stream=stream)
    assert st.hits_dropped == 0
    return None, st


def _check(dev, ref, edges, what):
    """every map against its host histogram, the energy outside against the surface's absorbed energy"""
    a, _, h = dev.get_tallies()
    for s, (H, e_out, n_out, n_hits) in ref.items():
        got = dev.get_fluxmap(s)
        assert got.shape == H.shape and n_hits == h[s], (what, s, n_hits, h[s])       # (the hit list holds every hit the surface counted)
        tol = 1e-9 * H.max()
        print('%s surface %d: %d x %d, %d hits, %d outside, largest difference %.3g of %.3g' %
              (what, s, H.shape[0], H.shape[1], n_hits, n_out, N.abs(got - H).max(), H.max()))
        assert N.allclose(got, H, rtol=1e-9, atol=tol), (what, s, N.abs(got - H).max(), H.max())
        assert N.isclose(a[s] - got.sum(), e_out, rtol=1e-9, atol=tol), (what, s, a[s] - got.sum(), e_out)


def _captured(dev, cs_frames, edges):
    hits = dev.get_hits()
    h = dev.get_tallies()[2]
    captured = [i for i in range(dev.n_surf) if dev.compiled.capture[i]]
    assert len(hits['surf']) == h[captured].sum()
    return fs.host_maps(hits, cs_frames, edges)


@pytest.mark.parametrize('given', [False, True], ids=['source', 'given-bundle'])
@pytest.mark.parametrize('regime', ['small', 'middle', 'large'])
@pytest.mark.parametrize('form', sorted(FORMS))
def test_maps_equal_the_host_histogram_of_the_hits(ctx, cavity, form, regime, given):
    """2e5 rays (one batch) from the pillbox disc source -- fresh rays through the footprint map -- or the same rays as a given
    bundle -- through the general queue path -- by every form, with the bins in every storage regime."""
    cs, T, frames = cavity
    n, seed = 200000, 11
    edges = fs.map_edges(regime)
    bundle = fs.source(n, T, seed)
    if given:
        bundle = _given(bundle)
    dev = _device(ctx, cs, edges, 0 if form == 'ordered' else _capacity(n))
    hits, st = _trace(dev, bundle, form, seed)
    ref = fs.host_maps(hits, frames, edges) if hits is not None else _captured(dev, frames, edges)
    fs.check_inputs(ref, edges)
    assert st.segments > 1.5 * n and sum(r[3] for r in ref.values()) > n
    _check(dev, ref, edges, (form, regime, given))
    dev.close()


def test_k_s_absorb_runs_in_the_small_regime_only(ctx, cavity):
    """What the library reports of the regimes: its launches.  With TRC_STREAM_ABSORB=1 the terminal hits are listed and k_s_absorb
    is launched to finish them, one launch more per bounce than with TRC_STREAM_ABSORB=0 -- as long as the bins are in LDS for
    every kernel.  In the middle regime the knob changes nothing: k_s_absorb is switched off there (fm_ok, trc_stream_form_absorb)."""
    cs, T, frames = cavity
    n, seed = 200000, 11
    launches = {}
    for regime in ('small', 'middle'):
        for knob in (0, 1):
            dev = _device(ctx, cs, fs.map_edges(regime), _capacity(n))
            with env(TRC_STREAM_ABSORB=knob):
                st, _ = dev.trace_fast(fs.source(n, T, seed), REPS, EMIN, seed, accel=True, stream=True)
            launches[regime, knob] = st.launches
            dev.close()
    print('launches', launches)
    assert launches['small', 1] > launches['small', 0]
    assert launches['middle', 1] == launches['middle', 0]


@pytest.mark.parametrize('regime', ['small', 'middle', 'large'])
def test_maps_of_two_batches_in_flight(ctx, cavity, regime):
    """2e7 rays: calls of 2^23 rays and more are split into batches, two in flight on two streams, which flush their private bins
    into the same maps (below that a call is one batch: the 2e5 rays of the other tests).  Every batch launches its own kernels, so
    the call reports about twice the launches of a one-batch call on the same maps.  All five maps, all 2.2e7 hits (1.5 GB of hit
    buffer)."""
    cs, T, frames = cavity
    n, seed = 20000000, 12
    edges = fs.map_edges(regime)
    one = _device(ctx, cs, edges, _capacity(200000))
    _, st1 = _trace(one, fs.source(200000, T, seed), 'stream', seed)
    one.close()
    dev = _device(ctx, cs, edges, _capacity(n))
    _, st = _trace(dev, fs.source(n, T, seed), 'stream', seed)
    ref = _captured(dev, frames, edges)
    fs.check_inputs(ref, edges)
    print('launches: %d in one batch, %d at 2e7; segments %d' % (st1.launches, st.launches, st.segments))
    assert st.segments > 1.5 * n and st.launches > 1.5 * st1.launches
    _check(dev, ref, edges, ('2e7', regime))
    dev.close()


@pytest.mark.parametrize('form', ['megakernel', 'stream', 'ordered'])
def test_hits_exactly_on_edges(ctx, form):
    """Rays fired straight down on an axis-aligned plate land exactly on interior edges, on the first and last edges, one ulp
    either side of them and on corners of bins (fluxmap_scene.edge_cases: the expected map is written out by hand from
    numpy's rule).  Powers of two throughout: equality is exact."""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd import optics_callables as opt
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.scene import compile_scene
    x, y, e, want, outside = fs.edge_cases()
    cs = compile_scene(Assembly(objects=[AssembledObject(surfs=[Surface(RectPlateGM(16., 16.), opt.LambertianReceiver(1.))])]))
    assert N.array_equal(fs.projection(cs.surfaces[0]._temp_frame), N.eye(4))
    k = len(x)
    bundle = RayBundle(vertices=N.vstack((x, y, N.ones(k))), directions=N.vstack((N.zeros(k), N.zeros(k), -N.ones(k))), energy=e.copy())
    dev = _device(ctx, cs, {0: (fs.EDGE_U, fs.EDGE_V)}, 0 if form == 'ordered' else 4096)
    hits, st = _trace(dev, bundle, form, 3)
    a, r, h = dev.get_tallies()
    got = dev.get_fluxmap(0)
    assert h[0] == k and a[0] == e.sum()
    if hits is None:
        hits = dev.get_hits()
    assert sorted(zip(hits['points'][0], hits['points'][1])) == sorted(zip(x, y))         # every ray landed where it was aimed
    assert N.array_equal(got, want), (form, N.argwhere(got != want))
    assert a[0] - got.sum() == outside
    dev.close()


def _call(dev, cavity, edges, n, seed, form='stream'):
    """one more call on `dev`; the host maps of that call's hits alone (the hit buffer is emptied first)"""
    cs, T, frames = cavity
    dev.set_hit_capacity(_capacity(n))
    dev.lib.trc_scene_clear_hits(dev.handle)
    _trace(dev, fs.source(n, T, seed), form, seed)
    hits = dev.get_hits()
    return fs.host_maps(hits, frames, edges)


def _sum_refs(r1, r2):
    return dict((s, (r1[s][0] + r2[s][0], r1[s][1] + r2[s][1], r1[s][2] + r2[s][2], r1[s][3] + r2[s][3])) for s in r1)


@pytest.mark.parametrize('regime', ['small', 'middle'])
def test_bins_accumulate_reset_and_travel(ctx, cavity, regime):
    """Two calls -- the streaming form, then the megakernel -- accumulate to the sum of the two host histograms; export_tallies /
    import_tallies carries all five maps to another scene; reset_tallies zeroes every one, and the next call starts from zero."""
    cs, T, frames = cavity
    edges = fs.map_edges(regime)
    n = 200000
    dev = _device(ctx, cs, edges, _capacity(n))
    r1 = _call(dev, cavity, edges, n, 21, 'stream')
    _check(dev, r1, edges, 'first call')
    r2 = _call(dev, cavity, edges, n, 22, 'megakernel')
    both = _sum_refs(r1, r2)
    fs.check_inputs(both, edges)
    _check(dev, both, edges, 'two calls')
    assert all(both[s][0].sum() > 1.5 * r1[s][0].sum() for s in both)
    # another scene takes the tallies over: every map arrives, at its own place
    other = _device(ctx, cs, edges, 0)
    other.import_tallies(dev.export_tallies())
    for s in edges:
        assert N.array_equal(other.get_fluxmap(s), dev.get_fluxmap(s)), s
    assert all(N.array_equal(x, y) for x, y in zip(other.get_tallies(), dev.get_tallies()))
    _check(other, both, edges, 'imported')
    other.close()
    dev.reset_tallies()
    for s in edges:
        assert not dev.get_fluxmap(s).any(), s
    r3 = _call(dev, cavity, edges, n, 23, 'stream')
    _check(dev, r3, edges, 'after the reset')
    dev.close()


def test_maps_survive_update_frames_of_another_surface(ctx, cavity):
    """The tilted mirror turns (trc_scene_update_frames); the receivers do not move, and their maps are right for the next call:
    that call's own host histogram, which differs from the first one's (the mirror sends its rays elsewhere)."""
    from tracer_amd.scene import compile_scene
    cs, T, frames = cavity
    edges = fs.map_edges('small')
    n = 200000
    dev = _device(ctx, cs, edges, _capacity(n))
    r1 = _call(dev, cavity, edges, n, 31)
    _check(dev, r1, edges, 'before the update')
    cs2 = compile_scene(fs.cavity(mirror_turn=0.4)[0])
    frames2 = [N.array(s._temp_frame) for s in cs2.surfaces]
    assert all(N.array_equal(frames[s], frames2[s]) for s in edges) and not N.array_equal(frames[fs.MOVING], frames2[fs.MOVING])
    dev.update_frames(cs2)
    dev.reset_tallies()
    r2 = _call(dev, (cs2, T, frames2), edges, n, 31)
    fs.check_inputs(r2, edges)
    _check(dev, r2, edges, 'after the update')
    assert any(not N.array_equal(r1[s][0], r2[s][0]) for s in edges)
    dev.close()


def test_second_map_on_a_surface_is_refused(ctx, cavity):
    from tracer_amd import _cabi
    cs, T, frames = cavity
    edges = fs.map_edges('small')
    dev = _device(ctx, cs, edges, 0)
    with pytest.raises(_cabi.TracerAmdError, match='surface 2 already has a flux map'):
        dev.set_fluxmap(2, N.linspace(-1., 1., 4), N.linspace(-1., 1., 6))
    assert dev.get_fluxmap(2).shape == (14, 19)
    dev.close()


@pytest.mark.parametrize('kind', ['source-spectrum', 'polychromatic'])
@pytest.mark.parametrize('regime', ['small', 'middle'])
def test_maps_of_the_spectral_paths(ctx, cavity, kind, regime):
    """A source with a spectrum -- the shading instances that draw each ray's wavelength at its first hit -- and a polychromatic
    given bundle -- k_s_shade_x, which serves every hit when rays carry spectra -- against the same host histogram."""
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.source_spectrum import SourceSpectrum
    cs, T, frames = cavity
    edges = fs.map_edges(regime)
    n, seed = 200000, 41
    if kind == 'source-spectrum':
        wl = N.linspace(0.3e-6, 2.5e-6, 23)
        bundle = fs.source(n, T, seed, spectrum=SourceSpectrum.tabulated(wl, 1. + N.sin(4e6 * wl) ** 2))
    else:
        b = fs.source(n, T, seed)
        W = 5
        rng = N.random.RandomState(6)
        swl = N.sort(rng.uniform(0.3e-6, 2.5e-6, size=(W, n)), axis=0)
        spec = rng.uniform(0.5, 2., size=(W, n))
        spec *= N.asarray(b.get_energy()) / N.trapezoid(spec, swl, axis=0)
        bundle = RayBundle(vertices=N.array(b.get_vertices()), directions=N.array(b.get_directions()),
                           energy=N.trapezoid(spec, swl, axis=0), spectra=spec, wavelengths=swl)
    dev = _device(ctx, cs, edges, _capacity(n))
    _, st = _trace(dev, bundle, 'stream', seed)
    ref = _captured(dev, frames, edges)
    fs.check_inputs(ref, edges)
    assert st.segments > 1.5 * n
    _check(dev, ref, edges, (kind, regime))
    dev.close()


# -- five plates: the LDS image of every kernel that finishes hits, where its rounding shows -----------------------------------------
# form: (general class present, the rays carry spectra, environment knobs) -> the kernel whose image the form is there for
PLATES_FORMS = {'inline': (False, False, {}),                                  # k_s_bounce finishes the floor's hits itself
                'absorb-list': (False, False, {'TRC_STREAM_ABSORB': 1}),       # k_s_absorb
                'lean': (False, False, {'TRC_STREAM_ABSORB': 0}),              # k_s_shade_c of both classes, the floor's hits too
                'general': (True, False, {'TRC_STREAM_ABSORB': 0}),            # ... and k_s_shade
                'carried': (False, True, {})}                                  # k_s_shade_x


@pytest.fixture(scope='module')
def plates(ctx):
    """per scene (without / with the general class): compiled scene, frames, the 20 000 rays, and the megakernel's tallies of them"""
    from tracer_amd.scene import compile_scene
    out = {}
    for general in (False, True):
        asm, T = fs.plates(general)
        cs = compile_scene(asm)
        assert cs.n_surf == 5 and len(cs.extra) > 0
        rays = _given(fs.source(20000, T, 51))
        mega = _device(ctx, cs, fs.PLATES_EDGES, _capacity(20000))
        st, _ = mega.trace_fast(rays, 3, EMIN, 51, accel=True, stream=False)
        out[general] = (cs, [N.array(s._temp_frame) for s in cs.surfaces], rays, [N.array(x) for x in mega.get_tallies()])
        mega.close()
    return out


@pytest.mark.parametrize('form', sorted(PLATES_FORMS))
def test_five_plates_two_maps_and_an_optics_table(ctx, plates, form):
    """An odd surface count, two maps of different bin counts, a table-driven diffuse wall and a floor that ends every ray; 20 000
    rays, 3 bounces, through every kernel that stages the image (PLATES_FORMS): the device maps against the host histogram of the
    captured hits, the tallies against the megakernel's of the same rays (no optics of the scene reads a wavelength: rays that
    carry spectra lose the same shares)."""
    from tracer_amd.ray_bundle import RayBundle
    general, carried, knobs = PLATES_FORMS[form]
    cs, frames, rays, (a0, r0, h0) = plates[general]
    bundle = rays
    if carried:
        n, W = 20000, 3
        rng = N.random.RandomState(8)
        swl = N.sort(rng.uniform(0.3e-6, 2.5e-6, size=(W, n)), axis=0)
        spec = rng.uniform(0.5, 2., size=(W, n))
        spec *= N.asarray(rays.get_energy()) / N.trapezoid(spec, swl, axis=0)
        bundle = RayBundle(vertices=N.array(rays.get_vertices()), directions=N.array(rays.get_directions()),
                           energy=N.trapezoid(spec, swl, axis=0), spectra=spec, wavelengths=swl)
    dev = _device(ctx, cs, fs.PLATES_EDGES, _capacity(20000))
    with env(**knobs):
        st, _ = dev.trace_fast(bundle, 3, EMIN, 51, accel=True, stream=True)
    assert st.hits_dropped == 0
    ref = _captured(dev, frames, fs.PLATES_EDGES)
    fs.check_inputs(ref, fs.PLATES_EDGES)
    _check(dev, ref, fs.PLATES_EDGES, ('plates', form))
    a, r, h = dev.get_tallies()
    print('plates %s: hits %s, absorbed %s' % (form, h, a))
    assert h0.sum() > 20000 and (h0 > 500).all()
    assert N.array_equal(h, h0) and N.allclose(a, a0, rtol=1e-9, atol=0.) and N.allclose(r, r0, rtol=1e-9, atol=0.)
    dev.close()


def test_tally_layout_follows_the_transfer_matrix(ctx, plates):
    """The packed tally buffer of the five plates is [3 S + 2 | the 12 + 10 bins of the two maps], and (S + 1) S more while the
    transfer matrix is kept; every toggle gives a zeroed buffer with the maps at the same places.  With the matrix on, a trace's
    maps equal the host histogram of its hits, the matrix's columns sum to what the surfaces received and its last row (from the
    source) is what they receive in a trace of one bounce."""
    cs, frames, rays, _ = plates[False]
    S = cs.n_surf
    T = 3 * S + 2 + sum((len(u) - 1) * (len(v) - 1) for u, v in fs.PLATES_EDGES.values())
    assert T == 39
    dev = _device(ctx, cs, fs.PLATES_EDGES, _capacity(20000))
    assert dev.tally_size() == T
    for on, size in ((True, T + (S + 1) * S), (False, T), (True, T + (S + 1) * S)):
        dev.trace_fast(rays, 3, EMIN, 51, accel=True, stream=True)
        assert all(dev.get_fluxmap(s).any() for s in fs.PLATES_EDGES)
        dev.enable_transfer(on)
        assert dev.tally_size() == size
        assert all(dev.get_fluxmap(s).shape == (len(u) - 1, len(v) - 1) and not dev.get_fluxmap(s).any() for s, (u, v) in fs.PLATES_EDGES.items())
        assert not dev.export_tallies().any()
    dev.lib.trc_scene_clear_hits(dev.handle)
    st, _ = dev.trace_fast(rays, 3, EMIN, 51, accel=True, stream=True)
    assert st.hits_dropped == 0
    ref = _captured(dev, frames, fs.PLATES_EDGES)
    fs.check_inputs(ref, fs.PLATES_EDGES)
    _check(dev, ref, fs.PLATES_EDGES, 'matrix on')
    a, r, h = dev.get_tallies()
    M = dev.get_transfer()
    dev.close()
    one = _device(ctx, cs, fs.PLATES_EDGES, _capacity(20000))
    one.trace_fast(rays, 1, EMIN, 51, accel=True, stream=True)
    r1 = one.get_tallies()[1]
    one.close()
    print('matrix: from the source %s, first bounce received %s' % (M[-1], r1))
    assert r1.sum() > 0.5 * N.asarray(rays.get_energy()).sum()
    assert N.allclose(M.sum(axis=0), r, rtol=1e-9, atol=0.)
    assert N.allclose(M[-1], r1, rtol=1e-9, atol=0.) and N.isclose(M[-1].sum(), r1.sum(), rtol=1e-9, atol=0.)


def _plates_turned(turn):
    """the five plates with the mirror wall -y turned about its own x axis; the mapped surfaces stay"""
    from tracer_amd.scene import compile_scene
    from tracer_amd.spatial_geometry import rotx
    asm, T = fs.plates(False)
    wall = asm.get_objects()[4]
    wall.set_transform(N.dot(wall.get_transform(), rotx(turn)))
    cs = compile_scene(asm)
    return cs, [N.array(s._temp_frame) for s in cs.surfaces]


def test_update_frames_twice_then_a_trace(ctx, plates):
    """Two trc_scene_update_frames in a row (the search tables are rebuilt twice), then a trace: the maps equal the host histogram
    of that call's hits in the final poses, and tallies and maps are those of a scene compiled fresh in the final poses."""
    cs, frames, rays, (a0, r0, h0) = plates[False]
    (cs1, frames1), (cs2, frames2) = _plates_turned(0.25), _plates_turned(-0.15)
    assert all(N.array_equal(frames[s], frames2[s]) for s in fs.PLATES_EDGES)
    assert not N.array_equal(frames[4], frames1[4]) and not N.array_equal(frames1[4], frames2[4]) and not N.array_equal(frames[4], frames2[4])
    out = []
    for updates in (True, False):
        dev = _device(ctx, cs if updates else cs2, fs.PLATES_EDGES, _capacity(20000))
        if updates:
            dev.update_frames(cs1)
            dev.update_frames(cs2)
        st, _ = dev.trace_fast(rays, 3, EMIN, 51, accel=True, stream=True)
        assert st.hits_dropped == 0
        ref = _captured(dev, frames2, fs.PLATES_EDGES)
        fs.check_inputs(ref, fs.PLATES_EDGES)
        _check(dev, ref, fs.PLATES_EDGES, 'updated twice' if updates else 'compiled fresh')
        out.append((dev.get_tallies(), dict((s, dev.get_fluxmap(s)) for s in fs.PLATES_EDGES)))
        dev.close()
    ((a, r, h), maps), ((af, rf, hf), maps_f) = out
    assert not N.array_equal(h, h0)         # (the turned wall sends its rays elsewhere)
    assert N.array_equal(h, hf) and N.allclose(a, af, rtol=1e-9, atol=0.) and N.allclose(r, rf, rtol=1e-9, atol=0.)
    for s in fs.PLATES_EDGES:
        assert N.allclose(maps[s], maps_f[s], rtol=1e-9, atol=1e-9 * maps_f[s].max()), s
