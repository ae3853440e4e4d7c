"""
Tabulated materials evaluated on the device, per ray: TabulatedMaterial(..., device=True) sends its table
to the device with the scene, the engines evaluate m(lambda) at every hit between materials (trc_material_index; k_s_shade_x<.., MAT>,
k_ord_bounce<.., MAT>), a given bundle brings wavelengths only, and a source with a spectrum lights the scene while it stays pending.
The scene is the glass slab of test_gpu_media.py: two refracting plates over a black floor, air a constant table, glass a
dispersive one, 6 points from 0.3 to 2.5 um each; the wavelengths of the rays reach past both ends of the tables and sit on nodes.
The oracle evaluates the materials with their own m() (oracle.engine.trace_bundle).
"""
import ctypes as C
import os

import numpy as N
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NRAYS = 256 + 37            # several waves, the last one partial; 64 rays or more
TL = N.linspace(0.3e-6, 2.5e-6, 6)
GLASS_N = [1.55, 1.53, 1.51, 1.50, 1.49, 1.47]
GLASS_K = [3e-8, 2e-8, 1e-8, 5e-8, 2e-7, 6e-7]
SEED = 21


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context()


def _materials(device=True, glass_n=GLASS_N):
    from tracer_amd import optics_callables as opt
    air = opt.TabulatedMaterial(TL, N.ones(6), N.zeros(6), device=device)
    glass = opt.TabulatedMaterial(TL, glass_n, GLASS_K, device=device)
    return air, glass


def _slab_scene(single_ray, absorb=True, device=True, mats=None, glass_first=False):
    """glass_first: the optics name the glass as material_1, so a ray in the glass is known by `its index == glass.m(lambda)`,
    exactly, and any other ray enters the glass (optics_callables.py:750-751)"""
    from tracer_amd import optics_callables as opt
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.spatial_geometry import translate
    air, glass = mats if mats is not None else _materials(device)
    cls = opt.RefractiveAbsorbant if absorb else opt.Refractive
    kw = dict(attenuation_coefficient_1=1.) if absorb else {}
    if glass_first:
        cls = (lambda c: lambda a, g, **k: c(g, a, **k))(cls)
    top = AssembledObject(surfs=[Surface(RectPlateGM(40., 40.), cls(air, glass, single_ray=single_ray, **kw))], transform=translate(0., 0., 0.5))
    bottom = AssembledObject(surfs=[Surface(RectPlateGM(40., 40.), cls(air, glass, single_ray=single_ray, **kw))], transform=translate(0., 0., 0.))
    floor = AssembledObject(surfs=[Surface(RectPlateGM(60., 60.), opt.LambertianReceiver(1.))], transform=translate(0., 0., -1.))
    return Assembly(objects=[top, bottom, floor]), air, glass


N_INSIDE = 40


def _given(air, glass, n=NRAYS, seed=3, tilt=0.6):
    """rays from above the slab, the last N_INSIDE of them starting inside the glass with the index glass.m() gives the host;
    wavelengths over [0.25, 2.6] um (past both ends of the tables), a few exactly on nodes"""
    rng = N.random.RandomState(seed)
    v = N.vstack((rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), N.full(n, 3.)))
    d = N.vstack((rng.uniform(-tilt, tilt, n), rng.uniform(-tilt, tilt, n), -N.ones(n)))
    wl = rng.uniform(0.25e-6, 2.6e-6, n)
    wl[:6] = TL
    wl[n - 6:] = TL[::-1]
    inside = N.arange(n) >= n - N_INSIDE
    v[2, inside] = 0.25
    d[:2, inside] *= 0.3            # (steep enough to leave the glass whatever the wavelength)
    d /= N.sqrt(N.sum(d ** 2, axis=0))
    ref = N.where(inside, glass.m(wl), air.m(wl))
    return v, d, N.ones(n) / n, ref, wl, inside


def _bundle(cols):
    from tracer_amd.ray_bundle import RayBundle
    v, d, e, ref, wl, _ = cols
    return RayBundle(vertices=v.copy(), directions=d.copy(), energy=e.copy(), ref_index=ref.copy(), wavelengths=wl.copy())


def _oracle(cs, v, d, e, ref, wl, reps, seed=SEED, offset=0):
    from oracle import engine as oracle_engine
    with N.errstate(all='ignore'):
        return oracle_engine.trace_bundle(cs, v, d, e, reps, 1e-9, seed, ref_index=ref, wavelengths=wl, offset=offset)


def _assert_tallies(eng, o, what=''):
    a, r, h = [x.copy() for x in eng.get_tallies()]
    print(what, 'hits', h, o['hits'], 'segments', eng.stats['segments'], o['segments'], 'absorbed', a, o['absorbed'])
    assert N.array_equal(h, o['hits']) and eng.stats['segments'] == o['segments'], what
    assert N.allclose(a, o['absorbed'], rtol=1e-9, atol=1e-15) and N.allclose(r, o['received'], rtol=1e-9, atol=1e-15), what
    return a, r, h


# ---- 1. the lookup alone ------------------------------------------------------------------------------------------------------
def test_eval_materials_equals_material_rows(ctx):
    from tracer_amd.optics_callables import TabulatedMaterial, Refractive
    from tracer_amd.scene import compile_scene, DeviceScene, material_rows
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    rng = N.random.RandomState(5)
    big = N.cumsum(rng.uniform(1e-10, 1e-9, 4096)) + 0.3e-6
    mats = [TabulatedMaterial(TL, GLASS_N, GLASS_K, device=True),
            TabulatedMaterial([0.5e-6, 1.5e-6], [1.3, 1.4], [0., 1e-6], device=True),
            TabulatedMaterial(big, rng.uniform(1., 3., 4096), rng.uniform(0., 1e-3, 4096), device=True)]
    asm = Assembly(objects=[AssembledObject(surfs=[Surface(RectPlateGM(1., 1.), Refractive(mats[0], mats[1])),
                                                   Surface(RectPlateGM(1., 1.), Refractive(mats[0], mats[2]))])])
    cs = compile_scene(asm)
    assert cs.materials == mats and cs.material_tables is not None
    dev = DeviceScene(cs, ctx)
    assert dev.materials_on_device()
    wl = N.concatenate((rng.uniform(0.25e-6, 2.6e-6, 3000), rng.uniform(big[0], big[-1], 3000), TL, big, [0.5e-6, 1.5e-6],
                        N.nextafter(big[:50], N.inf), [0., -1., N.inf, -N.inf, N.nan]))
    with N.errstate(all='ignore'):
        want = material_rows(mats, wl)
    got = dev.material_rows(wl)
    assert got.shape == want.shape == (6, len(wl))
    nan = N.isnan(want)
    assert N.array_equal(nan, N.isnan(got)) and nan.sum() == 6
    assert N.array_equal(got[~nan].view(N.int64), want[~nan].view(N.int64))
    dev.close()


# ---- 2. a given bundle on the streaming form ------------------------------------------------------------------------------------
@pytest.mark.parametrize('single_ray', [True, False])
@pytest.mark.parametrize('absorb', [True, False])
def test_given_bundle_on_the_streaming_form(ctx, single_ray, absorb):
    from tracer_amd.tracer_engine import TracerEngine
    from tracer_amd.scene import compile_scene
    import tracer_amd.scene as scene_mod
    reps = 6
    asm, air, glass = _slab_scene(single_ray, absorb)
    cols = _given(air, glass)
    called = []
    host_rows = scene_mod.material_rows
    scene_mod.material_rows = lambda *a, **k: called.append(1) or host_rows(*a, **k)
    try:
        eng = TracerEngine(asm)
        eng.ray_tracer(_bundle(cols), reps=reps, min_energy=1e-9, tree=False, seed=SEED)
    finally:
        scene_mod.material_rows = host_rows
    assert not called                           # the host evaluated no material
    assert eng.stats['engine'] == 'fast' and eng.stats['form'] == 'stream'
    cs = compile_scene(asm)
    assert cs.material_tables is not None
    o = _oracle(cs, *cols[:5], reps=reps)
    a, r, h = _assert_tallies(eng, o, 'device tables')
    e_floor, p_floor = asm.get_surfaces()[2].get_optics_manager().get_all_hits()
    assert len(e_floor) == h[2] > NRAYS // 2
    # Rays that start inside the glass with the host's glass.m(wl) as their index, alone, on a slab whose optics know a ray in the
    # glass by `index == glass.m(lambda)`: the device's value has the host's bits, or they would be taken for rays in air, "enter"
    # the glass at its underside without bending or reflecting and arrive with other energies.  They leave into air and reach the floor.
    from tracer_amd.ray_bundle import RayBundle
    inside = cols[5]
    pad = 64 // N_INSIDE + 1        # (64 rays or more for the streaming form: the rays several times over)
    tiled = tuple(N.concatenate([c[..., inside]] * pad, axis=-1) for c in cols[:5])
    asm_i, _, _ = _slab_scene(single_ray, absorb, glass_first=True)
    eng_i = TracerEngine(asm_i)
    eng_i.ray_tracer(RayBundle(vertices=tiled[0], directions=tiled[1], energy=tiled[2], ref_index=tiled[3], wavelengths=tiled[4]),
                     reps=reps, min_energy=1e-9, tree=False, seed=SEED)
    assert eng_i.stats['engine'] == 'fast' and eng_i.stats['form'] == 'stream'
    o_i = _oracle(compile_scene(asm_i), *tiled, reps=reps)
    _, _, h_i = _assert_tallies(eng_i, o_i, 'rays from inside the glass')
    L1 = o_i['levels'][1]
    out = (L1['surf'] == 1) & (L1['directions'][2] < 0)
    assert out.sum() >= pad * N_INSIDE // 2 and (L1['ref'][out] == 1.).all() and (N.abs(tiled[3] - 1.) > 0.4).all()
    assert h_i[2] >= pad * N_INSIDE // 2
    # today's route, rows from the host: the same counts, the same energies
    asm_h, air_h, glass_h = _slab_scene(single_ray, absorb, device=False)
    eng_h = TracerEngine(asm_h)
    eng_h.ray_tracer(_bundle(cols), reps=reps, min_energy=1e-9, tree=False, seed=SEED)
    assert eng_h.stats['engine'] == 'fast' and eng_h.stats['form'] == 'stream' and compile_scene(asm_h).material_tables is None
    a_h, r_h, h_h = eng_h.get_tallies()
    assert N.array_equal(h_h, h) and eng_h.stats['segments'] == eng.stats['segments']
    assert N.allclose(a_h, a, rtol=1e-9, atol=1e-15) and N.allclose(r_h, r, rtol=1e-9, atol=1e-15)


# ---- 3., 4. a pending source with a spectrum --------------------------------------------------------------------------------------
def _spectrum():
    from tracer_amd.source_spectrum import SourceSpectrum
    rng = N.random.RandomState(17)
    wl = N.sort(N.concatenate(([0.27e-6, 2.58e-6], rng.uniform(0.27e-6, 2.58e-6, 21))))       # 23 irregular points, past the tables' ends
    return SourceSpectrum.tabulated(wl, rng.uniform(0.2, 1., 23), ref_index=1.)


def _source(n=NRAYS, seed=77, offset=1000, spectrum=None, tilt=0.):
    from tracer_amd.sources import rect_bundle
    direction = N.array([N.sin(tilt), 0., -N.cos(tilt)])
    return rect_bundle(n, N.array([0., 0., 3.]), direction, 2., 2., 0.3 if tilt == 0. else 0., flux=1.,
                       seed=seed, ray_offset=offset, spectrum=_spectrum() if spectrum is None else spectrum)


def _host_rays(src):
    """the rays of a pending source as the oracle generates them, with the wavelengths of the host-compiled sampler
    (tests/hostcheck; the `host_wavelengths` recipe of tests/shade_cases.py)"""
    from oracle import sources as oracle_sources, engine as oracle_engine
    desc, n, seed, off = src.source_args()
    v, d, e, rid = oracle_sources.generate(oracle_engine.source_from_desc(desc), n, seed, off)
    assert N.array_equal(rid, N.arange(n, dtype=N.uint64) + N.uint64(off))
    sp = src.source_spectrum()
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_spectrum_check.so'))
    p = C.POINTER(C.c_double)
    lib.hs_spectrum_draw.argtypes = [p, p, p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_long, p, p]
    wl, val, cdf = [N.ascontiguousarray(a, dtype=float) for a in sp.table()]
    out = N.empty(n)
    lib.hs_spectrum_draw(wl.ctypes.data_as(p), val.ctypes.data_as(p), cdf.ctypes.data_as(p), wl.size, seed, off, n, None, out.ctypes.data_as(p))
    return v, d, e, N.full(n, sp.ref_index), out, seed, off


def _compare_levels(tree, o):
    """parents exactly, geometry to 1e-9, complex index to 1e-12 (test_gpu_media.py)"""
    for k in range(1, min(tree.num_bunds(), len(o['levels']))):
        B, Lo = tree[k], o['levels'][k]
        assert N.array_equal(B.get_parents(), Lo['parents']), k
        assert N.allclose(B.get_vertices(), Lo['vertices'], rtol=1e-9, atol=1e-9), k
        assert N.allclose(B.get_directions(), Lo['directions'], rtol=1e-9, atol=1e-9), k
        assert N.allclose(B.get_energy(), Lo['energy'], rtol=1e-9, atol=1e-15), k
        assert N.iscomplexobj(B.get_ref_index()) and N.allclose(B.get_ref_index(), Lo['ref'], rtol=1e-12, atol=0), k
    assert tree.num_bunds() == len(o['levels'])


_PENDING_REF = {}


def _pending_reference(single_ray, absorb, n, reps):
    from tracer_amd.scene import compile_scene
    key = (single_ray, absorb, n, reps)
    if key not in _PENDING_REF:
        asm, _, _ = _slab_scene(single_ray, absorb)
        v, d, e, ref, wl, seed, off = _host_rays(_source(n))
        assert n < NRAYS or (wl.min() < TL[0] and wl.max() > TL[-1])       # the spectrum reaches past both ends of the tables
        _PENDING_REF[key] = (_oracle(compile_scene(asm), v, d, e, ref, wl, reps, seed=seed, offset=off), wl)
    return _PENDING_REF[key]


@pytest.mark.parametrize('single_ray', [True, False])
@pytest.mark.parametrize('absorb', [True, False])
def test_pending_spectral_source_on_the_streaming_form(ctx, single_ray, absorb):
    from tracer_amd.tracer_engine import TracerEngine
    reps = 7
    asm, air, glass = _slab_scene(single_ray, absorb)
    src = _source()
    eng = TracerEngine(asm)
    eng.ray_tracer(src, reps=reps, min_energy=1e-9, tree=False, seed=5)      # (a source bundle keeps its own seed)
    assert src.is_pending()
    assert eng.stats['engine'] == 'fast' and eng.stats['form'] == 'stream'
    o, _ = _pending_reference(single_ray, absorb, NRAYS, reps)
    a, r, h = _assert_tallies(eng, o, 'pending source')
    assert h[2] > NRAYS // 2


@pytest.mark.parametrize('single_ray', [True, False])
def test_pending_spectral_source_on_the_ordered_engine(ctx, single_ray):
    from tracer_amd.tracer_engine import TracerEngine
    reps = 6
    for n in (NRAYS, 40):
        asm, air, glass = _slab_scene(single_ray)
        src = _source(n)
        eng = TracerEngine(asm)
        eng.ray_tracer(src, reps=reps, min_energy=1e-9, tree=(n == NRAYS), seed=5)
        assert eng.stats['engine'] == 'ordered' and src.is_pending()
        o, wl = _pending_reference(single_ray, True, n, reps)
        _assert_tallies(eng, o, 'ordered, %d rays' % n)
        if n == NRAYS:
            _compare_levels(eng.tree, o)
            assert N.array_equal(eng.tree[0].get_wavelengths(), wl)
            assert N.array_equal(eng.tree[1].get_wavelengths(), wl[o['levels'][1]['parents']])
        else:       # (tree=False: the last level alone)
            last = o['levels'][-1]
            assert N.allclose(eng.tree[-1].get_vertices(), last['vertices'], rtol=1e-9, atol=1e-9)
            assert N.allclose(eng.tree[-1].get_energy(), last['energy'], rtol=1e-9, atol=1e-15)


# ---- 5. known answers ---------------------------------------------------------------------------------------------------------------
def test_known_answers(ctx):
    from tracer_amd.tracer_engine import TracerEngine
    from tracer_amd.source_spectrum import SourceSpectrum
    from tracer_amd.sources import rect_bundle
    # normal incidence, one wavelength, splitting optics, reps = 3 (top, bottom, floor): Fresnel twice, Beer-Lambert once -- the
    # formula of test_gpu_media.test_absorbing_slab_between_tabulated_materials
    lam = 2.0e-6
    m = 128
    asm, air, glass = _slab_scene(False)
    src = rect_bundle(m, N.array([0., 0., 3.]), N.array([0., 0., -1.]), 2., 2., 0., flux=m / 4., seed=9,
                      spectrum=SourceSpectrum.monochromatic(lam))
    eng = TracerEngine(asm)
    eng.ray_tracer(src, reps=3, min_energy=1e-12, tree=False)
    assert eng.stats['engine'] == 'fast' and eng.stats['form'] == 'stream' and src.is_pending()
    mg = glass.m(N.array([lam]))[0]
    R = (((1. - mg) / (1. + mg)) ** 2).real
    T_in = N.exp(-4. * N.pi * 2.5 * mg.imag / lam)
    e0 = src.source_args()[0].energy
    absorbed, hits = asm.get_surfaces()[2].get_optics_manager().get_all_hits()
    assert len(absorbed) == m and N.allclose(hits[2], -1.) and T_in < 0.5 and e0 > 0.
    assert N.allclose(absorbed, e0 * (1. - R) * T_in * (1. - R), rtol=1e-12, atol=0)
    # two colours through the slab at 0.5 rad, one ray per hit, no attenuation: the rays refracted on both faces land where Snell's
    # law with n(lambda) puts them -- apart from each other (dispersion)
    tilt = 0.5
    inside_shift = {}
    for lam in (0.4e-6, 2.4e-6):
        asm, air, glass = _slab_scene(True, absorb=False)
        src = _source(200, seed=31, offset=0, spectrum=SourceSpectrum.monochromatic(lam), tilt=tilt)
        eng = TracerEngine(asm)
        eng.ray_tracer(src, reps=3, min_energy=1e-12, tree=False)
        assert eng.stats['form'] == 'stream' and src.is_pending()
        e_hit, p = asm.get_surfaces()[2].get_optics_manager().get_all_hits()
        v0, d0 = _host_rays_geometry(src)            # where each ray started: the oracle's generator on the same descriptor and streams
        assert N.allclose(d0, N.c_[[N.sin(tilt), 0., -N.cos(tilt)]], rtol=0, atol=1e-15)
        ng = glass.m(N.array([lam]))[0].real
        th2 = N.arcsin(N.sin(tilt) / ng)
        # air down to the top plate at z = 0.5, half a metre of glass, a metre of air to the floor at z = -1; y stays
        want_x = v0[0] + (v0[2] - 0.5) * N.tan(tilt) + 0.5 * N.tan(th2) + 1. * N.tan(tilt)
        # (a ray reflected at a face never reaches the floor in three interactions: every hit there was refracted twice)
        assert 150 < p.shape[1] <= 200
        k = N.argmin(N.abs(p[1][:, None] - v0[1][None, :]), axis=1)          # the source ray of each hit, by its y
        assert len(set(k.tolist())) == len(k) and N.allclose(p[1], v0[1][k], rtol=0, atol=1e-9)
        assert N.allclose(p[0], want_x[k], rtol=0, atol=1e-9)
        inside_shift[lam] = 0.5 * N.tan(th2)
    assert abs(inside_shift[0.4e-6] - inside_shift[2.4e-6]) > 5e-3        # n = 1.5409 against 1.4791: millimetres apart


def _host_rays_geometry(src):
    from oracle import sources as oracle_sources, engine as oracle_engine
    desc, n, seed, off = src.source_args()
    return oracle_sources.generate(oracle_engine.source_from_desc(desc), n, seed, off)[:2]


# ---- 6. routes and refusals ---------------------------------------------------------------------------------------------------------
def test_routes_and_refusals(ctx):
    from tracer_amd import _cabi
    from tracer_amd.tracer_engine import TracerEngine
    from tracer_amd._cabi import TracerAmdError
    from tracer_amd.sources import rect_bundle
    from tracer_amd.scene import compile_scene, DeviceScene
    reps = 6
    for single_ray in (True, False):
        asm, air, glass = _slab_scene(single_ray)
        eng = TracerEngine(asm)
        with pytest.raises(TracerAmdError) as err:
            eng.ray_tracer(_source(), reps=reps, min_energy=1e-9, tree=False, engine='fast', fast_kernel='megakernel')
        assert 'trc_trace_ordered' in str(err.value) and err.value.status == _cabi.ERR_UNSUPPORTED
        with pytest.raises(TracerAmdError) as err:
            eng.ray_tracer(_source(40), reps=reps, min_energy=1e-9, tree=False, engine='fast')
        assert 'trc_trace_ordered' in str(err.value) and err.value.status == _cabi.ERR_UNSUPPORTED
        plain = rect_bundle(NRAYS, N.array([0., 0., 3.]), N.array([0., 0., -1.]), 2., 2., 0.3, flux=1., seed=77)
        for engine in ('fast', 'ordered'):
            with pytest.raises(TracerAmdError) as err:      # no spectrum: rays of wavelength 0
                eng.ray_tracer(plain, reps=reps, min_energy=1e-9, tree=False, engine=engine)
            assert err.value.status == _cabi.ERR_INVALID and 'spectrum' in str(err.value)
    # one material that stays on the host: the bundle is materialised and traced as a given one, as today
    mats = _materials()
    mats_mixed = (mats[0], _materials(device=False)[1])
    asm, air, glass = _slab_scene(True, mats=mats_mixed)
    assert compile_scene(asm).material_tables is None
    src = _source()
    eng = TracerEngine(asm)
    eng.ray_tracer(src, reps=reps, min_energy=1e-9, tree=False, seed=5)
    assert not src.is_pending()
    # (materialised, the bundle is a given one: its rays take the call's seed and the stream ids 0, 1, ...)
    v, d, e, ref, wl, seed, off = _host_rays(_source())
    o_mixed = _oracle(compile_scene(asm), v, d, e, ref, wl, reps, seed=5, offset=0)
    _assert_tallies(eng, o_mixed, 'one host material')


def test_rows_and_new_tables_at_the_c_abi(ctx):
    """A bundle that brings trc_rays.mat on a scene with tables is traced by its rows; tables set again are the ones the next
    call reads."""
    from tracer_amd import _cabi
    from tracer_amd.scene import compile_scene, DeviceScene, material_rows
    reps = 6
    asm, air, glass = _slab_scene(True)
    cols = _given(air, glass)
    v, d, e, ref, wl, _ = cols
    cs = compile_scene(asm)
    o = _oracle(cs, *cols[:5], reps=reps)

    def trace(dev, mat=None, ref=ref):
        dev.reset_tallies()
        c = [N.ascontiguousarray(x) for x in (v[0], v[1], v[2], d[0], d[1], d[2], e, ref.real, wl, ref.imag)]
        rays = _cabi.make_rays(len(e), *c[:7], ref_index=c[7], wavelength=c[8], ref_index_im=c[9], mat=mat)
        stats = _cabi.TraceStats()
        _cabi.check(dev.lib.trc_trace_fast_x(dev.handle, C.byref(rays), None, None, len(e), reps, 1e-9, SEED, 0, _cabi.TRACE_STREAM, None,
                                             C.byref(stats)))
        return dev.get_tallies(), stats

    dev = DeviceScene(cs, ctx)
    (a, r, h), st = trace(dev)
    assert N.array_equal(h, o['hits']) and st.segments == o['segments'] and N.allclose(a, o['absorbed'], rtol=1e-9, atol=1e-15)
    # rows of another glass, brought by the bundle: they win over the scene's tables
    air2, glass2 = _materials(glass_n=[1.75, 1.73, 1.71, 1.70, 1.69, 1.67])
    asm2, _, _ = _slab_scene(True, mats=(air2, glass2))
    cs2 = compile_scene(asm2)
    ref2 = N.where(cols[5], glass2.m(wl), air2.m(wl))
    o2 = _oracle(cs2, v, d, e, ref2, wl, reps=reps)
    assert not N.allclose(o2['absorbed'], o['absorbed'], rtol=1e-6, atol=0)
    (a_r, r_r, h_r), st_r = trace(dev, mat=material_rows([air2, glass2], wl), ref=ref2)
    assert N.array_equal(h_r, o2['hits']) and st_r.segments == o2['segments'] and N.allclose(a_r, o2['absorbed'], rtol=1e-9, atol=1e-15)
    # ... and the scene's own rows give the result of the tables
    (a_s, r_s, h_s), st_s = trace(dev, mat=material_rows([air, glass], wl))
    assert N.array_equal(h_s, h) and st_s.segments == st.segments and N.allclose(a_s, a, rtol=1e-9, atol=1e-15)
    # new tables on the same scene
    dev.set_materials(*cs2.material_tables)
    (a_n, r_n, h_n), st_n = trace(dev, ref=ref2)
    assert N.array_equal(h_n, o2['hits']) and st_n.segments == o2['segments'] and N.allclose(a_n, o2['absorbed'], rtol=1e-9, atol=1e-15)
    # without tables the scene asks for rows again
    dev.set_materials([], [])
    with pytest.raises(_cabi.TracerAmdError) as err:
        trace(dev)
    assert err.value.status == _cabi.ERR_INVALID and 'trc_rays.mat' in str(err.value)
    # tables the library refuses
    for npts, packed in (([1], [1e-6, 1., 0.]), ([2], [2e-6, 1e-6, 1., 1., 0., 0.]), ([2], [1e-6, 2e-6, 1., N.nan, 0., 0.]), ([4097], N.zeros(3 * 4097))):
        with pytest.raises(_cabi.TracerAmdError) as err:
            dev.set_materials(npts, packed)
        assert err.value.status == _cabi.ERR_INVALID
    dev.close()
