"""
The flux-map charts without a device: the per-ray core's chart function and bin index (trc_fluxmap_uv, trc_bin_index, compiled for
the host by `make hostcheck`) against the NumPy formulas and numpy.histogram2d; the hand-written tables of hits on edges against
histogram2d; the geometry managers' fluxmap_grid against the reference's own get_fluxmap arrays (tests/golden/fluxmap_charts.npz,
written by tests/golden/make_golden_fluxmaps.py); and what the device tests (test_gpu_fluxmap_charts.py) take for granted about
their inputs, from the oracle's hits of a tenth of the device case.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

import fluxmap_chart_scene as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHART_NO = dict((c, i) for i, c in enumerate(fc.CHARTS))
_f64 = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_f64)


@pytest.fixture(scope='module')
def lib():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_fluxmap_check.so'))
    lib.hf_fluxmap_uv.argtypes = [C.c_int, _f64, C.c_long] + [_f64] * 5
    lib.hf_fluxmap_bin.argtypes = [C.c_int, _f64, C.c_int, C.c_int, _f64, _f64, C.c_long, _f64, _f64, _f64, C.POINTER(C.c_long)]
    return lib


def _host_bins(lib, chart, proj, ue, ve, pts):
    p = N.ascontiguousarray(proj[:3].ravel())
    x, y, z = [N.ascontiguousarray(c, dtype=float) for c in pts]
    ue, ve = N.ascontiguousarray(ue, dtype=float), N.ascontiguousarray(ve, dtype=float)
    out = N.empty(len(x), dtype=N.int64)
    lib.hf_fluxmap_bin(CHART_NO[chart], _ptr(p), len(ue) - 1, len(ve) - 1, _ptr(ue), _ptr(ve), len(x), _ptr(x), _ptr(y), _ptr(z),
                       out.ctypes.data_as(C.POINTER(C.c_long)))
    return out


@pytest.fixture(scope='module')
def cloud():
    """1e5 random local points per chart under a general frame: (frame, {chart: global points})"""
    from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
    frame = N.dot(translate(3.1, -2.2, 0.7), N.dot(rotx(0.9), N.dot(roty(-0.3), rotz(2.1))))
    rng = N.random.RandomState(5)
    out = {}
    for chart in fc.CHARTS:
        local = N.vstack((rng.uniform(-2., 2., (3, 100000)), N.ones(100000)))
        out[chart] = N.dot(frame, local)[:3]
    return frame, out


def test_the_chart_numbers_are_the_headers(lib):
    from tracer_amd import _cabi
    assert lib.hf_n_charts() == len(fc.CHARTS) == len(_cabi.FM_CHARTS)
    assert [_cabi.FM_CHARTS[c] for c in fc.CHARTS] == [0, 1, 2, 3]
    header = open(os.path.join(ROOT, 'include', 'tracer_amd.h')).read()
    assert 'TRC_FM_XY = 0, TRC_FM_CYLINDER = 1, TRC_FM_POLAR = 2, TRC_FM_SPHERE = 3' in header


@pytest.mark.parametrize('chart', fc.CHARTS)
def test_chart_function_is_the_numpy_formula(lib, cloud, chart):
    """1e-12 absolute: a wrong formula (swapped arguments, a missing wrap) is off by 1e-3 or more, two correct libm
    implementations by a few ulp of values that are at most 2 pi"""
    frame, pts = cloud
    proj = fc.projection(frame)
    x, y, z = [N.ascontiguousarray(c) for c in pts[chart]]
    u, v = N.empty(len(x)), N.empty(len(x))
    lib.hf_fluxmap_uv(CHART_NO[chart], _ptr(N.ascontiguousarray(proj[:3].ravel())), len(x), _ptr(x), _ptr(y), _ptr(z), _ptr(u), _ptr(v))
    hu, hv = fc.chart_uv(chart, proj, pts[chart])
    print(chart, 'largest difference', N.abs(u - hu).max(), N.abs(v - hv).max())
    assert N.abs(u - hu).max() <= 1e-12 and N.abs(v - hv).max() <= 1e-12
    if chart == 'xy':
        assert N.array_equal(u, hu) and N.array_equal(v, hv)          # today's arithmetic, bit for bit
    else:
        assert hv.min() >= 0. and hv.max() <= 2. * N.pi and (hv > N.pi).mean() > 0.4
    # rows 0 and 1 exchanged: the azimuth is arctan2(x, y)
    if chart == 'polar':
        lib.hf_fluxmap_uv(CHART_NO[chart], _ptr(N.ascontiguousarray(fc.projection(frame, True)[:3].ravel())), len(x), _ptr(x), _ptr(y), _ptr(z), _ptr(u), _ptr(v))
        local = N.dot(proj, N.vstack((pts[chart], N.ones(len(x)))))
        az = N.arctan2(local[0], local[1])
        az[az < 0.] += 2. * N.pi
        assert N.abs(v - az).max() <= 1e-9                            # (the dot product sums in another order)


# edges per chart over local points of +-2 in every coordinate: part of the points outside in u and in v
CLOUD_EDGES = {'xy': (N.linspace(-1.5, 1.8, 12), fc.fs.nonuniform(-1.9, 1.2, 7)),
               'cylinder': (fc.fs.nonuniform(-1.7, 1.5, 9), N.linspace(0.3, 5.5, 14)),
               'polar': (N.linspace(0.2, 2.4, 10), N.linspace(0., 2. * N.pi, 17)),
               'sphere': (N.linspace(0.4, 2.6, 8), fc.fs.nonuniform(0., 2. * N.pi, 11))}


@pytest.mark.parametrize('chart', fc.CHARTS)
def test_bin_index_is_histogram2ds(lib, cloud, chart):
    """the full bin index against numpy.histogram2d on the same points, leaving out those whose NumPy coordinate lies within 1e-12
    of an edge (at most 0.1 % of them; uniform random points leave out about 1e-9 of themselves)"""
    frame, pts = cloud
    proj = fc.projection(frame)
    ue, ve = CLOUD_EDGES[chart]
    u, v = fc.chart_uv(chart, proj, pts[chart])
    keep = ~(fc.near_edge(u, ue) | fc.near_edge(v, ve))
    assert (~keep).mean() <= 1e-3
    u, v = u[keep], v[keep]
    got = _host_bins(lib, chart, proj, ue, ve, pts[chart][:, keep])
    nv = len(ve) - 1
    inside = (u >= ue[0]) & (u <= ue[-1]) & (v >= ve[0]) & (v <= ve[-1])
    assert 0.05 < (~inside).mean() < 0.95 and N.array_equal(got >= 0, inside)
    H = N.histogram2d(u, v, bins=[ue, ve])[0]
    mine = N.bincount(got[got >= 0], minlength=H.size).reshape(H.shape)
    assert N.array_equal(mine, H) and (H > 0).mean() > 0.5
    # ... and point by point: numpy's own rule for a coordinate (the last bin closed on the right)
    iu = N.minimum(N.searchsorted(ue, u[inside], side='right') - 1, len(ue) - 2)
    iv = N.minimum(N.searchsorted(ve, v[inside], side='right') - 1, nv - 1)
    assert N.array_equal(got[inside], iu * nv + iv)


def test_nan_coordinates_are_outside_every_map(lib):
    """the centre of a sphere has no polar angle (0 / 0), and a NaN point has no coordinate at all: outside, never a wild index"""
    pts = N.array([[0., N.nan, 1.], [0., 0., N.nan], [0., 2., 0.]])
    for chart in fc.CHARTS[1:]:
        ue, ve = CLOUD_EDGES[chart]
        got = _host_bins(lib, chart, N.eye(4), ue, ve, pts)
        assert got[1] == -1 and got[2] == -1
        if chart == 'sphere':
            assert got[0] == -1


@pytest.mark.parametrize('chart', ['cylinder', 'polar', 'sphere'])
def test_hand_written_edge_table_is_numpys(lib, chart):
    x, y, e, want, outside = fc.edge_cases(chart)
    ue, ve = fc.EDGE_EDGES[chart]
    pts = N.vstack((x, y, N.zeros(len(x))))
    u, v = fc.chart_uv(chart, fc.EDGE_PROJ[chart], pts)
    H = N.histogram2d(u, v, bins=[ue, ve], weights=e)[0]
    assert N.array_equal(H, want), N.argwhere(H != want)
    assert outside == e.sum() - want.sum() > 0 and (want > 0).mean() >= 0.4
    # the points are where the table says the arithmetic is exact
    if chart == 'cylinder':
        assert N.array_equal(u, x) and set(v[y == 0.]) == {0.} and set(v[y == fc.TINY]) == {2. * N.pi}
    if chart == 'polar':
        on_axis = (y == 0.) | (y == fc.TINY)
        assert N.array_equal(u[on_axis], x[on_axis]) and set(v[y == fc.TINY]) == {2. * N.pi}
        assert N.array_equal(u[~on_axis], 1.25 * N.maximum(N.abs(x), N.abs(y))[~on_axis])       # 3-4-5
    if chart == 'sphere':
        assert set(u[(x == 0.) & (y > 0.)]) == {0.} and set(v[x > 0.]) == {0.}
    # the core puts every point in the bin of the table
    got = _host_bins(lib, chart, fc.EDGE_PROJ[chart], ue, ve, pts)
    mine = N.zeros(want.size)
    N.add.at(mine, got[got >= 0], e[got >= 0])
    assert N.array_equal(mine.reshape(want.shape), want) and e[got < 0].sum() == outside


# -- the geometry managers' grids against the reference's own arrays -----------------------------------------------------------------
def _golden_gm(name):
    from tracer_amd.flat_surface import RectPlateGM, RoundPlateGM
    from tracer_amd.cylinder import FiniteCylinder
    from tracer_amd.paraboloid import ParabolicDishGM
    from tracer_amd.sphere_surface import SphericalGM
    return {'rect': lambda: RectPlateGM(3., 2.), 'round': lambda: RoundPlateGM(1.7), 'round_ri': lambda: RoundPlateGM(1.7, 0.6),
            'cylinder': lambda: FiniteCylinder(1.2, 1.4), 'cylinder_part': lambda: FiniteCylinder(1.2, 1.4, (0.4, 3.9)),
            'dish': lambda: ParabolicDishGM(1.6, 1.), 'sphere': lambda: SphericalGM(0.5)}[name]()


@pytest.fixture(scope='module')
def golden():
    return N.load(os.path.join(ROOT, 'tests', 'golden', 'fluxmap_charts.npz'))


@pytest.mark.parametrize('name', ['rect', 'round', 'round_ri', 'cylinder', 'cylinder_part', 'dish', 'sphere'])
def test_fluxmap_grid_reproduces_the_references_get_fluxmap(golden, name):
    """Binning the chart coordinates on fluxmap_grid's edges and dividing by its areas gives the reference's array (rtol 1e-12: only
    the order of sums differs); so does our own get_fluxmap, which therefore agrees with fluxmap_grid."""
    assert name in list(golden['names'])
    gm = _golden_gm(name)
    pts, e = golden[name + '_points'], golden[name + '_energy']
    for res in golden['resolutions']:
        res = int(res)
        want = golden['%s_flux_%d' % (name, res)]
        chart, swap, ue, ve, areas = gm.fluxmap_grid(res)
        proj = N.eye(4)[[1, 0, 2, 3]] if swap else N.eye(4)
        u, v = fc.chart_uv(chart, proj, pts)
        H = N.histogram2d(u, v, bins=[ue, ve], weights=e)[0]
        assert areas.shape == H.shape and (areas > 0).all()
        got = N.hstack(H / areas)
        assert got.shape == want.shape and (want > 0).mean() > 0.2
        assert N.allclose(got, want, rtol=1e-12, atol=0.), (name, res, N.abs(got - want).max())
        assert N.allclose(gm.get_fluxmap(e.copy(), pts.copy(), res), want, rtol=1e-12, atol=0.)
    assert swap == name.startswith('round')
    assert chart == {'rect': 'xy', 'round': 'polar', 'round_ri': 'polar', 'cylinder': 'cylinder', 'cylinder_part': 'cylinder',
                     'dish': 'polar', 'sphere': 'sphere'}[name]


def test_default_resolution_and_geometries_without_a_grid():
    from tracer_amd.flat_surface import RoundPlateGM, ExtrudedRectPlateGM, StraightCutRoundPlateGM, PerforatedRectPlateGM
    from tracer_amd.cone import ConicalFrustum
    from tracer_amd.sphere_surface import HemisphereGM
    chart, swap, rs, angs, areas = RoundPlateGM(2.).fluxmap_grid(None)          # (the reference's default of 40)
    assert len(rs) == 41 and areas.shape == (40, len(angs) - 1)
    assert PerforatedRectPlateGM(2., 2., [[0., 0.]], [0.1]).fluxmap_grid(3)[0] == 'xy'        # children inherit it
    assert HemisphereGM(1.).fluxmap_grid(3)[0] == 'sphere'
    for gm in (ExtrudedRectPlateGM(4., 4., N.c_[[0., 0.]], 1., 1.), StraightCutRoundPlateGM(1., 0.5)):
        with pytest.raises(NotImplementedError):
            gm.fluxmap_grid(6)
    assert not hasattr(ConicalFrustum(0., 0.5, 0.6, 0.9), 'fluxmap_grid')


def test_engine_keeps_chart_requests_and_refuses_what_it_cannot_map():
    """no device needed: the request is recorded for the next scene build, an unknown chart and a geometry without a grid are refused"""
    from tracer_amd.tracer_engine import TracerEngine
    asm, objs, T = fc.receivers()
    eng = TracerEngine(asm)
    with pytest.raises(ValueError, match='unknown flux-map chart'):
        eng.set_fluxmap(fc.CYLINDER, [0., 1.], [0., 1.], chart='conical')
    with pytest.raises(NotImplementedError):
        eng.set_surface_fluxmap(fc.FRUSTUM, 4)
    eng.set_surface_fluxmap(asm.get_surfaces()[fc.FLOOR], 6)
    eng.set_fluxmap(fc.FRUSTUM, [0., 0.3, 0.6], [0., 3., 6.3], chart='cylinder')
    u, v, chart, swap = eng._fluxmap_requests[fc.FLOOR]
    assert (chart, swap, len(u)) == ('polar', True, 7) and eng._fluxmap_areas[fc.FLOOR].shape == (6, len(v) - 1)
    assert eng._fluxmap_requests[fc.FRUSTUM][2:] == ('cylinder', False)
    # a map without bin areas, and a map that no trace has filled yet, are said so
    with pytest.raises(ValueError, match='no flux map set by set_surface_fluxmap'):
        eng.get_surface_flux(fc.FRUSTUM)
    with pytest.raises(ValueError, match='no trace since'):
        eng.get_surface_flux(fc.FLOOR)
    eng.set_fluxmap(fc.FLOOR, [0., 1., 2.], [0., 3., 6.3], chart='polar')         # (replaces the geometry's map: its areas go)
    with pytest.raises(ValueError, match='no flux map set by set_surface_fluxmap'):
        eng.get_surface_flux(fc.FLOOR)


# -- the inputs of the device tests ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def oracle_hits():
    from tracer_amd.scene import compile_scene
    from oracle import engine
    asm, objs, T = fc.receivers()
    cs = compile_scene(asm)
    n = 20000               # a tenth of the device case: what is filled here is filled there
    o = engine.trace_from_compiled(cs, fc.source(n, T, seed=11).source_args(), 12, 1e-10)
    return cs, o, n


@pytest.mark.parametrize('regime', sorted(fc.FLOOR_BINS))
def test_host_histograms_of_the_receivers_meet_the_conditions_on_the_inputs(oracle_hits, regime):
    cs, o, n = oracle_hits
    frames = [s._temp_frame for s in cs.surfaces]
    for f in frames:        # no frame is axis aligned
        assert (N.abs(f[:3, :3]) > 1e-3).sum() >= 8 and N.abs(f[:3, 3]).min() > 1.
    maps = fc.maps(regime)
    assert sorted(maps) == list(range(cs.n_surf)) and all(len(u) != len(v) for _, _, u, v in maps.values())
    ref = fc.host_maps(fc.fs.hits_of_levels(o['levels']), frames, maps)
    fc.check_inputs(ref, maps)
    for s, (H, e_out, n_out, n_hits, n_near) in ref.items():
        print('surface %d (%s, %s): %d hits, %d outside, %.0f %% of %d x %d bins filled' %
              (s, maps[s][0], fc.CLASS_OF[s], n_hits, n_out, 100. * (H > 0).mean(), H.shape[0], H.shape[1]))
        assert n_hits == o['hits'][s] > 0.02 * n
        assert N.isclose(H.sum() + e_out, o['absorbed'][s], rtol=1e-12)
        if s not in fc.CLIPPED:
            assert n_out == 0, s
    assert len(o['levels']) > 4


def test_the_scene_holds_what_the_device_tests_are_there_for():
    """every chart on some surface; a chart map on a surface of each shading class and on one that ends every ray; one plain XY map
    that is not the last; one map with x and y exchanged; a frustum on edges of the caller's; one clipped map; the two storage regimes
    either side of the streaming engine's byte limits (restated: 78 KiB for k_s_shade, 150 KiB for the lean kernels)"""
    import shade_cases as sc
    from tracer_amd.scene import compile_scene
    cs = compile_scene(fc.receivers()[0])
    maps = fc.maps('lds')
    assert set(m[0] for m in maps.values()) == set(fc.CHARTS)
    cls = {}
    for s in range(cs.n_surf):
        d = cs.descs[s]
        cls[s] = 'terminal' if sc.ends_every_ray(d) else {sc.CLS_MIRROR: 'mirror', sc.CLS_DIFFUSE: 'diffuse', sc.CLS_GENERAL: 'general'}[sc.shade_class_of(d)]
    assert cls == fc.CLASS_OF
    assert set(cls[s] for s, m in maps.items() if m[0] != 'xy') == {'terminal', 'mirror', 'diffuse', 'general'}
    assert maps[fc.WALL][0] == 'xy' and fc.WALL < max(maps)
    assert [s for s, m in maps.items() if m[1]] == [fc.FLOOR]
    assert cs.descs[fc.FRUSTUM].gm_kind == sc._kinds().GM_FRUSTUM and maps[fc.FRUSTUM][0] == 'cylinder'
    assert all(cs.capture[s] for s in maps)
    others = sum((len(u) - 1) * (len(v) - 1) for s, (_, _, u, v) in maps.items() if s != fc.FLOOR)
    assert others == fc.OTHER_BINS
    total = dict((k, (nu * nv + others) * 8 + 16) for k, (nu, nv) in fc.FLOOR_BINS.items())
    tables = 8 * 1024       # tallies, records, optics, edges, descriptors and flags of six surfaces: below this
    edges = dict((s, (u, v)) for s, (_, _, u, v) in fc.maps('global').items())
    S, n_edges = cs.n_surf, sum(len(u) + len(v) for u, v in edges.values())
    assert len(cs.extra) == 0       # (records of at most 32 doubles, trc_scene_create)
    assert (3 * S + 2) * 8 + S * 32 * 8 + 8 * S * 8 + n_edges * 8 + len(edges) * sc.SIZEOF_FLUXMAPDEV + 2 * S * 4 + 16 <= tables
    assert total['lds'] + tables <= 78 * 1024 and 150 * 1024 < total['global']
