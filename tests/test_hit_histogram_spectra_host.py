"""
The spectral histogram of captured hits without a device: the pass of k_hist_hits_x as a plain host loop over the per-entry code the
kernel runs, slice by slice, and the decision where the kernel keeps its bins (trc_hithist.h), compiled for the host by
`make hostcheck` (tests/hostcheck/hithist_x_check.cpp), against per-sample numpy.histogram2d, per-surface sums and a restatement of
the decision.

About 5 000 synthetic hits laid out like the hit buffer under a general rotated projection, as test_hit_histogram_host.py builds its
own: entries not written (surface -1), surfaces outside the range, coordinates exactly on inner edges and on both outer edges, NaN
and -0.0 coordinates -- with W in {1, 2, 5} samples in 3 W spectral columns whose stride is larger than the number of entries (what
lies behind the entries is NaN).
"""
import ctypes as C

import numpy as N
import pytest

import hit_histogram_spectra_cases as hx
from test_hit_histogram_host import _projection, _edges, CHART_NO, WEIGHT_NO, N_HITS, LO, HI

hh, fc = hx.hh, hx.fc
SLACK = 123                     # entries of the columns' stride behind the last hit
WS = (1, 2, 5)
CHARTS = ('cylinder', 'dir_angles')         # one chart of the hit point, one of the direction


def _ptr(a, typ=hh._f64):
    return a.ctypes.data_as(typ) if a is not None else typ()


@pytest.fixture(scope='module')
def lib():
    return hx.host_library()


@pytest.fixture(scope='module')
def hits(tmp_path_factory):
    """(proj, hit list with spectra of the largest W, {chart: NumPy's (u, v) of every hit}); the special entries first"""
    proj = _projection('general')
    rng = N.random.RandomState(29)
    n = N_HITS
    local = N.vstack((rng.uniform(-2., 2., (3, n)), N.ones(n)))
    pts = N.dot(N.linalg.inv(proj), local)[:3]
    d = rng.normal(size=(3, n))
    d /= N.sqrt((d * d).sum(axis=0))
    surf = rng.randint(-1, 7, size=n).astype(N.int32)
    e_in = rng.uniform(0.5, 2., n)
    e_abs = e_in * rng.uniform(0., 1., n)
    d[:, 0], d[:, 1] = (0., 0., 1.), (0., 0., -1.)
    d[:, 2], d[:, 3] = (-0., 1., 0.), (0., -0., -1.)
    d[:, 4] = (N.nan, 0.3, 0.4)
    pts[:, 5] = (N.nan, 1., 1.)
    pts[:, 6], pts[:, 7] = (-0., -0., -0.), (0., -0., 1.)
    surf[:8] = [2, 3, 4, 2, 3, 4, 2, 3]
    assert (surf == -1).sum() > 100 and ((surf >= 0) & (surf < LO)).sum() > 100 and (surf > HI).sum() > 100
    W = max(WS)
    arrived = rng.uniform(0.5, 2., (W, n))
    left = arrived * rng.uniform(0., 1., (W, n))
    wl = N.tile(N.linspace(0.3e-6, 2.5e-6, W)[:, None], (1, n))
    h = dict(surf=surf, e_abs=e_abs, e_in=e_in, points=pts, directions=d, spectra=(arrived, left, wl))
    return proj, h, hh.numpy_uv_by_libm(proj, pts, d, tmp_path_factory.mktemp('uv'))


def _cut(h, W):
    """the hit list with its first W samples"""
    return dict(h, spectra=tuple(c[:W] for c in h['spectra']))


def _run(lib, h, proj, chart, weight, ue, ve, counts=True, by_surface=False, wl=None, ks=0, lo=LO, hi=HI):
    """(sum, count, outside (W,), outside_n, off_grid) of hhx_histogram over the hit list laid out like the buffer"""
    n = len(h['surf'])
    arrived, left, swl = h['spectra']
    W, cap = len(arrived), n + SLACK
    x = N.full((3 * W, cap), N.nan)
    x[:W, :n], x[W:2 * W, :n], x[2 * W:, :n] = swl, arrived, left
    cols = N.ascontiguousarray(N.vstack([h['e_abs'], h['e_in']] + list(h['points']) + list(h['directions'])))
    nu, nv = (hi - lo + 1, 1) if by_surface else (len(ue) - 1, len(ve) - 1)
    total, outside = N.full((nu, nv, W), 7.), N.full(W + 1, 7.)           # (the outputs are overwritten)
    cnt = N.full((nu, nv), 7, dtype=N.int64) if counts else None
    off = C.c_longlong(7)
    f = lambda a: None if a is None else N.ascontiguousarray(a, dtype=float)
    ue, ve, p, wl = f(ue), f(ve), None if by_surface else f(proj[:3].ravel()), f(wl)
    lib.hhx_histogram(n, _ptr(N.ascontiguousarray(h['surf']), hh._i32), _ptr(cols), cap, _ptr(x), W, lo, hi, 0 if by_surface else CHART_NO[chart],
                      WEIGHT_NO[weight], int(by_surface), nu, nv, _ptr(ue), _ptr(ve), _ptr(p), _ptr(wl), ks, _ptr(total), _ptr(cnt, hh._i64),
                      _ptr(outside), C.byref(off))
    return total, cnt, outside[:W], outside[W], off.value


def _same(a, b):
    return all(N.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('weight', ['absorbed', 'incident'])
@pytest.mark.parametrize('chart', CHARTS)
@pytest.mark.parametrize('W', WS)
def test_host_loop_is_histogram2d_per_sample(lib, hits, W, chart, weight):
    """counts exact; sums within 1e-12 of the largest bin (only the order of the additions differs: n eps for n <= 5 000); evaluated in
    slices of 1, 2 and W samples the result is the unsliced one to the bit"""
    proj, h, uv = hits
    h = _cut(h, W)
    sel = (h['surf'] >= LO) & (h['surf'] <= HI)
    u, v = uv[chart]
    rng = N.random.RandomState(3)
    ue, ve = _edges(u[sel], 9, rng), _edges(v[sel], 6, rng)
    for c, e in ((u[sel], ue), (v[sel], ve)):       # hits exactly on inner edges and on both outer edges, in u and in v
        assert (c == e[0]).any() and (c == e[-1]).any() and N.isin(e[1:-1], c).sum() >= 2
    ref = hx.reference(h, LO, HI, chart, weight, proj, ue, ve, uv=uv[chart])
    assert 0.05 * ref['n'] < ref['outside_n'] < 0.6 * ref['n'] and ref['n'] == sel.sum() and (ref['count'] > 0).mean() > 0.8
    got = _run(lib, h, proj, chart, weight, ue, ve)
    total, cnt, outside, outside_n, off = got
    assert N.array_equal(cnt, ref['count']) and outside_n == ref['outside_n'] and off == 0
    assert cnt.sum() + outside_n == ref['n'] and total.shape == (9, 6, W)
    for mine, want in ((total, ref['sum']), (outside, ref['outside'])):
        assert N.abs(mine - want).max() <= 1e-12 * N.abs(ref['sum']).max(), (W, chart, weight, N.abs(mine - want).max())
    if weight == 'absorbed':
        assert not N.allclose(total, hx.reference(h, LO, HI, chart, 'incident', proj, ue, ve, uv=uv[chart])['sum'])
    # slice by slice: every sample's additions happen in the same order
    for ks in (1, 2, W):
        assert _same(_run(lib, h, proj, chart, weight, ue, ve, ks=ks), got), (W, ks)
    # without the count plane the sums are the same sums; with the grid the hits are on, nothing is off it
    alone = _run(lib, h, proj, chart, weight, ue, ve, counts=False)
    assert alone[1] is None and N.array_equal(alone[0], total) and N.array_equal(alone[2], outside) and alone[3] == outside_n
    assert _same(_run(lib, h, proj, chart, weight, ue, ve, wl=h['spectra'][2][:, 0]), got)
    # one surface, and a range that holds none of the hits
    one = _run(lib, h, proj, chart, weight, ue, ve, lo=3, hi=3)
    assert N.array_equal(one[1], hx.reference(h, 3, 3, chart, weight, proj, ue, ve, uv=uv[chart])['count'])
    none = _run(lib, h, proj, chart, weight, ue, ve, lo=7, hi=9)
    assert not none[0].any() and not none[1].any() and not none[2].any() and none[3] == 0 and none[4] == 0


@pytest.mark.parametrize('weight', ['absorbed', 'incident'])
@pytest.mark.parametrize('W', WS)
def test_by_surface_is_a_sum_per_surface(lib, hits, W, weight):
    proj, h, uv = hits
    h = _cut(h, W)
    for lo, hi in ((LO, HI), (0, 6), (3, 3)):
        ref = hx.reference_by_surface(h, lo, hi, weight)
        got = _run(lib, h, proj, None, weight, None, None, by_surface=True, lo=lo, hi=hi)
        total, cnt, outside, outside_n, off = got
        assert total.shape == (hi - lo + 1, 1, W) and N.array_equal(cnt[:, 0], ref['count']) and cnt.sum() > 0
        assert N.abs(total[:, 0] - ref['sum']).max() <= 1e-12 * ref['sum'].max(), (W, weight, lo, hi)
        assert not outside.any() and outside_n == 0 and off == 0
        for ks in (1, 2, W):
            assert _same(_run(lib, h, proj, None, weight, None, None, by_surface=True, lo=lo, hi=hi, ks=ks), got)


@pytest.mark.parametrize('W', WS)
def test_samples_off_the_grid_are_counted_and_left_out(lib, hits, W):
    """37 selected hits moved off the grid in one sample each: off_grid is 37 and exactly those samples are missing from the sums --
    by chart (some of them outside) and by surface, whole and in slices; without a grid they are binned like the others"""
    proj, h, uv = hits
    h = _cut(h, W)
    n = len(h['surf'])
    rng = N.random.RandomState(5)
    sel = N.nonzero((h['surf'] >= LO) & (h['surf'] <= HI))[0]
    moved = rng.choice(sel, 37, replace=False)
    which = rng.randint(0, W, 37)
    swl = h['spectra'][2].copy()
    grid = swl[:, 0].copy()
    swl[which, moved] *= 1. + 1e-15 * rng.choice([-4, 4, 1e12], 37)        # a few units in the last place, or far off
    swl[which[0], moved[0]] = N.nan
    skip = N.zeros((W, n), dtype=bool)
    skip[which, moved] = True
    assert skip.sum() == 37 and (swl[skip] != N.tile(grid[:, None], (1, n))[skip]).all()
    h = dict(h, spectra=(h['spectra'][0], h['spectra'][1], swl))
    u, v = uv['cylinder']
    r3 = N.random.RandomState(3)
    ue, ve = _edges(u[sel], 9, r3), _edges(v[sel], 6, r3)
    ref = hx.reference(h, LO, HI, 'cylinder', 'absorbed', proj, ue, ve, uv=uv['cylinder'], skip=skip)
    full = hx.reference(h, LO, HI, 'cylinder', 'absorbed', proj, ue, ve, uv=uv['cylinder'])
    got = _run(lib, h, proj, 'cylinder', 'absorbed', ue, ve, wl=grid)
    total, cnt, outside, outside_n, off = got
    assert off == 37 and N.array_equal(cnt, full['count']) and outside_n == full['outside_n']       # (the hits are counted all the same)
    scale = N.abs(full['sum']).max()
    assert N.abs(total - ref['sum']).max() <= 1e-12 * scale and N.abs(outside - ref['outside']).max() <= 1e-12 * scale
    missing = (full['sum'] - ref['sum']).sum() + (full['outside'] - ref['outside']).sum()
    assert missing > 0 and N.isclose((full['sum'].sum() + full['outside'].sum()) - (total.sum() + outside.sum()), missing, rtol=1e-9)
    for ks in (1, 2, W):
        assert _same(_run(lib, h, proj, 'cylinder', 'absorbed', ue, ve, wl=grid, ks=ks), got)
    loose = _run(lib, h, proj, 'cylinder', 'absorbed', ue, ve, wl=None)
    assert loose[4] == 0 and N.abs(loose[0] - full['sum']).max() <= 1e-12 * scale
    by = _run(lib, h, proj, None, 'incident', None, None, by_surface=True, wl=grid)
    want = hx.reference_by_surface(h, LO, HI, 'incident', skip=skip)
    assert by[4] == 37 and N.array_equal(by[1][:, 0], want['count']) and N.abs(by[0][:, 0] - want['sum']).max() <= 1e-12 * want['sum'].max()


PLAN_POINTS = [                                        # (nu, nv, W, counts) -> (in LDS, Ks, slices)
    ((1, 1, 1, False), (1, 1, 1)), ((4, 5, 1, True), (1, 1, 1)), ((100, 100, 1, False), (0, 1, 1)),
    ((1, 6, 7, False), (1, 7, 1)), ((1, 6, 7, True), (1, 7, 1)),                  # fits whole
    ((40, 40, 7, False), (1, 5, 2)), ((40, 40, 7, True), (1, 4, 2)),              # 5 + 2, 4 + 3: a partial last slice
    ((50, 50, 20, False), (1, 3, 7)), ((50, 50, 20, True), (1, 2, 10)),
    ((100, 100, 3, False), (0, 3, 1)), ((100, 100, 3, True), (0, 3, 1)),          # the global form
]


def test_the_plan_is_the_restatement(lib):
    assert lib.hhx_lds_budget() == hh.LDS_BUDGET == 8 * hx.LDS_WORDS
    for args, (in_lds, ks, slices) in PLAN_POINTS:
        got = hx.library_plan(lib, *args)
        assert got == hx.plan(*args) and got[:3] == (in_lds, ks, slices), (args, got)
        assert got[3] <= hh.LDS_BUDGET and (got[2] - 1) * got[1] < args[2] <= got[2] * got[1]
    # 40 x 40 with 7 samples in words: edges 82, bins 1600 Ks, Ks + 2 of `outside`; the count plane 1600 more
    assert hx.plan(40, 40, 7, False)[3] == 8 * (82 + 1600 * 5 + 5 + 2) and hx.plan(40, 40, 7, True)[3] == 8 * (82 + 1600 * 4 + 1600 + 4 + 2)
    # exactly at the budget: edges 2 + 4094, bins 4093, 1 + 2 of `outside` = 8192 words hold one sample of 1 x 4093 bins; one bin
    # more and none fits: the bins in global memory, the 3 + 2 words of `outside` in LDS
    assert hx.library_plan(lib, 1, 4093, 3, False) == (1, 1, 3, hh.LDS_BUDGET)
    assert hx.library_plan(lib, 1, 4094, 3, False) == (0, 3, 1, 8 * 5)
    # ... and with the count plane: 1 x 2728 is 2 + 2729 + 2728 + 2728 + 1 + 2 = 8190 words, 1 x 2729 is 8193
    assert hx.library_plan(lib, 1, 2728, 2, True) == (1, 1, 2, 8 * 8190) and hx.library_plan(lib, 1, 2729, 2, True)[:3] == (0, 2, 1)
    # 3 x 1023: edges 4 + 1024, 3070 Ks + 2 <= 7164 -> two samples a slice, the last slice one
    assert hx.library_plan(lib, 3, 1023, 5, False)[:3] == (1, 2, 3)
    for nu in list(range(1, 24)) + [40, 50, 64, 90, 128, 431, 1000, 4092, 4093, 8000, 100000]:
        for nv in (1, 2, 16, 50, 51, 100, 430):
            for W in (1, 2, 3, 7, 20, 4096):
                for counts in (False, True):
                    assert hx.library_plan(lib, nu, nv, W, counts) == hx.plan(nu, nv, W, counts), (nu, nv, W, counts)


def test_the_binding_names_the_headers_struct():
    import os
    from tracer_amd import _cabi
    header = open(os.path.join(hh.ROOT, 'include', 'tracer_amd.h')).read()
    assert 'typedef struct trc_hit_hist_x_desc {' in header and 'trc_scene_histogram_hits_x' in _cabi.SIGNATURES
    assert [f[0] for f in _cabi.HitHistXDesc._fields_] == ['base', 'n_samples', 'by_surface', 'wl']
    assert C.sizeof(_cabi.HitHistXDesc) == C.sizeof(_cabi.HitHistDesc) + 2 * 4 + 8 and C.sizeof(_cabi.HitHistDesc) == 6 * 4 + 3 * 8


def test_engine_without_a_device_scene_says_so():
    from tracer_amd.tracer_engine import TracerEngine
    asm, objs, T = fc.receivers()
    eng = TracerEngine(asm)
    with pytest.raises(ValueError, match='no device scene'):
        eng.histogram_spectra(fc.CYLINDER, [0., 1.], [0., 1.])
    with pytest.raises(ValueError, match='no device scene'):
        eng.surface_spectra()


def test_integrate_is_the_trapezoid_rule_and_needs_the_wavelengths():
    from tracer_amd.scene import SpectralHistogram
    wl = N.array([1., 2., 4.])
    H = SpectralHistogram(wl, N.array([[1., 3., 1.], [0., 0., 2.]]), None, N.zeros(3), 0, 0)
    assert N.array_equal(H.integrate(), [2. + 4., 2.])
    with pytest.raises(ValueError, match='without wavelengths'):
        SpectralHistogram(None, N.zeros((2, 3)), None, N.zeros(3), 0, 0).integrate()
