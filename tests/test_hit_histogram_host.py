"""
The histogram of captured hits without a device: the per-hit function of the core (trc_hit_hist_uv), the pass of k_hist_hits as a
plain host loop and the LDS decision of the kernel (trc_hithist.h), compiled for the host by `make hostcheck`
(tests/hostcheck/hithist_check.cpp), against the NumPy formulas of the charts, numpy.histogram2d and a restatement of the decision.

About 5 000 synthetic hits laid out like the hit buffer, under a general rotated projection rounded to 9 decimals (and under the
identity, where a direction along the axis has local x and y of exactly +-0): entries not written (surface -1), surfaces outside
the range, coordinates exactly on inner edges and on both outer edges, NaN and -0.0 coordinates, directions along +-z.
"""
import ctypes as C

import numpy as N
import pytest

import hit_histogram_cases as hh

fc = hh.fc
CHART_NO = dict((c, i) for i, c in enumerate(hh.CHARTS))
WEIGHT_NO = dict((w, i) for i, w in enumerate(hh.WEIGHTS))
N_HITS = 5000
LO, HI = 2, 4                 # the range of surfaces binned; the hits lie on surfaces -1..6


def _ptr(a, typ=hh._f64):
    return a.ctypes.data_as(typ)


@pytest.fixture(scope='module')
def lib():
    return hh.host_library()


def _projection(kind):
    from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
    if kind == 'identity':
        return N.eye(4)
    frame = N.dot(translate(3.1, -2.2, 0.7), N.dot(rotx(0.9), N.dot(roty(-0.3), rotz(2.1))))
    proj = fc.projection(frame)
    assert (N.abs(proj[:3, :3]) > 1e-3).all() and N.array_equal(proj, N.round(proj, 9))
    return proj


@pytest.fixture(scope='module', params=['general', 'identity'])
def hits(request, tmp_path_factory):
    """(proj, hit list, {chart: NumPy's (u, v) of every hit}): columns as the hit buffer holds them, the special entries first"""
    proj = _projection(request.param)
    rng = N.random.RandomState(17)
    n = N_HITS
    local = N.vstack((rng.uniform(-2., 2., (3, n)), N.ones(n)))
    pts = N.dot(N.linalg.inv(proj), local)[:3]
    d = rng.normal(size=(3, n))
    d /= N.sqrt((d * d).sum(axis=0))
    surf = rng.randint(-1, 7, size=n).astype(N.int32)
    e_in = rng.uniform(0.5, 2., n)
    e_abs = e_in * rng.uniform(0., 1., n)
    # the special entries, all on surfaces of the range
    d[:, 0], d[:, 1] = (0., 0., 1.), (0., 0., -1.)                  # directions along +-z
    d[:, 2], d[:, 3] = (-0., 1., 0.), (0., -0., -1.)                # -0.0 components
    d[:, 4] = (N.nan, 0.3, 0.4)                                     # a NaN direction
    pts[:, 5] = (N.nan, 1., 1.)                                     # a NaN point
    pts[:, 6], pts[:, 7] = (-0., -0., -0.), (0., -0., 1.)           # -0.0 coordinates
    surf[:8] = [2, 3, 4, 2, 3, 4, 2, 3]
    assert (surf == -1).sum() > 100 and ((surf >= 0) & (surf < LO)).sum() > 100 and (surf > HI).sum() > 100
    return proj, dict(surf=surf, e_abs=e_abs, e_in=e_in, points=pts, directions=d), \
        hh.numpy_uv_by_libm(proj, pts, d, tmp_path_factory.mktemp('uv'))


def _uv(lib, chart, proj, h):
    n = len(h['surf'])
    cols = [N.ascontiguousarray(c) for c in list(h['points']) + list(h['directions'])]
    u, v = N.empty(n), N.empty(n)
    lib.hh_uv(CHART_NO[chart], _ptr(N.ascontiguousarray(proj[:3].ravel())), n, *([_ptr(c) for c in cols] + [_ptr(u), _ptr(v)]))
    return u, v


def _same_bits(a, b):
    return N.array_equal(N.asarray(a).view(N.uint64), N.asarray(b).view(N.uint64)) or \
        N.array_equal(a, b, equal_nan=True) and N.array_equal(N.signbit(a), N.signbit(b))


@pytest.mark.parametrize('chart', hh.CHARTS)
def test_chart_coordinates_are_the_numpy_formulas_to_the_bit(lib, hits, chart):
    """The reference is hit_uv -- fluxmap_chart_scene.chart_uv and the two direction formulas -- evaluated by a NumPy that calls the C
    library's atan2 and acos (hit_histogram_cases.numpy_uv_by_libm says why); against this process's own NumPy, which may use its
    AVX512 loops, the difference is printed (one unit in the last place where this was written)."""
    proj, h, uv = hits
    u, v = _uv(lib, chart, proj, h)
    hu, hv = uv[chart]
    su, sv = hh.hit_uv(chart, proj, h['points'], h['directions'])
    print(chart, 'against this process\'s NumPy: %d of %d values differ, by at most %.3g' %
          (((u != su) & ~N.isnan(su)).sum() + ((v != sv) & ~N.isnan(sv)).sum(), 2 * len(u),
           max(N.nanmax(N.abs(u - su)), N.nanmax(N.abs(v - sv)))))
    bad = N.nonzero(~((u == hu) | (N.isnan(u) & N.isnan(hu))) | ~((v == hv) | (N.isnan(v) & N.isnan(hv))))[0]
    assert _same_bits(u, hu) and _same_bits(v, hv), (chart, bad[:10])
    if chart == 'dir_angles':
        ok = ~N.isnan(hu)
        assert hu[ok].min() >= 0. and hu[ok].max() <= N.pi / 2. and hv[ok].min() >= 0. and hv[ok].max() <= 2. * N.pi
        assert hu[0] == 0. and hu[1] == 0. or not N.array_equal(proj, N.eye(4))        # along the axis: the angle is exactly 0
        assert N.isnan(hu[4]) and N.isnan(u[4])


def _edges(c, n_bins, rng):
    """n_bins bins whose outer edges and every other inner edge are coordinates of the sample themselves (values at its 6th, 94th
    and intermediate percentiles): hits lie exactly on them, and a share of the hits outside"""
    c = N.sort(c[~N.isnan(c)])
    at = N.linspace(0.06, 0.94, n_bins + 1)
    e = c[(at * (len(c) - 1)).astype(int)].copy()
    mid = 0.5 * (e[:-1] + e[1:])
    e[1:-1:2] = mid[1::2][:len(e[1:-1:2])]          # the others between two sample values
    assert (N.diff(e) > 0).all()
    return e


def _run(lib, h, proj, chart, weight, ue, ve, moments, lo=LO, hi=HI):
    n = len(h['surf'])
    cols = N.ascontiguousarray(N.vstack([h['e_abs'], h['e_in']] + list(h['points']) + list(h['directions'])))
    nu, nv = len(ue) - 1, len(ve) - 1
    total, outside = N.full((nu, nv), 7.), N.full(2, 7.)            # (the outputs are overwritten)
    sq = N.full((nu, nv), 7.) if moments else None
    cnt = N.full((nu, nv), 7, dtype=N.int64) if moments else None
    null, nulli = hh._f64(), hh._i64()
    lib.hh_histogram(n, _ptr(N.ascontiguousarray(h['surf']), hh._i32), _ptr(cols), lo, hi, CHART_NO[chart], WEIGHT_NO[weight], nu, nv,
                     _ptr(N.ascontiguousarray(ue)), _ptr(N.ascontiguousarray(ve)), _ptr(N.ascontiguousarray(proj[:3].ravel())), _ptr(total),
                     _ptr(sq) if moments else null, _ptr(cnt, hh._i64) if moments else nulli, _ptr(outside))
    return total, sq, cnt, outside


@pytest.mark.parametrize('weight', hh.WEIGHTS)
@pytest.mark.parametrize('chart', hh.CHARTS)
def test_host_loop_is_histogram2d(lib, hits, chart, weight):
    """counts exact; sums within 1e-12 of the largest bin (only the order of the additions differs: n eps for n <= 5 000)"""
    proj, h, uv = hits
    sel = (h['surf'] >= LO) & (h['surf'] <= HI)
    u, v = uv[chart]
    rng = N.random.RandomState(3)
    ue, ve = _edges(u[sel], 9, rng), _edges(v[sel], 6, rng)
    # hits exactly on inner edges and on both outer edges, in u and in v
    for c, e in ((u[sel], ue), (v[sel], ve)):
        assert (c == e[0]).any() and (c == e[-1]).any() and N.isin(e[1:-1], c).sum() >= 2
    ref = hh.reference(h, LO, HI, chart, weight, proj, ue, ve, uv=uv[chart])
    assert 0.05 * ref['n'] < ref['outside'][1] < 0.6 * ref['n'] and ref['n'] == sel.sum() and (ref['count'] > 0).mean() > 0.8
    total, sq, cnt, outside = _run(lib, h, proj, chart, weight, ue, ve, True)
    assert N.array_equal(cnt, ref['count']) and outside[1] == ref['outside'][1]
    assert cnt.sum() + outside[1] == ref['n']
    for got, want in ((total, ref['sum']), (sq, ref['sum_sq']), (outside[0], ref['outside'][0])):
        assert N.abs(got - want).max() <= 1e-12 * max(N.abs(want).max(), 1e-300), (chart, weight, N.abs(got - want).max())
    if weight == 'count':
        assert N.array_equal(total, cnt) and N.array_equal(sq, cnt)
    # without the moment planes the sums are the same sums
    alone = _run(lib, h, proj, chart, weight, ue, ve, False)
    assert N.array_equal(alone[0], total) and N.array_equal(alone[3], outside)
    # one surface, and a range that holds none of the hits
    one = _run(lib, h, proj, chart, weight, ue, ve, True, 3, 3)
    assert N.array_equal(one[2], hh.reference(h, 3, 3, chart, weight, proj, ue, ve, uv=uv[chart])['count'])
    none = _run(lib, h, proj, chart, weight, ue, ve, True, 7, 9)
    assert not none[0].any() and not none[2].any() and not none[3].any()


def test_nan_coordinates_are_in_no_bin(lib, hits):
    proj, h, _ = hits
    few = dict((k, N.ascontiguousarray(v[..., :8])) for k, v in h.items())
    wide = N.array([-1e9, 0., 1e9])
    for chart, nan_at in (('xy', 5), ('dir_cosines', 4), ('dir_angles', 4)):
        ue = wide if chart != 'dir_angles' else N.array([0., 1., 2.])
        total, sq, cnt, outside = _run(lib, few, proj, chart, 'count', ue, N.array([-1e9, 1., 1e9]), True)
        assert cnt.sum() == 7 and outside[1] == 1, (chart, cnt, outside)


def test_lds_decision_is_the_restatement(lib):
    """edges, planes and the two words of `outside` in 64 KiB: at the budget, one bin beyond it, and over a grid of sizes"""
    assert lib.hh_lds_budget() == hh.LDS_BUDGET and lib.hh_n_charts() == len(hh.CHARTS)
    for nu in list(range(1, 40)) + [50, 64, 90, 128, 200, 431, 1000, 8000, 100000]:
        for nv in (1, 2, 16, 50, 51, 100, 430, 431, 8000):
            for planes in range(4):
                assert lib.hh_lds_bytes(nu, nv, planes) == hh.lds_bytes(nu, nv, planes)
                assert bool(lib.hh_in_lds(nu, nv, planes)) == hh.in_lds(nu, nv, planes), (nu, nv, planes)
    # (nu + 1)(nv + 1) = 8189 = 19 x 431 fills the budget to the byte with the sums alone
    assert hh.lds_bytes(18, 430, 0) == hh.LDS_BUDGET and lib.hh_in_lds(18, 430, 0) == 1
    assert lib.hh_in_lds(18, 431, 0) == 0 and lib.hh_in_lds(19, 430, 0) == 0 and lib.hh_in_lds(18, 430, 1) == 0
    # the receiver map of the NSTTF example fits with every plane
    assert lib.hh_in_lds(50, 50, 3) == 1 and hh.lds_bytes(50, 50, 3) == 60832


def test_the_binding_names_the_headers_numbers():
    import os
    from tracer_amd import _cabi
    header = open(os.path.join(hh.ROOT, 'include', 'tracer_amd.h')).read()
    assert 'TRC_HH_DIR_COSINES = 4, TRC_HH_DIR_ANGLES = 5' in header
    assert 'TRC_HH_ABSORBED = 0, TRC_HH_INCIDENT = 1, TRC_HH_COUNT = 2' in header
    assert [_cabi.HH_CHARTS[c] for c in hh.CHARTS] == list(range(6))
    assert [_cabi.HH_WEIGHTS[w] for w in hh.WEIGHTS] == [0, 1, 2]
    assert C.sizeof(_cabi.HitHistDesc) == 6 * 4 + 3 * 8


def test_engine_without_a_device_scene_says_so():
    from tracer_amd.tracer_engine import TracerEngine
    asm, objs, T = fc.receivers()
    with pytest.raises(ValueError, match='no device scene'):
        TracerEngine(asm).histogram_hits(fc.CYLINDER, [0., 1.], [0., 1.])
