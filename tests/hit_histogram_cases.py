"""
What the tests of the histogram of captured hits share (test_hit_histogram_host.py without a device, test_gpu_hit_histogram.py on
one): the NumPy formulas of the six charts, the host reference -- numpy.histogram2d of a hit list -- and the restatement of
k_hist_hits' LDS decision (trc_hithist.h).
"""
import ctypes as C
import os
import subprocess

import numpy as N

import fluxmap_chart_scene as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARTS = fc.CHARTS + ('dir_cosines', 'dir_angles')           # the library's numbers 0..5
WEIGHTS = ('absorbed', 'incident', 'count')                  # 0..2
PLANE_SUM_SQ, PLANE_COUNT = 1, 2
LDS_BUDGET = 64 * 1024

_f64 = C.POINTER(C.c_double)
_i32 = C.POINTER(C.c_int32)
_i64 = C.POINTER(C.c_longlong)


def host_library():
    """tests/hostcheck/libtrc_hithist_check.so, built if need be"""
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_hithist_check.so'))
    lib.hh_lds_budget.restype = C.c_long
    lib.hh_lds_bytes.restype = C.c_long
    lib.hh_lds_bytes.argtypes = [C.c_int] * 3
    lib.hh_in_lds.argtypes = [C.c_int] * 3
    lib.hh_uv.argtypes = [C.c_int, _f64, C.c_long] + [_f64] * 8
    lib.hh_histogram.argtypes = [C.c_long, _i32, _f64] + [C.c_int] * 6 + [_f64] * 5 + [_i64, _f64]
    return lib


def lds_bytes(nu, nv, planes):
    """the restatement: edges, one float64 plane of sums, one 8-byte plane more per moment, the two words of `outside`"""
    n_planes = 1 + bool(planes & PLANE_SUM_SQ) + bool(planes & PLANE_COUNT)
    return 8 * ((nu + 1) + (nv + 1) + nu * nv * n_planes + 2)


def in_lds(nu, nv, planes):
    return lds_bytes(nu, nv, planes) <= LDS_BUDGET


def direction_uv(chart, proj, directions):
    """(u, v) of incident directions (3, n) in the two direction charts: the rows of proj without the translation column, products
    and sums in the order the library takes them"""
    dx, dy, dz = N.asarray(directions, dtype=float)
    dxl = (proj[0, 0] * dx + proj[0, 1] * dy) + proj[0, 2] * dz
    dyl = (proj[1, 0] * dx + proj[1, 1] * dy) + proj[1, 2] * dz
    if chart == 'dir_cosines':
        return dxl, dyl
    assert chart == 'dir_angles'
    dzl = (proj[2, 0] * dx + proj[2, 1] * dy) + proj[2, 2] * dz
    phi = N.arctan2(-dyl, -dxl)
    phi[phi < 0.] += 2. * N.pi
    with N.errstate(invalid='ignore', divide='ignore'):
        return N.arccos(N.abs(dzl) / N.sqrt((dxl * dxl + dyl * dyl) + dzl * dzl)), phi


def hit_uv(chart, proj, points, directions):
    return fc.chart_uv(chart, proj, points) if chart in fc.CHARTS else direction_uv(chart, proj, directions)


def _dispatched_simd():
    """the SIMD features this NumPy may dispatch its loops to on this machine"""
    try:
        from numpy._core import _multiarray_umath as um
    except ImportError:         # NumPy 1
        from numpy.core import _multiarray_umath as um
    return [f for f in um.__cpu_dispatch__ if um.__cpu_features__.get(f)]


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as N
import hit_histogram_cases as hh
d = N.load(sys.argv[1])
out = {}
for c in hh.CHARTS:
    out[c + '_u'], out[c + '_v'] = hh.hit_uv(c, d['proj'], d['points'], d['directions'])
N.savez(sys.argv[2], **out)
"""


def numpy_uv_by_libm(proj, points, directions, tmpdir):
    """
    {chart: (u, v)} of hit_uv -- the same NumPy formulas, run by NumPy -- in a child process whose NumPy has its SIMD loops
    switched off (NPY_DISABLE_CPU_FEATURES, read when NumPy is imported).  Where NumPy dispatches arctan2 and arccos to its
    AVX512 loops they differ from the C library's by one unit in the last place in about 5 % of the values; with the loops off NumPy
    calls the C library, the one the host build of the core calls, and equality to the bit is a statement about the formulas --
    the order of their products and sums, the wrap of the azimuth, the signs -- and not about two implementations of atan2.
    """
    import sys
    src, dst = os.path.join(str(tmpdir), 'hits.npz'), os.path.join(str(tmpdir), 'uv.npz')
    N.savez(src, proj=proj, points=points, directions=directions)
    env = dict(os.environ)
    off = _dispatched_simd()
    if off:
        env['NPY_DISABLE_CPU_FEATURES'] = ' '.join(off)
    subprocess.check_call([sys.executable, '-c', _CHILD % (os.path.join(ROOT, 'tests'), ROOT), src, dst], env=env)
    d = N.load(dst)
    return dict((c, (d[c + '_u'], d[c + '_v'])) for c in CHARTS)


def weights_of(weight, hits, k):
    if weight == 'count':
        return N.ones(len(k))
    return N.asarray(hits['e_abs' if weight == 'absorbed' else 'e_in'])[k]


def reference(hits, lo, hi, chart, weight, proj, ue, ve, uv=None):
    """dict(sum, sum_sq, count, outside, near, n) of the hits of surfaces lo..hi of a hit list dict(surf, e_abs, e_in, points,
    directions): numpy.histogram2d with the NumPy chart formulas (uv: their values for every hit of the list, where the caller
    has them); near: selected hits within EDGE_EPS of an edge"""
    surf = N.asarray(hits['surf'])
    k = N.nonzero((surf >= lo) & (surf <= hi))[0]
    if uv is not None:
        u, v = uv[0][k], uv[1][k]
    else:
        pts = N.asarray(hits['points'])[:, k]
        dirs = N.asarray(hits['directions'])[:, k] if chart not in fc.CHARTS else None
        u, v = hit_uv(chart, proj, pts, dirs)
    w = weights_of(weight, hits, k)
    bins = [N.asarray(ue, dtype=float), N.asarray(ve, dtype=float)]
    out = ~((u >= ue[0]) & (u <= ue[-1]) & (v >= ve[0]) & (v <= ve[-1]))
    return dict(sum=N.histogram2d(u, v, bins=bins, weights=w)[0], sum_sq=N.histogram2d(u, v, bins=bins, weights=w * w)[0],
                count=N.histogram2d(u, v, bins=bins)[0].astype(N.int64), outside=(w[out].sum(), int(out.sum())),
                near=int((fc.near_edge(u, ue) | fc.near_edge(v, ve)).sum()), n=len(k))
