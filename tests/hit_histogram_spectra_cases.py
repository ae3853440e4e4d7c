"""
What the tests of the spectral histogram of captured hits share (test_hit_histogram_spectra_host.py without a device,
test_gpu_hit_histogram_spectra.py on one): the host library, the restatement of where k_hist_hits_x keeps its bins
(trc_hit_hist_x_plan_for, trc_hithist.h) and the NumPy reference -- per sample numpy.histogram2d of a hit list with its spectra, or
a sum per surface.
"""
import ctypes as C
import os
import subprocess

import numpy as N

import hit_histogram_cases as hh

fc = hh.fc
LDS_WORDS = hh.LDS_BUDGET // 8

_f64, _i32, _i64 = hh._f64, hh._i32, hh._i64


def host_library():
    """tests/hostcheck/libtrc_hithist_x_check.so, built if need be"""
    subprocess.check_call(['make', '-s', '-C', hh.ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(hh.ROOT, 'tests', 'hostcheck', 'libtrc_hithist_x_check.so'))
    lib.hhx_lds_budget.restype = C.c_long
    lib.hhx_plan.argtypes = [C.c_int] * 4 + [_i64]
    lib.hhx_histogram.argtypes = [C.c_long, _i32, _f64, C.c_long, _f64] + [C.c_int] * 8 + [_f64] * 4 + [C.c_int, _f64, _i64, _f64, _i64]
    return lib


def library_plan(lib, nu, nv, W, counts):
    out = N.zeros(4, dtype=N.int64)
    lib.hhx_plan(nu, nv, W, int(counts), out.ctypes.data_as(_i64))
    return tuple(int(v) for v in out)


def plan(nu, nv, W, counts):
    """(in LDS, Ks, slices, LDS bytes), restated: a workgroup keeps the edges, nb x Ks bins, the count plane, Ks words of `outside`, the
    number outside and the off-grid count in 8192 doubles; Ks is the widest slice that fits, W at most.  When not one sample fits,
    the bins stay in global memory and the Ks + 2 words alone are in LDS."""
    nb = nu * nv
    fixed = (nu + 1) + (nv + 1) + (nb if counts else 0) + 2
    ks = 0
    while fixed + nb * (ks + 1) + (ks + 1) <= LDS_WORDS and ks < W:
        ks += 1
    if ks >= 1:
        return 1, ks, -(-W // ks), 8 * (fixed + nb * ks + ks)
    ks = min(W, LDS_WORDS - 2)
    return 0, ks, -(-W // ks), 8 * (ks + 2)


def sample_weights(weight, spectra, k):
    """(W, len(k)): what sample rows of the hits k add -- arrived - left, or arrived"""
    arrived, left = N.asarray(spectra[0])[:, k], N.asarray(spectra[1])[:, k]
    return arrived - left if weight == 'absorbed' else arrived


def reference(hits, lo, hi, chart, weight, proj, ue, ve, uv=None, skip=None):
    """dict(sum (nu, nv, W), count, outside (W,), outside_n, near, n) of the hits of surfaces lo..hi of a hit list with 'spectra' =
    (arrived, left, wavelengths), (W, m) each: numpy.histogram2d per sample with the NumPy chart formulas.  skip: a (W, m) mask of
    the samples left out."""
    surf = N.asarray(hits['surf'])
    k = N.nonzero((surf >= lo) & (surf <= hi))[0]
    if uv is not None:
        u, v = uv[0][k], uv[1][k]
    else:
        pts = N.asarray(hits['points'])[:, k]
        dirs = N.asarray(hits['directions'])[:, k] if chart not in fc.CHARTS else None
        u, v = hh.hit_uv(chart, proj, pts, dirs)
    w = sample_weights(weight, hits['spectra'], k)
    if skip is not None:
        w = N.where(skip[:, k], 0., w)
    bins = [N.asarray(ue, dtype=float), N.asarray(ve, dtype=float)]
    out = ~((u >= ue[0]) & (u <= ue[-1]) & (v >= ve[0]) & (v <= ve[-1]))
    total = N.stack([N.histogram2d(u, v, bins=bins, weights=w[j])[0] for j in range(len(w))], axis=-1)
    return dict(sum=total, count=N.histogram2d(u, v, bins=bins)[0].astype(N.int64), outside=w[:, out].sum(axis=1), outside_n=int(out.sum()),
                near=int((fc.near_edge(u, ue) | fc.near_edge(v, ve)).sum()), n=len(k))


def reference_by_surface(hits, lo, hi, weight, skip=None):
    """dict(sum (hi - lo + 1, W), count): the sum per surface"""
    surf = N.asarray(hits['surf'])
    W = len(hits['spectra'][0])
    total, count = N.zeros((hi - lo + 1, W)), N.zeros(hi - lo + 1, dtype=N.int64)
    for s in range(lo, hi + 1):
        k = N.nonzero(surf == s)[0]
        w = sample_weights(weight, hits['spectra'], k)
        if skip is not None:
            w = N.where(skip[:, k], 0., w)
        total[s - lo], count[s - lo] = w.sum(axis=1), len(k)
    return dict(sum=total, count=count)
