// trc_hithist.h -- the histogram of captured hits (trc_scene_histogram_hits, k_hist_hits in trc_hithist.hip): what the kernel is
// handed, where it keeps its bins, what it does per entry of the hit buffer, and the same pass as a plain host loop.  No device code:
// tests/hostcheck compiles this header with g++ (hithist_check.cpp) and holds the restatements of tests/test_hit_histogram_host.py
// to it.
#ifndef TRC_HITHIST_H
#define TRC_HITHIST_H

#include "trc_core.h"

#define TRC_HH_PLANE_SUM_SQ 0x1     /* planes beside the sum of the weights: their squares ... */
#define TRC_HH_PLANE_COUNT 0x2      /* ... and the hits of every bin */

// One pass over entries [0, n) of the hit buffer's columns.  Entries of a surface outside [surf_lo, surf_hi] -- the -1 of an entry
// not written among them: surf_lo is never negative -- are passed over after their surface has been read.
struct trc_hit_hist_args {
    long long n;
    const int32_t *surf;
    const double *e_abs, *e_in, *px, *py, *pz, *dx, *dy, *dz;
    int32_t surf_lo, surf_hi, chart, weight, nu, nv, planes;
    double proj[12];
    const double *edges;            // u_edges[nu + 1] | v_edges[nv + 1]
    double *sum, *sum_sq;           // nu * nv each, row-major u (sum_sq, count: with their plane bits)
    unsigned long long *count;
    double *outside;                // weight and number of the selected hits in no bin
};

// The workgroups of k_hist_hits keep a private copy of the edges, the planes and the two words of `outside` in LDS while all of it
// fits TRC_HH_LDS_BUDGET, and add to the planes in global memory beyond.  64 KiB: what a kernel gets without being allowed more,
// and what leaves two workgroups on a CU's 160 KiB -- the pass is bound by the loads of the columns, and a workgroup alone on its CU
// has 4 waves to hide them behind.  The 50 x 50 map of the NSTTF receiver with both moment planes is 60 832 bytes.  Count bins are
// 64-bit in LDS too: one rule for every plane.
#define TRC_HH_LDS_BUDGET (64 * 1024)
TRC_HD int trc_hit_hist_n_planes(int planes) { return 1 + ((planes & TRC_HH_PLANE_SUM_SQ) ? 1 : 0) + ((planes & TRC_HH_PLANE_COUNT) ? 1 : 0); }
TRC_HD long long trc_hit_hist_lds_bytes(int nu, int nv, int planes) {
    return 8ll * ((long long)(nu + 1) + (nv + 1) + (long long)nu * nv * trc_hit_hist_n_planes(planes) + 2);
}
TRC_HD bool trc_hit_hist_in_lds(int nu, int nv, int planes) { return trc_hit_hist_lds_bytes(nu, nv, planes) <= TRC_HH_LDS_BUDGET; }

// The weight of entry i and its bin iu * nv + iv on the edges ue, ve (-1: in no bin).  Reads the columns the chart and the weight
// need and no others: the hit point or the direction, and one energy or none.
TRC_HD int trc_hit_hist_entry(const trc_hit_hist_args &A, const double *ue, const double *ve, long long i, double *w) {
    double px = 0.0, py = 0.0, pz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0, u, v;
    if (TRC_HH_IS_DIR(A.chart)) { dx = A.dx[i]; dy = A.dy[i]; dz = A.dz[i]; }
    else { px = A.px[i]; py = A.py[i]; pz = A.pz[i]; }
    *w = A.weight == TRC_HH_ABSORBED ? A.e_abs[i] : A.weight == TRC_HH_INCIDENT ? A.e_in[i] : 1.0;
    trc_hit_hist_uv(A.chart, A.proj, px, py, pz, dx, dy, dz, &u, &v);
    const int iu = trc_bin_index(ue, A.nu, u), iv = trc_bin_index(ve, A.nv, v);
    return (iu >= 0 && iv >= 0) ? iu * A.nv + iv : -1;
}

// the pass on the host, over host arrays: the planes and `outside` are added to
static inline void trc_hit_hist_host(const trc_hit_hist_args &A) {
    const double *ue = A.edges, *ve = A.edges + A.nu + 1;
    for (long long i = 0; i < A.n; ++i) {
        const int32_t s = A.surf[i];
        if (s < 0 || s < A.surf_lo || s > A.surf_hi) continue;
        double w;
        const int b = trc_hit_hist_entry(A, ue, ve, i, &w);
        if (b < 0) { A.outside[0] += w; A.outside[1] += 1.0; continue; }
        A.sum[b] += w;
        if (A.planes & TRC_HH_PLANE_SUM_SQ) A.sum_sq[b] += w * w;
        if (A.planes & TRC_HH_PLANE_COUNT) A.count[b] += 1;
    }
}

#ifdef __HIPCC__
// k_hist_hits over A on `stream` (trc_hithist.hip): the planes and `outside` on the device are added to.  The grid is k_bin_hits'.
hipError_t trc_hit_hist_launch(hipStream_t stream, int n_cu, const trc_hit_hist_args &A);
#endif

#endif  // TRC_HITHIST_H
