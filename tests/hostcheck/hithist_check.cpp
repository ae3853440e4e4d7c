// hithist_check.cpp -- TEST-ONLY host build of the histogram of captured hits (tracer_amd/csrc/trc_core.h: trc_hit_hist_uv;
// trc_hithist.h: the LDS decision of k_hist_hits, its per-entry function and its pass as a plain loop).  Built by `make hostcheck`
// into tests/hostcheck/, loaded only by tests/test_hit_histogram_host.py; not a product path.
#include "../../tracer_amd/csrc/trc_hithist.h"

extern "C" {

int hh_n_charts(void) { return TRC_HH_CHARTS; }
long hh_lds_budget(void) { return TRC_HH_LDS_BUDGET; }
long hh_lds_bytes(int nu, int nv, int planes) { return (long)trc_hit_hist_lds_bytes(nu, nv, planes); }
int hh_in_lds(int nu, int nv, int planes) { return trc_hit_hist_in_lds(nu, nv, planes) ? 1 : 0; }

// (u, v)[k] of hit k (point p, incident direction d) in `chart` through proj12
void hh_uv(int chart, const double *proj12, long m, const double *px, const double *py, const double *pz, const double *dx, const double *dy,
           const double *dz, double *u, double *v) {
    for (long k = 0; k < m; ++k) trc_hit_hist_uv(chart, proj12, px[k], py[k], pz[k], dx[k], dy[k], dz[k], &u[k], &v[k]);
}

// the pass of k_hist_hits over m entries laid out like the hit buffer: cols = e_abs | e_in | px | py | pz | dx | dy | dz, m each.
// sum, sum_sq, count (nu * nv) and outside (2) are overwritten; sum_sq and count may be NULL.
void hh_histogram(long m, const int32_t *surf, const double *cols, int surf_lo, int surf_hi, int chart, int weight, int nu, int nv,
                  const double *u_edges, const double *v_edges, const double *proj12, double *sum, double *sum_sq, long long *count,
                  double *outside) {
    trc_hit_hist_args A = {};
    A.n = m; A.surf = surf;
    A.e_abs = cols; A.e_in = cols + m; A.px = cols + 2 * m; A.py = cols + 3 * m; A.pz = cols + 4 * m;
    A.dx = cols + 5 * m; A.dy = cols + 6 * m; A.dz = cols + 7 * m;
    A.surf_lo = surf_lo; A.surf_hi = surf_hi; A.chart = chart; A.weight = weight; A.nu = nu; A.nv = nv;
    A.planes = (sum_sq ? TRC_HH_PLANE_SUM_SQ : 0) | (count ? TRC_HH_PLANE_COUNT : 0);
    for (int k = 0; k < 12; ++k) A.proj[k] = proj12[k];
    double *edges = new double[nu + nv + 2];
    for (int k = 0; k <= nu; ++k) edges[k] = u_edges[k];
    for (int k = 0; k <= nv; ++k) edges[nu + 1 + k] = v_edges[k];
    A.edges = edges;
    A.sum = sum; A.sum_sq = sum_sq; A.count = (unsigned long long *)count; A.outside = outside;
    for (long k = 0; k < (long)nu * nv; ++k) { sum[k] = 0.0; if (sum_sq) sum_sq[k] = 0.0; if (count) count[k] = 0; }
    outside[0] = outside[1] = 0.0;
    trc_hit_hist_host(A);
    delete[] edges;
}

}
