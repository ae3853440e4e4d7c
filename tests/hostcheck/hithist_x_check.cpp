// hithist_x_check.cpp -- TEST-ONLY host build of the spectral histogram of captured hits (tracer_amd/csrc/trc_hithist.h: where
// k_hist_hits_x keeps its bins -- trc_hit_hist_x_plan_for -- and its pass as a plain loop, slice by slice, over the per-entry code the
// kernel runs).  Built by `make hostcheck` into tests/hostcheck/, loaded only by tests/test_hit_histogram_spectra_host.py; not a
// product path.
#include "../../tracer_amd/csrc/trc_hithist.h"

extern "C" {

long hhx_lds_budget(void) { return TRC_HH_LDS_BUDGET; }

// out4 = in_lds, Ks, n_slices, lds_bytes
void hhx_plan(int nu, int nv, int W, int counts, long long *out4) {
    const trc_hit_hist_x_plan p = trc_hit_hist_x_plan_for(nu, nv, W, counts != 0);
    out4[0] = p.in_lds; out4[1] = p.Ks; out4[2] = p.n_slices; out4[3] = p.lds_bytes;
}

// The pass over m entries laid out like the hit buffer: cols = e_abs | e_in | px | py | pz | dx | dy | dz, m each; x = the 3 W spectral
// columns at stride cap >= m.  ks: the width of the slices the pass is evaluated in, one after the other (0: unsliced).  sum (bins x W),
// count (bins; may be NULL), outside (W + 1) and off_grid are overwritten; by_surface: bins = surf_hi - surf_lo + 1, no edges read.
void hhx_histogram(long m, const int32_t *surf, const double *cols, long cap, const double *x, int W, int surf_lo, int surf_hi, int chart,
                   int weight, int by_surface, int nu, int nv, const double *u_edges, const double *v_edges, const double *proj12,
                   const double *wl, int ks, double *sum, long long *count, double *outside, long long *off_grid) {
    trc_hit_hist_x_args X = {};
    trc_hit_hist_args &A = X.h;
    if (by_surface) { nu = surf_hi - surf_lo + 1; nv = 1; }
    A.n = m; A.surf = surf;
    A.e_abs = cols; A.e_in = cols + m; A.px = cols + 2 * m; A.py = cols + 3 * m; A.pz = cols + 4 * m;
    A.dx = cols + 5 * m; A.dy = cols + 6 * m; A.dz = cols + 7 * m;
    A.surf_lo = surf_lo; A.surf_hi = surf_hi; A.chart = chart; A.weight = weight; A.nu = nu; A.nv = nv;
    A.planes = count ? TRC_HH_PLANE_COUNT : 0;
    double *edges = nullptr;
    if (!by_surface) {
        for (int k = 0; k < 12; ++k) A.proj[k] = proj12[k];
        edges = new double[nu + nv + 2];
        for (int k = 0; k <= nu; ++k) edges[k] = u_edges[k];
        for (int k = 0; k <= nv; ++k) edges[nu + 1 + k] = v_edges[k];
    }
    A.edges = edges;
    A.sum = sum; A.count = (unsigned long long *)count; A.outside = outside;
    unsigned long long off = 0;
    X.off_grid = &off;
    X.x = x; X.cap = cap; X.wl = wl; X.W = W; X.by_surface = by_surface;
    for (long k = 0; k < (long)nu * nv * W; ++k) sum[k] = 0.0;
    for (long k = 0; count && k < (long)nu * nv; ++k) count[k] = 0;
    for (int k = 0; k <= W; ++k) outside[k] = 0.0;
    X.Ks = ks > 0 ? ks : W;
    for (int k0 = 0; k0 < W; k0 += X.Ks) trc_hit_hist_x_host(X, k0, k0 + X.Ks < W ? k0 + X.Ks : W);
    *off_grid = (long long)off;
    delete[] edges;
}

}
