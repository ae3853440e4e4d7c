// trc_hithist.h -- the histogram of captured hits (trc_scene_histogram_hits, k_hist_hits in trc_hithist.hip): what the kernel is
// handed, where it keeps its bins, what it does per entry of the hit buffer, and the same pass as a plain host loop; then the same
// four things for the spectra of the hits (trc_scene_histogram_hits_x, k_hist_hits_x).  No device code: tests/hostcheck compiles
// this header with g++ (hithist_check.cpp, hithist_x_check.cpp) and holds the restatements of tests/test_hit_histogram_host.py and
// tests/test_hit_histogram_spectra_host.py to it.
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

// ---- The spectra of the captured hits, binned the same way (trc_scene_histogram_hits_x, k_hist_hits_x) --------------------------------
// Hits of polychromatic rays bring 3 W columns more (HitBuffer::x, column c at x + c * cap): the W sample wavelengths, the W samples
// of the spectrum that arrived and the W of the spectrum that left.  Sample k of a hit in bin b adds arrived[k] - left[k] (absorbed)
// or arrived[k] (incident) to sum[b * W + k]; the bin is the chart's, or the hit's surface less surf_lo (by_surface).
struct trc_hit_hist_x_args {
    trc_hit_hist_args h;            // n, surf, the columns of the chart, range, chart, weight, nu, nv, planes (the count bit alone), proj,
                                    // edges (not read by_surface); sum[nu nv W], count[nu nv] or NULL, outside[W + 1]: per sample, then the number
    const double *x;                // the spectral columns
    long long cap;                  // ... and their stride
    const double *wl;               // the W wavelengths every hit is held to, or NULL: no wavelength column is read
    unsigned long long *off_grid;   // (hit, sample) pairs left out because the hit's wavelength is not wl[k]
    int32_t W, by_surface;
    int32_t Ks;                     // samples per slice (trc_hit_hist_x_plan): workgroups of blockIdx.y do [y Ks, min(W, (y + 1) Ks))
};

// Where k_hist_hits_x keeps its bins.  nu nv W doubles soon exceed LDS, so the samples are sliced: a workgroup keeps the edges, the
// nu nv x Ks bins of its slice, the count plane when there is one (slice 0 fills it; every slice has the room: one layout), its Ks
// words of `outside`, the number outside and the off-grid count, in TRC_HH_LDS_BUDGET.  Ks is the widest slice that fits, W at most.
// When not even one sample fits the bins and the edges stay in global memory -- all of them, as in k_hist_hits -- and LDS holds the
// words of `outside` alone, sliced by the same rule.  (By-surface bins count their unused edges as nu = the surfaces, nv = 1: one
// formula.)
struct trc_hit_hist_x_plan { int32_t in_lds, Ks, n_slices; long long lds_bytes; };
TRC_HD trc_hit_hist_x_plan trc_hit_hist_x_plan_for(int nu, int nv, int W, bool counts) {
    const long long room = TRC_HH_LDS_BUDGET / 8, nb = (long long)nu * nv, fixed = (long long)(nu + 1) + (nv + 1) + (counts ? nb : 0) + 2;
    trc_hit_hist_x_plan p;
    long long ks = room >= fixed ? (room - fixed) / (nb + 1) : 0;        // fixed + nb Ks + Ks <= room
    p.in_lds = ks >= 1;
    if (!p.in_lds) ks = room - 2;                                        // Ks + 2 <= room
    p.Ks = (int32_t)(ks < W ? ks : W);
    p.n_slices = (W + p.Ks - 1) / p.Ks;
    p.lds_bytes = 8 * (p.in_lds ? fixed + (nb + 1) * p.Ks : (long long)p.Ks + 2);
    return p;
}

// where one slice adds: sample k of bin b at sum[b * stride + k - k_sum], of `outside` at outside[k - k_out]
struct trc_hit_hist_x_dest {
    double *sum;
    unsigned long long *count;      // NULL: no count plane, or not slice 0
    double *outside;
    int32_t stride, k_sum, k_out;
};

// the bin of entry i on the edges ue, ve (-1: in no bin): the coordinate part of trc_hit_hist_entry, which reads a weight between its
// loads and its chart (it stays as it is: calling this from it gives k_hist_hits other instructions, and its listing is held equal)
TRC_HD int trc_hit_hist_bin(const trc_hit_hist_args &A, const double *ue, const double *ve, long long i) {
    double px = 0.0, py = 0.0, pz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0, u, v;
    if (TRC_HH_IS_DIR(A.chart)) { dx = A.dx[i]; dy = A.dy[i]; dz = A.dz[i]; }
    else { px = A.px[i]; py = A.py[i]; pz = A.pz[i]; }
    trc_hit_hist_uv(A.chart, A.proj, px, py, pz, dx, dy, dz, &u, &v);
    const int iu = trc_bin_index(ue, A.nu, u), iv = trc_bin_index(ve, A.nv, v);
    return (iu >= 0 && iv >= 0) ? iu * A.nv + iv : -1;
}

#define TRC_HH_X_BATCH 4        /* samples whose loads are in flight together: 2 or 3 columns each */

// Samples [k0, k1) of the selected entry i of surface s: its bin once, then the samples in batches, every load of a batch issued
// before the first is used.  *o_n and *off count the entry when it is in no bin (slice 0 alone) and its samples off the grid.
// `add` is `+=` on the host and an atomic in the kernel.
template <class Add>
TRC_HD void trc_hit_hist_x_entry(const trc_hit_hist_x_args &X, const double *ue, const double *ve, long long i, int32_t s, int k0, int k1,
                                 const trc_hit_hist_x_dest &D, unsigned long long *o_n, unsigned long long *off, Add add) {
    const trc_hit_hist_args &A = X.h;
    const int b = X.by_surface ? s - A.surf_lo : trc_hit_hist_bin(A, ue, ve, i);
    const bool absorbed = A.weight == TRC_HH_ABSORBED, held = X.wl != nullptr;
    const double *wl_i = X.x + i, *in_i = wl_i + (long long)X.W * X.cap, *out_i = in_i + (long long)X.W * X.cap;
    if (k0 == 0) {
        if (b < 0) *o_n += 1;
        else if (D.count) add(&D.count[b], 1ull);
    }
    double *sum = D.sum + (long long)(b < 0 ? 0 : b) * D.stride;
    for (int k = k0; k < k1; k += TRC_HH_X_BATCH) {
        double arrived[TRC_HH_X_BATCH], left[TRC_HH_X_BATCH], at[TRC_HH_X_BATCH];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < TRC_HH_X_BATCH; ++j) {
            if (k + j >= k1) continue;
            arrived[j] = in_i[(long long)(k + j) * X.cap];
            left[j] = absorbed ? out_i[(long long)(k + j) * X.cap] : 0.0;
            at[j] = held ? wl_i[(long long)(k + j) * X.cap] : 0.0;
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < TRC_HH_X_BATCH; ++j) {
            if (k + j >= k1) continue;
            if (held && !(at[j] == X.wl[k + j])) { *off += 1; continue; }
            if (b < 0) add(&D.outside[k + j - D.k_out], arrived[j] - left[j]);
            else add(&sum[k + j - D.k_sum], arrived[j] - left[j]);
        }
    }
}

struct trc_hit_hist_add_plain {
    void operator()(double *p, double v) const { *p += v; }
    void operator()(unsigned long long *p, unsigned long long v) const { *p += v; }
};

// one slice of the pass on the host, over host arrays: sum, count, outside and off_grid are added to.  Slices [0, Ks), [Ks, 2 Ks) ..
// one after the other add to every sample what the unsliced pass [0, W) adds, in the same order.
static inline void trc_hit_hist_x_host(const trc_hit_hist_x_args &X, int k0, int k1) {
    const trc_hit_hist_args &A = X.h;
    const double *ue = A.edges, *ve = X.by_surface ? nullptr : A.edges + A.nu + 1;
    const trc_hit_hist_x_dest D = {A.sum, k0 == 0 ? A.count : nullptr, A.outside, X.W, 0, 0};
    unsigned long long o_n = 0, off = 0;
    for (long long i = 0; i < A.n; ++i) {
        const int32_t s = A.surf[i];
        if (s < 0 || s < A.surf_lo || s > A.surf_hi) continue;
        trc_hit_hist_x_entry(X, ue, ve, i, s, k0, k1, D, &o_n, &off, trc_hit_hist_add_plain());
    }
    A.outside[X.W] += (double)o_n;
    *X.off_grid += off;
}

#endif  // TRC_HITHIST_H
