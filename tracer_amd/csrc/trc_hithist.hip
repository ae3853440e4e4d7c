// trc_hithist.hip -- k_hist_hits: the captured hits binned where they lie, in any chart of the hit point or of the incident direction
// (trc_scene_histogram_hits), and k_hist_hits_x: the spectra of those hits binned the same way or per surface
// (trc_scene_histogram_hits_x), with their entry points below them.  A translation unit of its own: the kernels of the engines are
// compiled as they were.
//
// One grid-stride pass over the reserved entries of the hit buffer.  A thread reads the surface of its entry first -- 4 bytes, which
// for the entries of other surfaces and for the unwritten ends of the streaming engine's open chunks are all it reads -- then the
// three columns of the chart and the one of the weight, each a coalesced 8-byte load of consecutive entries by consecutive lanes, all
// four in flight before the first is used.  The bin comes from trc_hit_hist_entry (trc_hithist.h), the host loop's own.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "trc_scene.h"
#include "trc_hithist.h"

#define HH_THREADS 256

// LDS: edges, planes and `outside` are a private copy of the workgroup (float64 and 64-bit integer LDS atomics), whose non-zero bins
// go to global memory with one atomic each when the workgroup is done; otherwise every hit is a global atomic per plane, and the
// edges are read where the host left them.  All of them or none, so that every access has a known address space.
template <bool LDS>
__global__ __launch_bounds__(HH_THREADS) void k_hist_hits(trc_hit_hist_args A) {
    extern __shared__ double lds[];
    const int nb = A.nu * A.nv, ne = A.nu + A.nv + 2, np = trc_hit_hist_n_planes(A.planes);
    const bool sq = (A.planes & TRC_HH_PLANE_SUM_SQ) != 0, cnt = (A.planes & TRC_HH_PLANE_COUNT) != 0;
    // LDS: [u edges | v edges] [sum] [sum_sq] [count] [outside] (trc_hit_hist_lds_bytes); otherwise the two words of `outside` alone,
    // which leave as one global atomic per workgroup and word either way
    double *l_sum = lds + ne, *l_out = LDS ? l_sum + nb * np : lds;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < ne; i += HH_THREADS) lds[i] = A.edges[i];
        for (int i = threadIdx.x; i < nb * np; i += HH_THREADS) l_sum[i] = 0.0;       // (all bits zero: the count bins too)
    }
    if (threadIdx.x < 2) l_out[threadIdx.x] = 0.0;
    __syncthreads();
    const double *ue = LDS ? lds : A.edges, *ve = ue + A.nu + 1;
    double *sum = LDS ? l_sum : A.sum, *sum_sq = LDS ? l_sum + nb : A.sum_sq;
    unsigned long long *count = LDS ? (unsigned long long *)(l_sum + (sq ? 2 : 1) * nb) : A.count;
    double o_w = 0.0;               // selected hits of this thread in no bin: the map may be clipped to a part of the surface
    unsigned long long o_n = 0;
    for (long long i = (long long)blockIdx.x * HH_THREADS + threadIdx.x; i < A.n; i += (long long)gridDim.x * HH_THREADS) {
        const int32_t s = A.surf[i];
        if (s < 0 || s < A.surf_lo || s > A.surf_hi) continue;
        double w;
        const int b = trc_hit_hist_entry(A, ue, ve, i, &w);
        if (b < 0) { o_w += w; o_n += 1; continue; }
        atomicAdd(&sum[b], w);
        if (sq) atomicAdd(&sum_sq[b], w * w);
        if (cnt) atomicAdd(&count[b], 1ull);
    }
    if (o_n) { atomicAdd(&l_out[0], o_w); atomicAdd(&l_out[1], (double)o_n); }
    __syncthreads();
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < nb; i += HH_THREADS) {
            if (sum[i] != 0.0) atomicAdd(&A.sum[i], sum[i]);
            if (sq && sum_sq[i] != 0.0) atomicAdd(&A.sum_sq[i], sum_sq[i]);
            if (cnt && count[i] != 0) atomicAdd(&A.count[i], count[i]);
        }
    }
    if (threadIdx.x < 2 && l_out[threadIdx.x] != 0.0) atomicAdd(&A.outside[threadIdx.x], l_out[threadIdx.x]);
}

// k_hist_hits_x: the spectra of the same hits (trc_scene_histogram_hits_x).  blockIdx.y is a slice [k0, k1) of the W samples
// (trc_hit_hist_x_plan_for); every slice passes over all entries, reads the surface and the chart's columns again -- 28 bytes against the
// 16 to 24 of each of its samples -- and needs nothing of another slice.  trc_hit_hist_x_entry (trc_hithist.h) is the host loop's own.
struct hh_add_atomic {
    __device__ void operator()(double *p, double v) const { atomicAdd(p, v); }
    __device__ void operator()(unsigned long long *p, unsigned long long v) const { atomicAdd(p, v); }
};

// LDS: [u edges | v edges] [bins of the slice: nb x Ks] [count] [outside: Ks | number | off grid] (trc_hit_hist_x_plan_for), flushed
// with one global atomic per non-zero word; otherwise the last part alone, the bins added to in global memory.
template <bool LDS>
__global__ __launch_bounds__(HH_THREADS) void k_hist_hits_x(trc_hit_hist_x_args X) {
    extern __shared__ double lds[];
    const trc_hit_hist_args &A = X.h;
    const int nb = A.nu * A.nv, ne = A.nu + A.nv + 2, Ks = X.Ks;
    const int k0 = (int)blockIdx.y * Ks, k1 = k0 + Ks < X.W ? k0 + Ks : X.W;
    const bool has_cnt = (A.planes & TRC_HH_PLANE_COUNT) != 0, cnt = has_cnt && k0 == 0;
    double *l_sum = lds + ne, *l_out = LDS ? l_sum + nb * Ks + (has_cnt ? nb : 0) : lds;
    unsigned long long *l_cnt = (unsigned long long *)(l_sum + nb * Ks);
    if constexpr (LDS) {
        if (!X.by_surface)
            for (int i = threadIdx.x; i < ne; i += HH_THREADS) lds[i] = A.edges[i];
        for (int i = threadIdx.x; i < nb * Ks + (has_cnt ? nb : 0); i += HH_THREADS) l_sum[i] = 0.0;      // (all bits zero: the count bins too)
    }
    for (int i = threadIdx.x; i < Ks + 2; i += HH_THREADS) l_out[i] = 0.0;
    __syncthreads();
    const double *ue = LDS ? lds : A.edges, *ve = ue + A.nu + 1;
    const trc_hit_hist_x_dest D = {LDS ? l_sum : A.sum, cnt ? (LDS ? l_cnt : A.count) : nullptr, l_out, LDS ? Ks : X.W, LDS ? k0 : 0, k0};
    unsigned long long o_n = 0, off = 0;
    for (long long i = (long long)blockIdx.x * HH_THREADS + threadIdx.x; i < A.n; i += (long long)gridDim.x * HH_THREADS) {
        const int32_t s = A.surf[i];
        if (s < 0 || s < A.surf_lo || s > A.surf_hi) continue;
        trc_hit_hist_x_entry(X, ue, ve, i, s, k0, k1, D, &o_n, &off, hh_add_atomic());
    }
    if (o_n) atomicAdd(&l_out[Ks], (double)o_n);
    if (off) atomicAdd((unsigned long long *)&l_out[Ks + 1], off);
    __syncthreads();
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < nb * Ks; i += HH_THREADS) {
            const int b = i / Ks, k = k0 + i % Ks;
            if (k < k1 && l_sum[i] != 0.0) atomicAdd(&A.sum[(long long)b * X.W + k], l_sum[i]);
        }
        if (cnt)
            for (int i = threadIdx.x; i < nb; i += HH_THREADS)
                if (l_cnt[i] != 0) atomicAdd(&A.count[i], l_cnt[i]);
    }
    for (int i = threadIdx.x; i < k1 - k0; i += HH_THREADS)
        if (l_out[i] != 0.0) atomicAdd(&A.outside[k0 + i], l_out[i]);
    if (threadIdx.x == 0) {
        const unsigned long long n_off = *(const unsigned long long *)&l_out[Ks + 1];
        if (l_out[Ks] != 0.0) atomicAdd(&A.outside[X.W], l_out[Ks]);
        if (n_off) atomicAdd(X.off_grid, n_off);
    }
}

// k_hist_hits_x over X on `stream`, sliced as trc_hit_hist_x_plan_for says: X.Ks is set here
static hipError_t trc_hit_hist_x_launch(hipStream_t stream, int n_cu, trc_hit_hist_x_args X) {
    if (X.h.n <= 0) return hipSuccess;
    const trc_hit_hist_x_plan p = trc_hit_hist_x_plan_for(X.h.nu, X.h.nv, X.W, (X.h.planes & TRC_HH_PLANE_COUNT) != 0);
    X.Ks = p.Ks;
    // as many workgroups in all as k_hist_hits has, shared among the slices
    const long long blocks = (X.h.n + HH_THREADS - 1) / HH_THREADS, room = (long long)n_cu * 8 / p.n_slices;
    const dim3 grid((unsigned)(blocks < room ? blocks : room > 1 ? room : 1), (unsigned)p.n_slices);
    if (p.in_lds) hipLaunchKernelGGL(k_hist_hits_x<true>, grid, dim3(HH_THREADS), (size_t)p.lds_bytes, stream, X);
    else hipLaunchKernelGGL(k_hist_hits_x<false>, grid, dim3(HH_THREADS), (size_t)p.lds_bytes, stream, X);
    return hipGetLastError();
}

// k_hist_hits over A on `stream`: the planes and `outside` on the device are added to.  The grid is k_bin_hits'.
static hipError_t trc_hit_hist_launch(hipStream_t stream, int n_cu, const trc_hit_hist_args &A) {
    if (A.n <= 0) return hipSuccess;
    const long long blocks = (A.n + HH_THREADS - 1) / HH_THREADS;
    const unsigned grid = (unsigned)(blocks < (long long)n_cu * 8 ? blocks : (long long)n_cu * 8);
    if (trc_hit_hist_in_lds(A.nu, A.nv, A.planes))
        hipLaunchKernelGGL(k_hist_hits<true>, dim3(grid), dim3(HH_THREADS), (size_t)trc_hit_hist_lds_bytes(A.nu, A.nv, A.planes), stream, A);
    else
        hipLaunchKernelGGL(k_hist_hits<false>, dim3(grid), dim3(HH_THREADS), 16, stream, A);
    return hipGetLastError();
}

// ================================================================================================
// C-ABI: the histograms of the captured hits
// ================================================================================================
// Edges up, one pass over the reserved entries, planes down.
#define TRC_HH_MAX_BINS (1ll << 27)      /* bins of a plane: 1 GiB of float64 */
// what both histograms refuse, `fn` in front of the message; charted: the chart, the bins, their edges and proj12 are used (the spectra
// by surface use none of them)
static int hit_hist_check(const char *fn, const trc_scene *sc, const trc_hit_hist_desc *d, bool charted) {
    if (d->weight != TRC_HH_ABSORBED && d->weight != TRC_HH_INCIDENT && d->weight != TRC_HH_COUNT)
        return trc_fail(TRC_ERR_INVALID, "%s: unknown weight %d", fn, d->weight);
    if (charted) {
        if (!d->u_edges || !d->v_edges || !d->proj12) return trc_fail(TRC_ERR_INVALID, "%s: bad arguments", fn);
        if (d->chart < 0 || d->chart >= TRC_HH_CHARTS) return trc_fail(TRC_ERR_INVALID, "%s: unknown chart %d", fn, d->chart);
        if (d->nu < 1 || d->nv < 1) return trc_fail(TRC_ERR_INVALID, "%s: a histogram has at least one bin either way (%d x %d)", fn, d->nu, d->nv);
        if ((long long)d->nu * d->nv > TRC_HH_MAX_BINS)
            return trc_fail(TRC_ERR_CAPACITY, "%s: %d x %d bins (at most %lld)", fn, d->nu, d->nv, (long long)TRC_HH_MAX_BINS);
        for (int ax = 0; ax < 2; ++ax) {
            const double *e = ax ? d->v_edges : d->u_edges;
            const int n = ax ? d->nv : d->nu;
            for (int k = 0; k <= n; ++k)
                if (!std::isfinite(e[k]) || (k > 0 && !(e[k] > e[k - 1])))
                    return trc_fail(TRC_ERR_INVALID, "%s: the %s edges must be finite and increase strictly", fn, ax ? "v" : "u");
        }
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(d->proj12[k])) return trc_fail(TRC_ERR_INVALID, "%s: proj12 holds a value that is not finite", fn);
    }
    if (d->surf_lo < 0 || d->surf_hi >= sc->n_surf || d->surf_lo > d->surf_hi)
        return trc_fail(TRC_ERR_INVALID, "%s: surfaces %d..%d are not a range of the scene's %d", fn, d->surf_lo, d->surf_hi, sc->n_surf);
    const bool full = (charted && TRC_HH_IS_DIR(d->chart)) || d->weight == TRC_HH_INCIDENT;
    bool captures = false;
    for (int s = d->surf_lo; s <= d->surf_hi; ++s) {
        const int32_t fl = sc->surfaces[s].flags;
        if (!(fl & TRC_SURF_CAPTURE_HITS)) continue;
        captures = true;
        if (full && (fl & TRC_SURF_CAPTURE_LEAN))
            return trc_fail(TRC_ERR_INVALID, "%s: surface %d is captured lean (TRC_SURF_CAPTURE_LEAN): the direction and the "
                            "incident energy of its hits were not written", fn, s);
    }
    if (!captures) return trc_fail(TRC_ERR_INVALID, "%s: none of the surfaces %d..%d captures its hits", fn, d->surf_lo, d->surf_hi);
    return TRC_OK;
}

// What both histograms end with, `e` being what queuing their uploads gave: the launch between the context's two events, the words
// from d_back on down into `back`, the wait -- always: nothing queued may outlive the buffers it uses -- and the device time of the
// kernel into hist_ms.
template <class Launch>
static int hit_hist_run(const char *fn, trc_scene *sc, hipError_t e, Launch launch, const double *d_back, std::vector<double> &back) {
    trc_ctx *ctx = sc->ctx;
    if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back.data(), d_back, back.size() * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) sc->hist_ms = ms;
    return TRC_OK;
}

extern "C" int trc_scene_histogram_hits(trc_scene *sc, const trc_hit_hist_desc *d, double *sum, double *sum_sq, int64_t *count, double *outside) {
    static const char *fn = "trc_scene_histogram_hits";
    if (!sc || !d || !sum) return trc_fail(TRC_ERR_INVALID, "%s: bad arguments", fn);
    TRC_TRY(hit_hist_check(fn, sc, d, true));

    trc_ctx *ctx = sc->ctx;
    unsigned long long cursor;
    TRC_TRY(scene_hit_cursor(sc, &cursor));
    const HitBuffer &hb = sc->hits;
    const size_t nb = (size_t)d->nu * d->nv, ne = (size_t)d->nu + d->nv + 2;
    for (size_t k = 0; k < nb; ++k) { sum[k] = 0.0; if (sum_sq) sum_sq[k] = 0.0; if (count) count[k] = 0; }
    if (outside) outside[0] = outside[1] = 0.0;
    sc->hist_ms = 0.0;
    trc_hit_hist_args A;
    memset(&A, 0, sizeof(A));
    A.n = hb.used(cursor);
    if (A.n == 0) return TRC_OK;
    A.planes = (sum_sq ? TRC_HH_PLANE_SUM_SQ : 0) | (count ? TRC_HH_PLANE_COUNT : 0);
    // one block: [edges] [sum] [sum_sq] [count] [outside]
    const size_t np = (size_t)trc_hit_hist_n_planes(A.planes), words = ne + nb * np + 2;
    DevBuf<double> d_buf;
    TRC_TRY(d_buf.alloc(words));
    std::vector<double> edges(ne);
    std::copy(d->u_edges, d->u_edges + d->nu + 1, edges.begin());
    std::copy(d->v_edges, d->v_edges + d->nv + 1, edges.begin() + d->nu + 1);
    A.surf = hb.surf.get();
    A.e_abs = hb.col[0].get(); A.e_in = hb.col[1].get(); A.px = hb.col[2].get(); A.py = hb.col[3].get(); A.pz = hb.col[4].get();
    A.dx = hb.col[5].get(); A.dy = hb.col[6].get(); A.dz = hb.col[7].get();
    A.surf_lo = d->surf_lo; A.surf_hi = d->surf_hi; A.chart = d->chart; A.weight = d->weight; A.nu = d->nu; A.nv = d->nv;
    for (int k = 0; k < 12; ++k) A.proj[k] = d->proj12[k];
    A.edges = d_buf.get();
    A.sum = d_buf.get() + ne;
    A.sum_sq = sum_sq ? A.sum + nb : nullptr;
    A.count = count ? (unsigned long long *)(A.sum + nb * (sum_sq ? 2 : 1)) : nullptr;
    A.outside = A.sum + nb * np;
    std::vector<double> back(nb * np + 2);
    hipError_t e = hipMemcpyAsync(d_buf.get(), edges.data(), ne * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(A.sum, 0, (nb * np + 2) * 8, ctx->stream);
    TRC_TRY(hit_hist_run(fn, sc, e, [&] { return trc_hit_hist_launch(ctx->stream, ctx->n_cu, A); }, A.sum, back));
    memcpy(sum, back.data(), nb * 8);
    if (sum_sq) memcpy(sum_sq, back.data() + nb, nb * 8);
    if (count) memcpy(count, back.data() + nb * (sum_sq ? 2 : 1), nb * 8);
    if (outside) { outside[0] = back[nb * np]; outside[1] = back[nb * np + 1]; }
    return TRC_OK;
}

// The spectra of the captured hits binned where they lie (k_hist_hits_x): per bin of the chart, or per surface, and per sample.
extern "C" int trc_scene_histogram_hits_x(trc_scene *sc, const trc_hit_hist_x_desc *dx, double *sum, int64_t *count, double *outside,
                                          int64_t *off_grid) {
    static const char *fn = "trc_scene_histogram_hits_x";
    if (!sc || !dx || !sum) return trc_fail(TRC_ERR_INVALID, "%s: bad arguments", fn);
    const trc_hit_hist_desc *d = &dx->base;
    const bool by_surface = dx->by_surface != 0;
    TRC_TRY(hit_hist_check(fn, sc, d, !by_surface));
    if (d->weight == TRC_HH_COUNT)
        return trc_fail(TRC_ERR_INVALID, "%s: the weight is the absorbed or the incident spectrum (the count is the `count` plane)", fn);
    const int W = dx->n_samples, nu = by_surface ? d->surf_hi - d->surf_lo + 1 : d->nu, nv = by_surface ? 1 : d->nv;
    if (W < 1) return trc_fail(TRC_ERR_INVALID, "%s: %d samples", fn, W);
    for (int k = 0; dx->wl && k < W; ++k)
        if (!std::isfinite(dx->wl[k])) return trc_fail(TRC_ERR_INVALID, "%s: wl holds a value that is not finite", fn);
    const size_t nb = (size_t)nu * nv, ne = (size_t)nu + nv + 2;
    if ((long long)nb * W > TRC_HH_MAX_BINS)
        return trc_fail(TRC_ERR_CAPACITY, "%s: %d x %d bins of %d samples (at most %lld in all)", fn, nu, nv, W, (long long)TRC_HH_MAX_BINS);

    trc_ctx *ctx = sc->ctx;
    unsigned long long cursor;
    TRC_TRY(scene_hit_cursor(sc, &cursor));
    const HitBuffer &hb = sc->hits;
    const long long n = hb.used(cursor);
    if (n > 0 && hb.x_cols == 0) return trc_fail(TRC_ERR_INVALID, "%s: the hit buffer holds no spectral columns: its hits are not those of polychromatic rays", fn);
    if (hb.x_cols != 0 && hb.x_cols != 3 * W)
        return trc_fail(TRC_ERR_INVALID, "%s: the hit buffer holds %d spectral columns, 3 x %d samples, not 3 x %d", fn, hb.x_cols, hb.x_cols / 3, W);
    for (size_t k = 0; k < nb * W; ++k) sum[k] = 0.0;
    for (size_t k = 0; count && k < nb; ++k) count[k] = 0;
    for (int k = 0; outside && k <= W; ++k) outside[k] = 0.0;
    if (off_grid) *off_grid = 0;
    sc->hist_ms = 0.0;
    if (n == 0) return TRC_OK;
    // one block: [edges] [sum] [count] [outside: W, and the number] [off grid]
    const size_t tail = nb * W + (count ? nb : 0) + W + 2, words = ne + tail;
    DevBuf<double> d_buf;
    TRC_TRY(d_buf.alloc(words));
    trc_hit_hist_x_args X;
    memset(&X, 0, sizeof(X));
    trc_hit_hist_args &A = X.h;
    A.n = n;
    A.planes = count ? TRC_HH_PLANE_COUNT : 0;
    A.surf = hb.surf.get();
    A.px = hb.col[2].get(); A.py = hb.col[3].get(); A.pz = hb.col[4].get();
    A.dx = hb.col[5].get(); A.dy = hb.col[6].get(); A.dz = hb.col[7].get();
    A.surf_lo = d->surf_lo; A.surf_hi = d->surf_hi; A.chart = by_surface ? 0 : d->chart; A.weight = d->weight; A.nu = nu; A.nv = nv;
    A.edges = d_buf.get();
    A.sum = d_buf.get() + ne;
    A.count = count ? (unsigned long long *)(A.sum + nb * W) : nullptr;
    A.outside = A.sum + nb * W + (count ? nb : 0);
    X.off_grid = (unsigned long long *)(A.outside + W + 1);
    X.x = hb.x.get(); X.cap = hb.cap; X.W = W; X.by_surface = by_surface ? 1 : 0;
    // the edges up, and in a block of their own the wavelengths the hits are held to
    DevBuf<double> d_wl;
    if (dx->wl) TRC_TRY(d_wl.alloc((size_t)W));
    std::vector<double> edges(ne, 0.0), back(tail);
    hipError_t e = hipSuccess;
    if (!by_surface) {
        for (int k = 0; k < 12; ++k) A.proj[k] = d->proj12[k];
        std::copy(d->u_edges, d->u_edges + nu + 1, edges.begin());
        std::copy(d->v_edges, d->v_edges + nv + 1, edges.begin() + nu + 1);
        e = hipMemcpyAsync(d_buf.get(), edges.data(), ne * 8, hipMemcpyHostToDevice, ctx->stream);
    }
    if (dx->wl) {
        X.wl = d_wl.get();
        if (e == hipSuccess) e = hipMemcpyAsync(d_wl.get(), dx->wl, (size_t)W * 8, hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(A.sum, 0, tail * 8, ctx->stream);
    TRC_TRY(hit_hist_run(fn, sc, e, [&] { return trc_hit_hist_x_launch(ctx->stream, ctx->n_cu, X); }, A.sum, back));
    const double *b_out = back.data() + nb * W + (count ? nb : 0);
    memcpy(sum, back.data(), nb * W * 8);
    if (count) memcpy(count, back.data() + nb * W, nb * 8);
    if (outside) memcpy(outside, b_out, (size_t)(W + 1) * 8);
    if (off_grid) memcpy(off_grid, b_out + W + 1, 8);
    return TRC_OK;
}

extern "C" int trc_scene_histogram_hits_ms(trc_scene *sc, double *ms) {
    if (!sc || !ms) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    *ms = sc->hist_ms;
    return TRC_OK;
}
