// trc_hithist.hip -- k_hist_hits: the captured hits binned where they lie, in any chart of the hit point or of the incident direction
// (trc_scene_histogram_hits), and k_hist_hits_x: the spectra of those hits binned the same way or per surface
// (trc_scene_histogram_hits_x).  A translation unit of its own: the kernels of the engines are compiled as they were.
//
// One grid-stride pass over the reserved entries of the hit buffer.  A thread reads the surface of its entry first -- 4 bytes, which
// for the entries of other surfaces and for the unwritten ends of the streaming engine's open chunks are all it reads -- then the
// three columns of the chart and the one of the weight, each a coalesced 8-byte load of consecutive entries by consecutive lanes, all
// four in flight before the first is used.  The bin comes from trc_hit_hist_entry (trc_hithist.h), the host loop's own.
#include <hip/hip_runtime.h>
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

hipError_t trc_hit_hist_x_launch(hipStream_t stream, int n_cu, trc_hit_hist_x_args X) {
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

hipError_t trc_hit_hist_launch(hipStream_t stream, int n_cu, const trc_hit_hist_args &A) {
    if (A.n <= 0) return hipSuccess;
    const long long blocks = (A.n + HH_THREADS - 1) / HH_THREADS;
    const unsigned grid = (unsigned)(blocks < (long long)n_cu * 8 ? blocks : (long long)n_cu * 8);
    if (trc_hit_hist_in_lds(A.nu, A.nv, A.planes))
        hipLaunchKernelGGL(k_hist_hits<true>, dim3(grid), dim3(HH_THREADS), (size_t)trc_hit_hist_lds_bytes(A.nu, A.nv, A.planes), stream, A);
    else
        hipLaunchKernelGGL(k_hist_hits<false>, dim3(grid), dim3(HH_THREADS), 16, stream, A);
    return hipGetLastError();
}
