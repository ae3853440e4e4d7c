// trc_hithist.hip -- k_hist_hits: the captured hits binned where they lie, in any chart of the hit point or of the incident direction
// (trc_scene_histogram_hits).  A translation unit of its own: the kernels of the engines are compiled as they were.
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
