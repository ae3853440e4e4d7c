// trc_kernels.hip -- the engines: their CDNA4 (gfx950) kernels, the trace entry points of include/tracer_amd.h and the results of
// the ordered ones.  A scene comes to them whole (trc_scene.h) and they reach it through make_dscene, scene_facts, scene_quiet and
// the public methods of its parts; what they keep on it between calls is one object of their own (EngineState, below), which the
// scene holds and does not look into.  The scene's own entry points are trc_scene.hip, the histograms of the captured hits
// trc_hithist.hip, the entry points that take a context and no scene trc_protocol.hip; the host plumbing all share is trc_host.h.
//
// Two engines over the same per-ray core (trc_core.h):
//   * fast engine  (k_trace_fast): persistent wavefronts.  A lane carries one ray through all of its
//     bounces in registers; when a lane's ray dies (miss, absorbed, culled) the wave refills its dead
//     lanes from its slice of the ray-id range (ballot + prefix rank), so every iteration of the wave
//     loop traces 64 live segments.  Surface frames, Kd nodes and the Buie table are staged in LDS;
//     per-surface tallies are privatised in LDS and flushed once per workgroup.
//   * ordered engine (k_ord_*): one launch per bounce, reproducing the reference's bundle order and
//     parent indices for RayTree (tracer_engine.py:218-274); dead-ray compaction by wavefront ballot +
//     prefix sum, surface-major ordering by a stable radix sort of (culled, surface, block) keys.
//
// No CPU fallback lives here: without a GPU every entry point fails with TRC_ERR_DEVICE.

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>      // (wants <cstring> before it)

#include "trc_footprint.h"
#include "trc_scene.h"

// The source of the call in progress on the device, kept between calls: the descriptor with what the copy holds -- a Monte-Carlo
// loop hands over the same descriptor every call (hipMalloc / hipFree per call cost more than the upload) -- and the packed
// spectrum (FastParams.spec).
class StagedSource {
    DevBuf<trc_source_desc> d_src_;
    trc_source_desc host_;
    bool host_ok_ = false;
    GrowBuf<double> d_spec_;
public:
    int source(const trc_source_desc *src, const trc_source_desc **d_src) {
        if (!d_src_) { host_ok_ = false; TRC_TRY(d_src_.alloc(1)); }
        if (!(host_ok_ && memcmp(&host_, src, sizeof(trc_source_desc)) == 0)) {
            host_ok_ = false;
            if (hipMemcpy(d_src_.get(), src, sizeof(trc_source_desc), hipMemcpyHostToDevice) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "source upload failed");
            memcpy(&host_, src, sizeof(trc_source_desc));
            host_ok_ = true;
        }
        *d_src = d_src_.get();
        return TRC_OK;
    }
    int spectrum(const std::vector<double> &packed, const double **d_spec) {
        TRC_TRY(d_spec_.reserve((size_t)3 + 3 * TRC_SPECTRUM_MAX_POINTS));     // (room for any table: allocated once)
        // (the stream is idle between calls: every call ends with a synchronous read of its counters)
        HIP_TRY(hipMemcpy(d_spec_.get(), packed.data(), packed.size() * 8, hipMemcpyHostToDevice));
        *d_spec = d_spec_.get();
        return TRC_OK;
    }
};

// what rays of the ordered engine carry beyond the nine columns: rows of one matrix `pay` (row r of ray i at pay[r * n + i]):
// [Im of the refractive index] [Re, Im of each material at the ray's wavelength] [wavelengths of the spectrum] [spectrum]
struct PayLayout {
    int has_im = 0, n_mat = 0, W = 0;
    __host__ __device__ int rows() const { return has_im + 2 * n_mat + 2 * W; }
    __host__ __device__ int r_mat() const { return has_im; }
    __host__ __device__ int r_wl() const { return has_im + 2 * n_mat; }
    __host__ __device__ int r_spec() const { return has_im + 2 * n_mat + W; }
};

struct Level {
    int64_t n_total, n_live;
    double *x, *y, *z, *dx, *dy, *dz, *e, *ref, *wl;
    uint64_t *rid;
    int64_t *parent;
    int32_t *surf;
    double *pay;
    DevBuf<char> slab;    // the one allocation the columns above are carved from
};

// Scratch of the bounce loop: allocated for the first (usually the largest) bounce and kept; a bounce that needs more -- refractive
// surfaces can double a level -- gets a new set.
#define ORD_SCRATCH_KEEP ((size_t)1 << 26)
struct OrdScratch {
    DevBuf<double> o[9];
    DevBuf<uint64_t> orid;
    DevBuf<double> opay;
    DevBuf<uint32_t> key, ckey, cslot, skey, sslot;
    DevBuf<unsigned> blk_cnt, blk_cul;
    DevBuf<unsigned long long> blk_off, totals;
    GrowBuf<char> sort_tmp;
    size_t cap_slots = 0;
    int cap_pay = 0;
    int ensure(size_t slots, int n_pay) {
        if (slots <= cap_slots && n_pay <= cap_pay) return TRC_OK;
        if (slots < cap_slots) slots = cap_slots;
        *this = OrdScratch();
        cap_pay = n_pay;
        for (int i = 0; i < 9; ++i) TRC_TRY(o[i].alloc(slots));
        TRC_TRY(orid.alloc(slots));
        if (n_pay > 0) TRC_TRY(opay.alloc(slots * (size_t)n_pay));
        TRC_TRY(key.alloc(slots));
        TRC_TRY(ckey.alloc(slots)); TRC_TRY(cslot.alloc(slots));      // the occupied slots: at most all of them
        TRC_TRY(skey.alloc(slots)); TRC_TRY(sslot.alloc(slots));
        const size_t nblk = (slots + 255) / 256;
        TRC_TRY(blk_cnt.alloc(nblk)); TRC_TRY(blk_cul.alloc(nblk)); TRC_TRY(blk_off.alloc(nblk));
        TRC_TRY(totals.alloc(2));
        cap_slots = slots;
        return TRC_OK;
    }
};

struct trc_result {
    trc_ctx *ctx;
    std::vector<Level> levels;
    PayLayout lay;
};

// ------------------------------------------------------------------------------------------------
// Wave-cooperative fast path (k_trace_coop).  Same candidates, same exact float64 tests and the same winner as
// trc_nearest_accel32 / brute force -- the work is only distributed differently over the 64 lanes:
//   refill   dead lanes take fresh rays; a ray with no candidate at all (misses the Kd root box and the boxes of
//            the always-relevant surfaces) is finished on the spot and its lane refilled again, up to 3 passes,
//            so that the lanes entering the walk are (almost) all doing useful work;
//   walk     each lane walks the tree for its own ray (single precision, packed 4-byte LDS stack) and only lists
//            the leaves it crosses;
//   boxes    all lanes drain the leaf lists together: one (ray, leaf) item per lane per round (prefix sum +
//            binary search), box test of every surface of the leaf;
//   exact    survivors are queued; all lanes drain that queue with trc_intersect (float64) and combine per ray
//            with LDS atomics: minimal t, then the lowest surface index among equal t (tracer_engine.py:58-63).
// ------------------------------------------------------------------------------------------------
// (COOP_LEAFCAP, COOP_E, COOP_WAVE_BYTES and the limits of the packed stack: trc_forms.h, where mega_plan sizes the launch)
struct CoopLds {
    double *exq_t;                // [COOP_E]
    unsigned long long *best_t;   // [64]
    uint32_t *exq;                // [COOP_E]
    int *best_s;                  // [64]
    int *dirty;                   // [64]
    uint32_t *pre;                // [64] inclusive prefix of the leaf-list lengths
    uint16_t *lst;                // [COOP_LEAFCAP][64] leaves crossed by each lane's ray
    uint32_t *stack;              // [depth][64]
};

__device__ __forceinline__ CoopLds coop_carve(char *base) {
    CoopLds W;
    W.exq_t = (double *)base; base += COOP_E * 8;
    W.best_t = (unsigned long long *)base; base += 64 * 8;
    W.exq = (uint32_t *)base; base += COOP_E * 4;
    W.best_s = (int *)base; base += 64 * 4;
    W.dirty = (int *)base; base += 64 * 4;
    W.pre = (uint32_t *)base; base += 64 * 4;
    W.lst = (uint16_t *)base; base += COOP_LEAFCAP * 64 * 2;
    W.stack = (uint32_t *)base;
    return W;
}

// LDS traffic between lanes of one wave: order it for the compiler and the hardware
#define WAVE_SYNC()                                              \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)

// the float64 ray of every lane, kept in the owner's registers and read by other lanes with cross-lane shuffles
struct CoopRay {
    double px, py, pz, dx, dy, dz;
};

// drain the exact-test queue (wave-uniform call)
__device__ __forceinline__ void coop_drain_exact(const CoopLds &W, int ecount, const CoopRay &ray, const double *recs, int stride,
                                                 const double *extra, unsigned lane) {
    if (ecount == 0) return;
    WAVE_SYNC();
    for (int base = 0; base < ecount; base += 64) {
        int i = base + (int)lane;
        const bool valid = i < ecount;
        uint32_t en = valid ? W.exq[i] : 0u;
        int L = (int)(en >> 16), sidx = (int)(en & 0xFFFFu);
        // all lanes shuffle (the source lane must be active), only the valid ones compute
        double qx = __shfl(ray.px, L, 64), qy = __shfl(ray.py, L, 64), qz = __shfl(ray.pz, L, 64);
        double ex = __shfl(ray.dx, L, 64), ey = __shfl(ray.dy, L, 64), ez = __shfl(ray.dz, L, 64);
        if (valid) {
            double t = trc_intersect(recs + (size_t)sidx * stride, extra, qx, qy, qz, ex, ey, ez);
            if (!(t > 0.0) || !(t < TRC_INF)) t = TRC_INF;    // t == 0 is not a hit (tracer_engine.py:58)
            W.exq_t[i] = t;
            if (t < TRC_INF) {
                unsigned long long bits = (unsigned long long)__double_as_longlong(t);   // t > 0: bit order = numeric order
                unsigned long long old = atomicMin(&W.best_t[L], bits);
                if (bits < old) W.dirty[L] = 1;
            }
        }
    }
    WAVE_SYNC();
    if (W.dirty[lane]) { W.best_s[lane] = 0x7FFFFFFF; W.dirty[lane] = 0; }   // a strictly nearer hit: forget the old surface
    WAVE_SYNC();
    for (int base = 0; base < ecount; base += 64) {
        int i = base + (int)lane;
        if (i < ecount) {
            double t = W.exq_t[i];
            if (t < TRC_INF) {
                uint32_t en = W.exq[i];
                int L = (int)(en >> 16), sidx = (int)(en & 0xFFFFu);
                if ((unsigned long long)__double_as_longlong(t) == W.best_t[L]) atomicMin(&W.best_s[L], sidx);   // lowest index wins ties
            }
        }
    }
    WAVE_SYNC();
}

// append (ray lane, surface) to the exact queue for the lanes whose `want` is set (wave-uniform call)
__device__ __forceinline__ void coop_push_exact(const CoopLds &W, int &ecount, bool want, uint32_t entry, const CoopRay &ray,
                                                const double *recs, int stride, const double *extra, unsigned lane) {
    unsigned long long m = __ballot(want);
    if (!m) return;
    int add = __popcll(m);
    if (ecount + add > COOP_E) { coop_drain_exact(W, ecount, ray, recs, stride, extra, lane); ecount = 0; }
    if (want) W.exq[ecount + __popcll(m & ((1ull << lane) - 1ull))] = entry;
    ecount += add;
}

// drain the per-lane leaf lists: items (ray lane, leaf) are dealt to the 64 lanes round by round (wave-uniform call)
__device__ __forceinline__ void coop_drain_leaves(const trc_accel_view &A, const CoopLds &W, unsigned cnt, int &ecount,
                                                  const trc_ray32 &mine, const CoopRay &ray, const double *recs, int stride,
                                                  const double *extra, unsigned lane) {
    // inclusive prefix sum of the list lengths
    unsigned incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        unsigned o = __shfl_up(incl, off, 64);
        if ((int)lane >= off) incl += o;
    }
    const unsigned total = __shfl(incl, 63, 64);
    if (total == 0) return;
    W.pre[lane] = incl;
    WAVE_SYNC();
    for (unsigned base = 0; base < total; base += 64) {
        const unsigned e = base + lane;
        const bool valid = e < total;
        unsigned lc = 0, off = 0, L = 0;
        trc_ray32 r;
        r.ox = r.oy = r.oz = r.ix = r.iy = r.iz = r.dx = r.dy = r.dz = 0.0f;
        if (valid) {
            // first lane whose inclusive prefix exceeds e
            unsigned lo = 0, hi = 63;
            while (lo < hi) {
                unsigned mid = (lo + hi) >> 1;
                if (W.pre[mid] > e) hi = mid; else lo = mid + 1;
            }
            L = lo;
            unsigned j = e - (L ? W.pre[L - 1] : 0u);
            unsigned node = W.lst[j * 64 + L];
            off = A.nodes[2 * node];
            lc = A.nodes[2 * node + 1] >> 2;
        }
        r.ox = __shfl(mine.ox, (int)L, 64); r.oy = __shfl(mine.oy, (int)L, 64); r.oz = __shfl(mine.oz, (int)L, 64);
        r.ix = __shfl(mine.ix, (int)L, 64); r.iy = __shfl(mine.iy, (int)L, 64); r.iz = __shfl(mine.iz, (int)L, 64);
        // box tests of the leaf's surfaces, four at a time (independent LDS loads in flight), hits kept as a bit mask;
        // the wave-level queue append happens once per round, for the (rare) set bits
        for (unsigned kb = 0; __ballot(kb < lc); kb += 32) {        // the hit mask holds 32 surfaces at a time
            unsigned hits = 0;
            for (unsigned k0 = kb; k0 < kb + 32 && __ballot(k0 < lc); k0 += 4) {
                unsigned sid[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) sid[q] = (k0 + q < lc) ? (unsigned)A.leaf_surfs[off + k0 + q] : 0u;
                bool h[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) h[q] = trc_box_hit32(A.sbox + 6 * (size_t)sid[q], r);
#pragma unroll
                for (int q = 0; q < 4; ++q) if (h[q] && k0 + q < lc) hits |= 1u << (k0 + q - kb);
            }
            while (__ballot(hits != 0)) {
                bool want = hits != 0;
                unsigned k = want ? kb + (unsigned)__ffs((int)hits) - 1u : 0u;
                unsigned sidx = want ? (unsigned)A.leaf_surfs[off + k] : 0u;
                coop_push_exact(W, ecount, want, (L << 16) | sidx, ray, recs, stride, extra, lane);
                hits &= hits - 1u;
            }
        }
    }
    WAVE_SYNC();
}

// fresh ray for a lane: from the source descriptor or from the given bundle (SUN: trc_source_ray_t's; LAMP: the descriptor is one
// of the arc-lamp kinds, trc_lamp_ray_t)
template <int KIND = -1, bool SPEC = false, bool SUN = false, bool LAMP = false>
__device__ __forceinline__ void fast_new_ray(const FastParams &P, const double *buie, long long id, double &px, double &py,
                                             double &pz, double &dx, double &dy, double &dz, double &e, double &ref, double &wl,
                                             unsigned long long &rid, const trc_buie_fast *bf = nullptr) {
    rid = P.rid ? P.rid[id] : (P.ray_offset + (unsigned long long)id);
    if (P.src) {
        if constexpr (LAMP) trc_lamp_ray_t<KIND>(P.src, P.seed, rid, &px, &py, &pz, &dx, &dy, &dz);
        else trc_source_ray_t<KIND, SUN>(P.src, buie, buie ? buie + TRC_BUIE_TABLE : nullptr, P.seed, rid, &px, &py, &pz, &dx, &dy, &dz, bf);
        e = P.src->energy;
        if (SPEC) trc_spectrum_of(P.spec, P.seed, rid, &wl, &ref);     // (the megakernel draws at birth: its rays live in registers)
        else { ref = 1.0; wl = 0.0; }
    } else {
        px = P.x[id]; py = P.y[id]; pz = P.z[id];
        dx = P.dx[id]; dy = P.dy[id]; dz = P.dz[id];
        e = P.e[id];
        ref = P.ref ? P.ref[id] : 1.0;
        wl = P.wl ? P.wl[id] : 0.0;
    }
}

// the megakernel's two kernels (trc_mega.inc): the instances of every source kind but the arc lamps ...
#define MEGA_KERNEL_FAST template <int THREADS, bool SPEC = false, bool SUN = false, bool CHART = false> __global__ __launch_bounds__(THREADS) void k_trace_fast(FastParams P)
#define MEGA_KERNEL_COOP template <int THREADS, bool SPEC = false, bool SUN = false, bool CHART = false> __global__ __launch_bounds__(THREADS) void k_trace_coop(FastParams P)
#define MEGA_SUN SUN
#define MEGA_LAMP false
#include "trc_mega.inc"
#undef MEGA_KERNEL_FAST
#undef MEGA_KERNEL_COOP
#undef MEGA_SUN
#undef MEGA_LAMP
// ... and those of the arc lamps, under names of their own
#define MEGA_KERNEL_FAST template <int THREADS, bool SPEC, bool CHART> __global__ __launch_bounds__(THREADS) void k_lamp_fast(FastParams P)
#define MEGA_KERNEL_COOP template <int THREADS, bool SPEC, bool CHART> __global__ __launch_bounds__(THREADS) void k_lamp_coop(FastParams P)
#define MEGA_SUN false
#define MEGA_LAMP true
#include "trc_mega.inc"
#undef MEGA_KERNEL_FAST
#undef MEGA_KERNEL_COOP
#undef MEGA_SUN
#undef MEGA_LAMP

// What the decisions of trc_forms.h read of the scene.  walk: with the pass over the surfaces, which the streaming engine alone needs.
static trc_scene_facts scene_facts(const trc_scene *sc, bool walk) {
    trc_scene_facts s = {};
    trc_scene_facts_fill(sc->surfaces.data(), sc->n_surf, sc->search.host(), walk, &s);
    sc->surfaces.facts(s); sc->search.facts(s); sc->kd.facts(s); sc->tally.facts(s);
    return s;
}

// Lets `fn` take `lds` bytes of dynamic LDS: beyond 64 KiB a kernel must be allowed them first
static int kernel_allow_lds(const void *fn, size_t lds) {
    if (lds <= LDS_MAX_PLAIN) return TRC_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
    return TRC_OK;
}

// ... and sets *cap to its workgroups resident at once: the occupancy, at least one and at most `max_bpc` per CU, on `n_cu` CUs
static int kernel_grid_cap(const void *fn, int threads, size_t lds, int max_bpc, int n_cu, unsigned *cap) {
    TRC_TRY(kernel_allow_lds(fn, lds));
    int bpc = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, fn, threads, lds) != hipSuccess || bpc < 1) bpc = 1;
    if (bpc > max_bpc) bpc = max_bpc;
    *cap = (unsigned)(n_cu * bpc);
    return TRC_OK;
}

#include "trc_stream.inc"

// ================================================================================================
// ordered engine
// ================================================================================================
struct OrdParams {
    DScene sc;
    // current bundle (live rays of the previous level)
    const double *x, *y, *z, *dx, *dy, *dz, *e, *ref, *wl;
    const uint64_t *rid;
    long long n;
    int event;  // index of this interaction (1-based), same for the whole bundle
    int flags;
    double min_energy;
    unsigned long long seed;
    // outputs, 2n slots: child 0 of ray i at slot i, child 1 at slot n+i
    double *ox, *oy, *oz, *odx, *ody, *odz, *oe, *oref, *owl;
    uint64_t *orid;
    uint32_t *key;  // (culled << 30) | (surface << 2) | block, 0xFFFFFFFF = empty slot
    const double *pay;      // PayLayout rows of the current bundle (null: none), rows pay_stride apart (the level's total ray count:
                            // its culled rays sit behind the n live ones)
    long long pay_stride;
    double *opay;           // the children's, rows 2n apart
    PayLayout lay;
    const double *mat_tab;  // the scene's tabulated materials (trc_material_index's table): read by the MAT instances alone; last
};

// pending far children of the single-precision Kd walk (trc_nearest_accel32), in LDS: entry sp of thread t at [sp * 256 + t].
// (In private memory the two stacks of this kernel were 576 bytes of scratch per lane -- 300 MB per dispatch, more than the
// runtime keeps, so every launch allocated and freed it: 7.4 ms per bounce, whatever the number of rays.)  ORD_STACK_DEPTH entries
// each (trc_forms.h).
struct LdsStack32 {
    uint32_t *na;
    float *tmax;
    __device__ __forceinline__ void push(int sp, uint32_t n, float t) { na[sp * 256] = n; tmax[sp * 256] = t; }
    __device__ __forceinline__ void pop(int sp, uint32_t *n, float *t) { *n = na[sp * 256]; *t = tmax[sp * 256]; }
};

#define ORD_EMPTY 0xFFFFFFFFu
#define ORD_CULLED_BIT (1u << 30)

// FAST: the conservative single-precision search of the fast engines (boxes of the geometry, packed Kd nodes) in front of the exact
// float64 tests -- the same nearest hit, the same tie rule (trc_nearest_accel32; tests/hostcheck pins it against brute force) --
// with its stack in LDS; otherwise the float64 walk of the caller's tree / brute force, with a stack in private memory.
// MODE 2: the scene stands on the large grid (a mesh): trc_nearest_grid32.
// CHART: the flux maps may bin in the charts other than XY (trc_fluxmap_uv)
// MAT: the scene's tabulated materials are on the device (P.mat_tab) and the rays bring no rows of them (P.lay.n_mat == 0): a hit
//      between materials evaluates both at the ray's wavelength (trc_shade_xt)
template <int MODE, bool CHART = false, bool MAT = false>
__global__ __launch_bounds__(256) void k_ord_bounce(OrdParams P) {
    constexpr bool FAST = MODE == 1;
    __shared__ uint32_t s_na[FAST ? ORD_STACK_DEPTH * 256 : 1];
    __shared__ float s_tm[FAST ? ORD_STACK_DEPTH * 256 : 1];
    const DScene &sc = P.sc;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < P.n;              // (no lane leaves early: the tallies below are summed per wave)
    if (!live) i = 0;
    double px = P.x[i], py = P.y[i], pz = P.z[i], dx = P.dx[i], dy = P.dy[i], dz = P.dz[i], e = P.e[i];
    double ref = P.ref[i], wl = P.wl[i];
    unsigned long long rid = P.rid[i];
    double t;
    int s;
    const bool use_kd = sc.has_kd && (P.flags & TRC_TRACE_ACCEL);
    if (MODE == 2) {
        trc_nearest_grid32(sc, px, py, pz, dx, dy, dz, &t, &s);
    } else if (FAST) {
        const trc_accel_view A = stream_accel_global(sc, use_kd ? 1 : 0);
        LdsStack32 stk;
        stk.na = s_na + threadIdx.x; stk.tmax = s_tm + threadIdx.x;
        trc_nearest_accel32(A, stk, sc.recs, sc.stride, sc.extra, px, py, pz, dx, dy, dz, use_kd, &t, &s);
        if (s < 0) t = 0.0;
    } else if (use_kd) {
        trc_kd_view kd = make_kd_view(sc, sc.kd_a, sc.kd_b, sc.kd_split, sc.kd_leaf, sc.kd_always);
        LocalKdStack stk;
        trc_nearest_kd(kd, stk, sc.recs, sc.stride, sc.extra, px, py, pz, dx, dy, dz, &t, &s);
    } else {
        trc_nearest_brute(sc.recs, sc.stride, sc.n_surf, sc.extra, px, py, pz, dx, dy, dz, &t, &s);
    }
    if (!live) s = -1;
    int ts = -1;                // the surface this lane's hit is tallied on, with absorbed and incident energy
    double tea = 0.0, tei = 0.0;
    uint32_t k0 = ORD_EMPTY, k1 = ORD_EMPTY;
    if (s >= 0) {
        const double *rec = sc.recs + (size_t)s * sc.stride;
        double hx = px + t * dx, hy = py + t * dy, hz = pz + t * dz;
        double nx, ny, nz;
        trc_normal(rec, hx, hy, hz, dx, dy, dz, &nx, &ny, &nz);
        trc_ray_out out[2];
        const double path = sqrt((hx - px) * (hx - px) + (hy - py) * (hy - py) + (hz - pz) * (hz - pz));
        trc_ray_ext X;
        X.ref_im = 0.0; X.W = P.lay.W; X.n_mat = P.lay.n_mat; X.stride = P.pay_stride; X.mat = X.wl = X.spec = nullptr;
        if (P.pay) {
            if (P.lay.has_im) X.ref_im = P.pay[i];
            X.mat = P.pay + (size_t)P.lay.r_mat() * P.pay_stride + i;
            X.wl = P.pay + (size_t)P.lay.r_wl() * P.pay_stride + i;
            X.spec = P.pay + (size_t)P.lay.r_spec() * P.pay_stride + i;
        }
        double out_im[2], poly_th;
        int n_out;
        if constexpr (MAT)
            n_out = trc_shade_xt(trc_rec_opt_kind(rec), sc.opt + (size_t)s * 8, sc.extra, trc_rec_extra_off(rec),
                                 trc_rec_extra_len(rec), rec[2], rec[5], rec[8], dx, dy, dz, e, ref, wl, path, nx, ny,
                                 nz, P.seed, rid, (uint32_t)P.event, X, P.mat_tab, out, out_im, &poly_th);
        else
            n_out = trc_shade_x(trc_rec_opt_kind(rec), sc.opt + (size_t)s * 8, sc.extra, trc_rec_extra_off(rec),
                                trc_rec_extra_len(rec), rec[2], rec[5], rec[8], dx, dy, dz, e, ref, wl, path, nx, ny,
                                nz, P.seed, rid, (uint32_t)P.event, X, out, out_im, &poly_th);
        double e_out = out[0].e + (n_out > 1 ? out[1].e : 0.0);
        const bool volume = out[0].back > 0.0;      // scattered in the medium before the surface: nothing recorded there
        if (volume) { hx -= out[0].back * dx; hy -= out[0].back * dy; hz -= out[0].back * dz; }
        if (!volume) { ts = s; tea = e - e_out; tei = e; }         // (the three sums of the surface: below, per wave)
        int fm = (!volume && sc.fm_of_surf) ? sc.fm_of_surf[s] : -1;
        if (fm >= 0) {
            const FluxMapDev &m = sc.fms[fm];
            double u, v;
            if constexpr (CHART) trc_fluxmap_uv(m.chart, m.proj, hx, hy, hz, &u, &v);
            else {
                u = m.proj[0] * hx + m.proj[1] * hy + m.proj[2] * hz + m.proj[3];
                v = m.proj[4] * hx + m.proj[5] * hy + m.proj[6] * hz + m.proj[7];
            }
            int iu = trc_bin_index(sc.fm_edges + m.edges_u, m.nu, u);
            int iv = trc_bin_index(sc.fm_edges + m.edges_v, m.nv, v);
            if (iu >= 0 && iv >= 0) atomicAdd(&sc.tally[m.bins + (int64_t)iu * m.nv + iv], e - e_out);
        }
        for (int c = 0; c < n_out; ++c) {
            long long slot = (c == 0) ? i : (P.n + i);
            P.ox[slot] = hx + out[c].shift * nx; P.oy[slot] = hy + out[c].shift * ny; P.oz[slot] = hz + out[c].shift * nz;
            P.odx[slot] = out[c].dx; P.ody[slot] = out[c].dy; P.odz[slot] = out[c].dz;
            P.oe[slot] = out[c].e; P.oref[slot] = out[c].ref; P.owl[slot] = wl;
            P.orid[slot] = (c == 0) ? rid : trc_child_rid(rid, (uint32_t)P.event);
            if (P.opay) {       // children inherit what the ray carries (RayBundle.inherit, ray_bundle.py:117-143), the optics' changes applied
                const size_t S2 = 2 * (size_t)P.n;
                if (P.lay.has_im) P.opay[slot] = out_im[c];
                for (int k = 0; k < 2 * P.lay.n_mat; ++k) P.opay[(size_t)(P.lay.r_mat() + k) * S2 + slot] = X.mat[(size_t)k * P.pay_stride];
                const double *tab = sc.extra + trc_rec_extra_off(rec);
                for (int w = 0; w < P.lay.W; ++w) {
                    const double xw = X.wl[(size_t)w * P.pay_stride];
                    const double f = poly_th >= 0.0 ? 1.0 - trc_poly_absorptance(tab, poly_th, xw) : out[c].sf;
                    P.opay[(size_t)(P.lay.r_wl() + w) * S2 + slot] = xw;
                    P.opay[(size_t)(P.lay.r_spec() + w) * S2 + slot] = X.spec[(size_t)w * P.pay_stride] * f;
                }
            }
            uint32_t k = ((uint32_t)s << 2) | (uint32_t)out[c].blk;
            if (out[c].e <= P.min_energy) k |= ORD_CULLED_BIT;   // tracer_engine.py:242, :270-274
            if (c == 0) k0 = k; else k1 = k;
        }
    }
    // The three sums per surface: global float64 atomics on one word are served one after the other, and a bounce whose rays all land
    // on the receiver of a field put 640 000 x 3 of them on three words -- 7.8 ms for a bounce of 6e5 rays: per wave (tally_by_wave)
    tally_by_wave<8>(sc.tally, sc.n_surf, ts, tea, tei, 4);
    if (live) {
        P.key[i] = k0;
        P.key[P.n + i] = k1;
    }
}

// ---- order-preserving compaction of the occupied slots: ballot + prefix sum ----
// pass 1: per-block counts of occupied and of culled slots
__global__ __launch_bounds__(256) void k_compact_count(const uint32_t *key, long long n, unsigned *blk_cnt,
                                                       unsigned *blk_culled) {
    __shared__ unsigned s_cnt[4], s_cul[4];
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t k = (i < n) ? key[i] : ORD_EMPTY;
    bool occ = k != ORD_EMPTY;
    bool cul = occ && (k & ORD_CULLED_BIT);
    unsigned long long m = __ballot(occ), mc = __ballot(cul);
    int w = threadIdx.x >> 6;
    if (lane_id() == 0) { s_cnt[w] = __popcll(m); s_cul[w] = __popcll(mc); }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        blk_culled[blockIdx.x] = s_cul[0] + s_cul[1] + s_cul[2] + s_cul[3];
    }
}

// pass 2: exclusive scan of the block counts (one workgroup, wave-level scan over 256-wide chunks)
__global__ __launch_bounds__(256) void k_scan_blocks(const unsigned *blk_cnt, const unsigned *blk_culled,
                                                     long long n_blocks, unsigned long long *blk_off,
                                                     unsigned long long *totals) {
    __shared__ unsigned long long s_wave[4];
    __shared__ unsigned long long s_carry;
    unsigned long long culled = 0;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (long long base = 0; base < n_blocks; base += blockDim.x) {
        long long i = base + threadIdx.x;
        unsigned long long v = (i < n_blocks) ? blk_cnt[i] : 0;
        culled += (i < n_blocks) ? blk_culled[i] : 0;
        // inclusive scan inside the wave
        unsigned long long incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            unsigned long long o = __shfl_up(incl, off, 64);
            if ((int)lane_id() >= off) incl += o;
        }
        int w = threadIdx.x >> 6;
        if (lane_id() == 63) s_wave[w] = incl;
        __syncthreads();
        unsigned long long wave_off = 0;
        for (int k = 0; k < w; ++k) wave_off += s_wave[k];
        unsigned long long carry = s_carry;
        if (i < n_blocks) blk_off[i] = carry + wave_off + incl - v;
        __syncthreads();
        if (threadIdx.x == blockDim.x - 1) s_carry = carry + wave_off + incl;
        __syncthreads();
    }
    // total culled: block reduction
    __shared__ unsigned long long s_cul[4];
    unsigned long long c = culled;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if (lane_id() == 0) s_cul[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        totals[0] = s_carry;
        totals[1] = s_cul[0] + s_cul[1] + s_cul[2] + s_cul[3];
    }
}

// pass 3: scatter (key, slot) of the occupied slots, in slot order
__global__ __launch_bounds__(256) void k_compact_scatter(const uint32_t *key, long long n,
                                                         const unsigned long long *blk_off, uint32_t *ckey,
                                                         uint32_t *cslot) {
    __shared__ unsigned s_cnt[4];
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t k = (i < n) ? key[i] : ORD_EMPTY;
    bool occ = k != ORD_EMPTY;
    unsigned long long m = __ballot(occ);
    int w = threadIdx.x >> 6;
    if (lane_id() == 0) s_cnt[w] = __popcll(m);
    __syncthreads();
    unsigned wave_off = 0;
    for (int q = 0; q < w; ++q) wave_off += s_cnt[q];
    if (occ) {
        unsigned long long pos = blk_off[blockIdx.x] + wave_off + __popcll(m & ((1ull << lane_id()) - 1ull));
        ckey[pos] = k;
        cslot[pos] = (uint32_t)i;
    }
}

struct GatherParams {
    const double *ox, *oy, *oz, *odx, *ody, *odz, *oe, *oref, *owl;
    const uint64_t *orid;
    const uint32_t *skey, *sslot;
    long long m, n_parent;
    double *x, *y, *z, *dx, *dy, *dz, *e, *ref, *wl;
    uint64_t *rid;
    int64_t *parent;
    int32_t *surf;
    const double *opay;     // n_pay rows, 2 n_parent apart
    double *pay;            // n_pay rows, m apart
    int n_pay;
    const double *recs;     // surface records (optics kind): a ray of the scattered block of a scattering medium never reached the
    int stride;             // surface it is filed under -- the level says so (TRC_LEVEL_VOLUME)
};

__global__ __launch_bounds__(256) void k_ord_gather(GatherParams G) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G.m) return;
    uint32_t slot = G.sslot[j], k = G.skey[j];
    G.x[j] = G.ox[slot]; G.y[j] = G.oy[slot]; G.z[j] = G.oz[slot];
    G.dx[j] = G.odx[slot]; G.dy[j] = G.ody[slot]; G.dz[j] = G.odz[slot];
    G.e[j] = G.oe[slot]; G.ref[j] = G.oref[slot]; G.wl[j] = G.owl[slot];
    G.rid[j] = G.orid[slot];
    G.parent[j] = (int64_t)(slot >= G.n_parent ? slot - G.n_parent : slot);   // tracer_engine.py:235-236
    {
        const int32_t sj = (int32_t)((k & ~ORD_CULLED_BIT) >> 2);
        // block 0 of a scattering medium is the scattered block (trc_shade: the blocks of the surface interaction come behind it)
        const bool vol = (k & 3u) == 0u && trc_rec_opt_kind(G.recs + (size_t)sj * G.stride) == TRC_OPT_REFRACTIVE_SCATTERING;
        G.surf[j] = vol ? (sj | TRC_LEVEL_VOLUME) : sj;
    }
    for (int r = 0; r < G.n_pay; ++r) G.pay[(size_t)r * G.m + j] = G.opay[(size_t)r * 2 * G.n_parent + slot];
}

__global__ void k_fill_f64(double *p, long long n, double v) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        p[i] = v;
}
__global__ void k_fill_rid(uint64_t *p, long long n, unsigned long long offset) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        p[i] = offset + (unsigned long long)i;
}

// ================================================================================================
// rocprim's scan and sort for the library (trc_host.h)
// ================================================================================================
hipError_t dev_exclusive_scan_u32(void *tmp, size_t &tmp_bytes, uint32_t *in, uint32_t *out, size_t n, hipStream_t stream) {
    return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), stream);
}
hipError_t dev_sort_pairs_u32(void *tmp, size_t &tmp_bytes, uint32_t *key_in, uint32_t *key_out, uint32_t *val_in, uint32_t *val_out, size_t n,
                              unsigned end_bit, hipStream_t stream) {
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key_out, val_in, val_out, n, 0, end_bit, stream);
}

// ================================================================================================
// what the engines keep on a scene between calls
// ================================================================================================
// Made by the first trace of a scene (engine_state) and freed with it: trc_scene_destroy has waited for the context's stream by then.
// Nothing in it holds device memory before its first use: the streaming engine's slots are made by stream_engine_init, the ordered
// scratch by OrdScratch::ensure.
struct EngineState {
    StreamEngine stream_eng;          // slots of the streaming fast engine (trc_stream.inc)
    OrdScratch ord_scratch;           // scratch of the ordered engine's bounce loop (ORD_SCRATCH_KEEP)
    StagedSource staged;
    GrowBuf<double> d_last[7];        // device side of trc_trace_fast's `last` bundle (seven hipMalloc / hipFree per call were a millisecond
                                      // of a Monte-Carlo loop's 1e6-ray calls)
    GrowBuf<double> d_last_x;         // ... and the spectra of the rays a source that carries its spectrum leaves (W rows)
};

void EngineStateDelete::operator()(EngineState *e) const { delete e; }

static int engine_state(trc_scene *sc, EngineState **out) {
    if (!sc->engine) {
        sc->engine.reset(new (std::nothrow) EngineState());
        if (!sc->engine) return trc_fail(TRC_ERR_NOMEM, "out of host memory");
    }
    *out = sc->engine.get();
    return TRC_OK;
}

// ================================================================================================
// what a call brings: the source's spectrum, the columns rays carry beyond the nine (both engines)
// ================================================================================================
// The spectrum travels to the fast engine as FastParams.spec (trc_spectrum_of layout: n, constant wavelength, index, then the
// table), in a buffer the engines keep on the scene between calls.  The SPEC instances of the kernels draw the wavelength where a source ray
// first needs one.
static int scene_stage_spectrum(EngineState &E, const SourceSpectrum &sp, const double **d_spec) {
    const int n_tab = sp.desc->kind != TRC_SPECTRUM_CONSTANT ? sp.desc->n : 0;
    std::vector<double> packed((size_t)3 + sp.tab.size());
    packed[0] = (double)n_tab; packed[1] = sp.desc->wavelength; packed[2] = sp.desc->ref_index;
    std::copy(sp.tab.begin(), sp.tab.end(), packed.begin() + 3);
    return E.staged.spectrum(packed, d_spec);
}

// The scene's tabulated materials are evaluated on the device for this call: it has a table for every material its optics name
// (trc_scene_set_materials), the bundle brings no rows of its own (trc_rays.mat: those are traced as they are), and no flux map
// bins in a chart other than XY (there is no CHART x MAT kernel instance)
static bool scene_mat_route(const trc_scene *sc, const trc_rays *in) {
    return sc->mat_tab_serves() && !(in && in->mat) && !sc->tally.has_chart();
}

// What the bundle `in` (NULL: a source descriptor, whose rays carry nothing but what its spectrum gives them: has_spec) brings
// beyond the nine columns, against what the scene's optics read: lay->n_mat and lay->W.  has_im is the ordered engine's to set.
// *mat_dev: scene_mat_route -- the materials' indices come from the scene's tables, lay->n_mat is 0.
// carried_W: the source carries its spectrum (TRC_SPECTRUM_CARRIED) -- its rays bring W samples each, and no wavelength of their own.
static int check_carried(const trc_scene *sc, const trc_rays *in, bool has_spec, int carried_W, const char *who, PayLayout *lay, bool *mat_dev) {
    const CarryNeeds &needs = sc->surfaces.needs();
    lay->n_mat = (in && in->mat) ? (int)in->n_mat : 0;
    lay->W = (in && in->spectra && in->spec_wl) ? in->n_spec : (!in ? carried_W : 0);
    *mat_dev = scene_mat_route(sc, in);
    if (!in && carried_W > 0 && needs.max_mat >= 0)
        return trc_fail(TRC_ERR_UNSUPPORTED, "%s: the scene refracts between tabulated materials, and a ray that carries the source's spectrum has no single wavelength to evaluate them at", who);
    if (lay->W < 0 || lay->W > 4096 || lay->n_mat < 0 || lay->n_mat > 64) return trc_fail(TRC_ERR_INVALID, "%s: n_spec or n_mat out of range", who);
    if (needs.max_mat >= 0 && *mat_dev) {
        if (in && !in->wavelength)
            return trc_fail(TRC_ERR_INVALID, "%s: the scene refracts between tabulated materials: the bundle needs wavelengths", who);
        if (!in && !has_spec)       // (rays of wavelength 0 would index nothing sensible)
            return trc_fail(TRC_ERR_INVALID, "%s: the scene refracts between tabulated materials: a source descriptor needs a source spectrum, which gives its rays their wavelengths", who);
    } else if (needs.max_mat >= 0 && (!in || !in->wavelength || lay->n_mat <= needs.max_mat))
        return trc_fail(TRC_ERR_INVALID, "%s: the scene refracts between tabulated materials: the bundle needs wavelengths and the %d materials' indices at them (trc_rays.mat)",
                        who, needs.max_mat + 1);
    if (needs.poly && lay->W < 2)
        return trc_fail(TRC_ERR_INVALID, "%s: a polychromatic wall needs rays with spectra of at least two samples (trc_rays.spectra, spec_wl)", who);
    return TRC_OK;
}

// the carried columns of a bundle in the order of PayLayout's rows: Im of the index, materials, sample wavelengths, spectra
struct CarriedBlock { const double *src; int rows; };
static void carried_blocks(const trc_rays *in, const PayLayout &lay, CarriedBlock blk[4]) {
    blk[0] = {in->ref_index_im, 1};
    blk[1] = {in->mat, 2 * lay.n_mat};
    blk[2] = {lay.W ? in->spec_wl : nullptr, lay.W};
    blk[3] = {lay.W ? in->spectra : nullptr, lay.W};
}

// `rows` rows of a carried column to the device block `dst`: in->n apart where they come from, n apart there
static int stage_carried(double *dst, const double *src, int rows, int64_t n, const trc_rays *in) {
    if (rows <= 0 || n <= 0) return TRC_OK;
    if (hipMemcpy2D(dst, (size_t)n * 8, src, (size_t)in->n * 8, (size_t)n * 8, (size_t)rows,
                    in->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) != hipSuccess)
        return trc_fail(TRC_ERR_DEVICE, "upload of the carried columns failed");
    return TRC_OK;
}

// ================================================================================================
// fast engine
// ================================================================================================
// One call: its arguments, and what its steps hand one another
struct FastCall {
    // the arguments of trc_trace_fast_x (src as source_resolve left it)
    trc_scene *sc; const trc_rays *in; const trc_source_desc *src; const SourceSpectrum *spec;
    int64_t n; int32_t reps; double min_energy; uint64_t seed, ray_offset; int32_t flags; trc_rays *last;
    EngineState *eng;   // fast_steps: what the engines keep on the scene
    // fast_check_args: the knobs (facts.knobs), whether the rays carry more than the megakernel knows, and what; fast_facts: the rest
    // of what the choice of kernels reads (trc_forms.h)
    trc_source_desc src_res;
    trc_facts facts;
    bool carry;
    bool mat_dev;       // the materials' indices come from the scene's tables (scene_mat_route)
    PayLayout lay;
    // fast_stage_inputs: the bundle and its carried columns (the caller's own when they are on the device, else copies held
    // here), or the source descriptor and its spectrum
    DevRays dr;
    double *carry_d[4];
    DevBuf<double> carry_own[4];
    const trc_source_desc *d_src;
    const double *d_spec;
    // fast_stage_last (d_last_x: spectra of the rays left, for a source that carries its spectrum, kept on the scene as d_last is;
    // last_wl: their sample wavelengths, for a caller that wants the grid tiled)
    double *d_last[7];
    int64_t last_cap;
    double *d_last_x;
    DevBuf<double> last_wl;
    // fast_begin
    CounterValues before;
    int64_t dirty_before;
    bool captures;
    double *hit_x;
    // segments and hits: counted on the host by the streaming form, else the difference of the tallies from tally_before
    bool stream_counts_known;
    double stream_seg, stream_hits, tally_before[2];
    trc_trace_stats s;
};

static int fast_check_args(FastCall &C) {
    trc_scene *sc = C.sc;
    if (!sc) return trc_fail(TRC_ERR_INVALID, "scene is NULL");
    if ((C.in == nullptr) == (C.src == nullptr)) return trc_fail(TRC_ERR_INVALID, "exactly one of `in` and `src` must be given");
    if (C.n < 0 || C.reps < 0) return trc_fail(TRC_ERR_INVALID, "n and reps must be >= 0");
    TRC_TRY(source_resolve(sc->ctx, C.src, C.src_res, "trc_trace_fast"));
    // Optics that send two rays on from a hit are traced by the streaming form alone (k_s_shade_x<.., SPLIT>), as rays that carry
    // more are: not by the megakernel, not in calls too small for that form, and not under a source with a spectrum -- unless the
    // scene's materials are on the device: the MAT instances of k_s_shade_x are the ones that draw wavelengths.
    const bool mat_dev = scene_mat_route(sc, C.in);
    const int carried_W = C.spec->carried();
    if (sc->surfaces.splits() && ((C.flags & TRC_TRACE_MEGAKERNEL) || C.n < 64 || (C.spec->desc && !mat_dev && !carried_W)))
        return trc_fail(TRC_ERR_UNSUPPORTED, "the scene has ray-splitting optics, which the fast engine traces in its streaming form only (64 rays or more, no source spectrum): use trc_trace_ordered");
    C.facts.knobs = stream_knobs();
    // Rays that carry the imaginary part of a complex index, materials evaluated at their wavelength or a sampled spectrum are
    // traced by the streaming form (k_s_shade_x); the megakernel knows nothing of them.
    // ... and so are the rays of a source that carries its spectrum (k_s_shade_p)
    C.carry = sc->surfaces.needs().any() || (C.in && (C.in->ref_index_im || C.in->spectra || C.in->mat)) || carried_W > 0;
    if (C.carry && !C.in && !mat_dev && !carried_W) return trc_fail(TRC_ERR_UNSUPPORTED, "the scene has optics that read what only the rays of a given bundle carry (materials, spectra)");
    TRC_TRY(check_carried(sc, C.in, C.spec->desc != nullptr, carried_W, "trc_trace_fast", &C.lay, &C.mat_dev));
    if (C.carry && ((C.flags & TRC_TRACE_MEGAKERNEL) || C.n < 64))
        return trc_fail(TRC_ERR_UNSUPPORTED, "complex refractive indices and spectra travel with the streaming form of the fast engine (64 rays or more) and with trc_trace_ordered");
    return TRC_OK;
}

static int fast_stage_inputs(FastCall &C) {
    if (!C.in) {
        if (C.spec->desc) TRC_TRY(scene_stage_spectrum(*C.eng, *C.spec, &C.d_spec));
        TRC_TRY(source_kind_check(C.src));
        return C.eng->staged.source(C.src, &C.d_src);
    }
    TRC_TRY(check_rays(C.in, C.n, "trc_trace_fast"));
    TRC_TRY(stage_rays(C.in, C.n, true, &C.dr));
    if (!C.carry) return TRC_OK;
    CarriedBlock blk[4];
    carried_blocks(C.in, C.lay, blk);
    for (int b = 0; b < 4; ++b) {
        if (!blk[b].src || blk[b].rows <= 0) continue;
        if (C.in->on_device && C.in->n == C.n) { C.carry_d[b] = (double *)blk[b].src; continue; }
        TRC_TRY(C.carry_own[b].alloc((size_t)blk[b].rows * (size_t)C.n));
        C.carry_d[b] = C.carry_own[b].get();
        TRC_TRY(stage_carried(C.carry_d[b], blk[b].src, blk[b].rows, C.n, C.in));
    }
    return TRC_OK;
}

// the device side of the `last` bundle, kept on the scene between calls
static int fast_stage_last(FastCall &C) {
    EngineState &E = *C.eng;
    const trc_rays *last = C.last;
    if (!(C.flags & TRC_TRACE_KEEP_LAST)) return TRC_OK;
    if (!last || !last->x || !last->y || !last->z || !last->dx || !last->dy || !last->dz || !last->e || last->on_device)
        return trc_fail(TRC_ERR_INVALID, "TRC_TRACE_KEEP_LAST needs a host `last` bundle with x..e");
    C.last_cap = last->n;
    for (int i = 0; i < 7; ++i) {
        if (C.last_cap > 0) TRC_TRY(E.d_last[i].reserve((size_t)C.last_cap));
        C.d_last[i] = E.d_last[i].get();
    }
    // the rays left by a source that carries its spectrum bring their spectra back, when the caller made room for them
    const int W = C.spec->carried();
    if (W > 0 && last->spectra && last->n_spec == W && C.last_cap > 0) {
        const size_t need = (size_t)W * (size_t)C.last_cap;
        TRC_TRY(E.d_last_x.reserve(need));
        C.d_last_x = E.d_last_x.get();
        if (last->spec_wl) TRC_TRY(C.last_wl.alloc(need));
    }
    return TRC_OK;
}

// Where the call's counts start, and the hit buffer made ready.  Polychromatic hits: the captured ones keep their sample
// wavelengths and their spectrum before and after (3 W columns beside the hit buffer); a call whose hits would not have the shape
// of those the buffer holds is refused before anything is written.
static int fast_begin(FastCall &C) {
    trc_scene *sc = C.sc;
    TRC_TRY(sc->counters.snapshot(&C.before));
    if (sc->hits.cap > 0)
        for (int i = 0; i < sc->n_surf && !C.captures; ++i) C.captures = (sc->surfaces[i].flags & TRC_SURF_CAPTURE_HITS) != 0;
    if (C.captures) TRC_TRY(sc->hits.spectra_for(3 * C.lay.W, C.before.hit_cursor, &C.hit_x));
    C.dirty_before = sc->hits.begin_call();      // (fast_finish says how far the hit buffer was used)
    return sc->counters.restart_last(C.before);
}

static void fast_params(const FastCall &C, const MegaPlan &M, FastParams *P, CarryIn *carry_in) {
    memset(P, 0, sizeof(*P));
    P->sc = make_dscene(C.sc);
    P->x = C.dr.x; P->y = C.dr.y; P->z = C.dr.z; P->dx = C.dr.dx; P->dy = C.dr.dy; P->dz = C.dr.dz; P->e = C.dr.e;
    P->ref = C.dr.ref; P->wl = C.dr.wl; P->rid = C.dr.rid;
    P->src = C.d_src;
    P->spec = C.d_spec;
    P->n = C.n; P->reps = C.reps; P->flags = C.flags; P->min_energy = C.min_energy; P->seed = C.seed; P->ray_offset = C.ray_offset;
    P->lx = C.d_last[0]; P->ly = C.d_last[1]; P->lz = C.d_last[2]; P->ldx = C.d_last[3]; P->ldy = C.d_last[4]; P->ldz = C.d_last[5]; P->le = C.d_last[6];
    P->last_cap = C.last_cap;
    P->capture = C.captures ? 1 : 0;
    P->lds_tally = M.lds_tally; P->lds_scene = M.lds_scene;
    memset(carry_in, 0, sizeof(*carry_in));
    carry_in->hit_x = C.hit_x; carry_in->hit_x_cap = C.hit_x ? C.sc->hits.cap : 0;
    carry_in->ref_im = C.carry_d[0]; carry_in->mat = C.carry_d[1]; carry_in->spec_wl = C.carry_d[2]; carry_in->spec = C.carry_d[3];
    carry_in->n_mat = C.lay.n_mat; carry_in->n_spec = C.lay.W;
    carry_in->mat_tab = C.mat_dev ? C.sc->d_mat_tab.get() : nullptr;
    carry_in->last_spec = C.d_last_x; carry_in->last_wl = C.last_wl.get();
}

// the facts of the call for the decisions of trc_forms.h (the scene's without the pass over its surfaces; the knobs are there already)
static void fast_facts(FastCall &C) {
    C.facts.scene = scene_facts(C.sc, false);
    int poly_walls = 0;
    if (C.spec->carried())
        for (int i = 0; i < C.sc->n_surf; ++i) poly_walls += C.sc->surfaces[i].optics_kind == TRC_OPT_LAMBERTIAN_POLYCHROMATIC ? 1 : 0;
    C.facts.call = {C.n, C.flags, C.src ? C.src->kind : -1, C.d_spec != nullptr, C.carry, C.mat_dev && C.sc->d_mat_tab.get(), C.min_energy >= 0.0,
                    C.spec->carried(), poly_walls};
}

// the megakernel's instance of an id (mega_plan, trc_forms.h); null: the library has none
template <bool SPEC, bool SUN, bool CHART>
static const void *mega_kernel_of(int family, int threads) {
    if (family == TRC_K_TRACE_FAST) return threads == 256 ? (const void *)k_trace_fast<256, SPEC, SUN, CHART> : nullptr;
    return threads == 512 ? (const void *)k_trace_coop<512, SPEC, SUN, CHART> : threads == 256 ? (const void *)k_trace_coop<256, SPEC, SUN, CHART> : nullptr;
}
// ... of an arc-lamp source: k_lamp_coop, k_lamp_fast
template <bool SPEC, bool CHART>
static const void *lamp_kernel_of(int family, int threads) {
    if (family == TRC_K_LAMP_FAST) return threads == 256 ? (const void *)k_lamp_fast<256, SPEC, CHART> : nullptr;
    return threads == 512 ? (const void *)k_lamp_coop<512, SPEC, CHART> : threads == 256 ? (const void *)k_lamp_coop<256, SPEC, CHART> : nullptr;
}
static const void *mega_kernel_fn(const trc_kernel_id &id) {
    if (id.family == TRC_K_LAMP_COOP || id.family == TRC_K_LAMP_FAST) {
        const bool spec = id.a[1] != 0, chart = id.a[2] != 0;
        return spec ? (chart ? lamp_kernel_of<true, true>(id.family, id.a[0]) : lamp_kernel_of<true, false>(id.family, id.a[0]))
                    : (chart ? lamp_kernel_of<false, true>(id.family, id.a[0]) : lamp_kernel_of<false, false>(id.family, id.a[0]));
    }
    if (id.family != TRC_K_TRACE_COOP && id.family != TRC_K_TRACE_FAST) return nullptr;
    switch (4 * id.a[1] + 2 * id.a[2] + id.a[3]) {        // SPEC, SUN, CHART
    case 0: return mega_kernel_of<false, false, false>(id.family, id.a[0]);
    case 1: return mega_kernel_of<false, false, true>(id.family, id.a[0]);
    case 2: return mega_kernel_of<false, true, false>(id.family, id.a[0]);
    case 3: return mega_kernel_of<false, true, true>(id.family, id.a[0]);
    case 4: return mega_kernel_of<true, false, false>(id.family, id.a[0]);
    case 5: return mega_kernel_of<true, false, true>(id.family, id.a[0]);
    case 6: return mega_kernel_of<true, true, false>(id.family, id.a[0]);
    case 7: return mega_kernel_of<true, true, true>(id.family, id.a[0]);
    default: return nullptr;
    }
}

static int mega_launch(FastCall &C, const MegaPlan &M, const FastParams &P) {
    trc_scene *sc = C.sc;
    trc_ctx *ctx = sc->ctx;
    (void)hipStreamSynchronize(ctx->stream);       // (the sums of an earlier streaming call may still be on their way into the buffer)
    if (hipMemcpy(C.tally_before, sc->tally.device() + 3 * sc->n_surf, sizeof(C.tally_before), hipMemcpyDeviceToHost) != hipSuccess)
        return trc_fail(TRC_ERR_DEVICE, "counter readback failed");
    void (*kern)(FastParams) = (void (*)(FastParams))mega_kernel_fn(M.id);
    if (!kern) return trc_fail(TRC_ERR_UNSUPPORTED, "the library holds no megakernel instance for this call");
    // persistent grid: as many workgroups as are resident at once (at most 8 per CU), never more waves than rays/64
    unsigned resident = 0;
    TRC_TRY(kernel_grid_cap((const void *)kern, M.threads, M.lds, 8, ctx->n_cu, &resident));
    long long grid = resident;
    const long long max_grid = (C.n + M.threads - 1) / M.threads;
    if (grid > max_grid) grid = max_grid;
    if (grid < 1) grid = 1;
    if (C.n == 0) return TRC_OK;
    if (hipEventRecord(ctx->ev0, ctx->stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "event record failed");
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(M.threads), M.lds, ctx->stream, P);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "k_trace_fast launch failed: %s", hipGetErrorString(le));
    if (hipEventRecord(ctx->ev1, ctx->stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "event record failed");
    hipError_t se = hipStreamSynchronize(ctx->stream);
    if (se != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "k_trace_fast failed: %s", hipGetErrorString(se));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    C.s.kernel_ms = ms;
    C.s.launches = 1;
    return TRC_OK;
}

// the counters read back (one 64-byte copy), the stats of the call, the rays left
static int fast_finish(FastCall &C) {
    trc_scene *sc = C.sc;
    trc_trace_stats &s = C.s;
    CounterValues after = {};
    TRC_TRY(sc->counters.read_back(&after));
    sc->hits.end_call(C.dirty_before, after.hit_cursor);
    if (C.stream_counts_known) {
        s.segments = (int64_t)(C.stream_seg + 0.5);
        s.hits = (int64_t)(C.stream_hits + 0.5);
    } else {
        double tally_after[2];
        if (hipMemcpy(tally_after, sc->tally.device() + 3 * sc->n_surf, sizeof(tally_after), hipMemcpyDeviceToHost) != hipSuccess)
            return trc_fail(TRC_ERR_DEVICE, "counter readback failed");
        s.segments = (int64_t)(tally_after[0] - C.tally_before[0] + 0.5);
        s.hits = (int64_t)(tally_after[1] - C.tally_before[1] + 0.5);
    }
    s.rays_left = (int64_t)(after.rays_left - C.before.rays_left);
    s.hits_dropped = (int64_t)(after.dropped - C.before.dropped);
    s.energy_left = after.energy_left - C.before.energy_left;
    s.bounces = C.reps;
    if (C.flags & TRC_TRACE_KEEP_LAST) {
        trc_rays *last = C.last;
        const int64_t m = (int64_t)after.last_cursor;
        if (m > C.last_cap) return trc_fail(TRC_ERR_CAPACITY, "%lld rays left but `last` holds %lld", (long long)m, (long long)C.last_cap);
        double *dst[7] = {last->x, last->y, last->z, last->dx, last->dy, last->dz, last->e};
        for (int i = 0; i < 7 && m > 0; ++i) TRC_TRY(dev_download(dst[i], C.d_last[i], (size_t)m));
        double *dst_x[2] = {last->spectra, last->spec_wl};      // (rows last_cap apart on both sides)
        const double *src_x[2] = {C.d_last_x, C.last_wl.get()};
        for (int i = 0; i < 2 && m > 0; ++i)
            if (src_x[i])
                HIP_TRY(hipMemcpy2D(dst_x[i], (size_t)C.last_cap * 8, src_x[i], (size_t)C.last_cap * 8, (size_t)m * 8, (size_t)C.spec->carried(), hipMemcpyDeviceToHost));
        last->n = m;
    }
    return TRC_OK;
}

// the steps of a call after its arguments have passed, in order
static int fast_steps(FastCall &C) {
    trc_scene *sc = C.sc;
    TRC_TRY(engine_state(sc, &C.eng));
    TRC_TRY(fast_stage_inputs(C));
    TRC_TRY(fast_stage_last(C));
    TRC_TRY(fast_begin(C));
    fast_facts(C);
    const MegaPlan M = mega_plan(C.facts.scene, C.facts.call);
    FastParams P;
    CarryIn carry_in;
    fast_params(C, M, &P, &carry_in);
    const trc_engine_choice engine = trc_fast_choose_engine(C.facts.scene, C.facts.call, C.facts.knobs);
    if (engine.refused) return trc_fail(TRC_ERR_UNSUPPORTED, "no streaming form for this scene: rays that carry complex indices or spectra, and ray-splitting optics, go through trc_trace_ordered");
    if (engine.use_stream) {
        if (int e = stream_trace(sc, P, carry_in, engine.plan, C.facts, C.src, C.eng->stream_eng, &C.s, &C.stream_seg, &C.stream_hits)) {
            sc->hits.rollback(sc->counters.device() + CNT_HIT_CURSOR, C.before.hit_cursor);     // (the hits captured by the bounces that completed)
            return e;
        }
        C.stream_counts_known = true;
    } else TRC_TRY(mega_launch(C, M, P));
    return fast_finish(C);
}

static int trace_fast_impl(trc_scene *sc, const trc_rays *in, const trc_source_desc *src, const SourceSpectrum &spec, int64_t n, int32_t reps,
                           double min_energy, uint64_t seed, uint64_t ray_offset, int32_t flags, trc_rays *last,
                           trc_trace_stats *stats) {
    FastCall C = {sc, in, src, &spec, n, reps, min_energy, seed, ray_offset, flags, last};      // (the rest: zero, empty)
    TRC_TRY(fast_check_args(C));
    HIP_TRY(hipSetDevice(sc->ctx->device));
    const int st = fast_steps(C);
    if (stats) *stats = C.s;        // what the call gathered is handed back whatever its outcome
    return st;
}

// ================================================================================================
// ordered engine
// ================================================================================================
// One allocation per level (a trace of five levels used to cost 65 hipMalloc / hipFree pairs, 2 ms of a 1e5-ray call): eleven
// 8-byte columns and the surface column, each starting on a 256-byte boundary, then the carried rows (n apart, as the kernels index them).
static int level_alloc(Level &L, int64_t n, int n_pay) {
    L.n_total = n; L.n_live = n;
    const size_t m = ((size_t)(n > 0 ? n : 1) + 31) & ~(size_t)31;
    const size_t bytes = m * (11 * 8 + 4) + (n_pay > 0 ? (size_t)n * n_pay * 8 : 0);
    TRC_TRY(L.slab.alloc(bytes));
    char *slab = L.slab.get();
    double **p[9] = {&L.x, &L.y, &L.z, &L.dx, &L.dy, &L.dz, &L.e, &L.ref, &L.wl};
    for (int i = 0; i < 9; ++i) *p[i] = (double *)(slab + (size_t)i * m * 8);
    L.rid = (uint64_t *)(slab + 9 * m * 8);
    L.parent = (int64_t *)(slab + 10 * m * 8);
    L.surf = (int32_t *)(slab + 11 * m * 8);
    L.pay = n_pay > 0 ? (double *)(slab + 11 * m * 8 + m * 4) : nullptr;
    return TRC_OK;
}

extern "C" int trc_result_destroy(trc_result *res) {
    if (!res) return TRC_OK;
    (void)hipSetDevice(res->ctx->device);
    delete res;
    return TRC_OK;
}

// One call: what its steps share
struct OrdCall {
    trc_scene *sc; OrdScratch *scratch; trc_result *res; PayLayout lay; int32_t flags; double min_energy; uint64_t seed;
    trc_trace_stats s;
    float total_ms;
    const double *mat_tab;      // the scene's material tables when the rays bring no rows of them (scene_mat_route), else null
};

static void fill_f64(hipStream_t stream, long long grid, double *col, int64_t n, double v) {
    hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)grid), dim3(256), 0, stream, col, (long long)n, v);
}

// Level 0: the source bundle, generated from `src` or copied from `in` into a slab that the result owns (it outlives the call)
static int ordered_level0(OrdCall &C, const trc_rays *in, const trc_source_desc *src, const SourceSpectrum &spec, int64_t n, uint64_t ray_offset) {
    trc_ctx *ctx = C.sc->ctx;
    const PayLayout &lay = C.lay;
    Level L0;
    TRC_TRY(level_alloc(L0, n, lay.rows()));
    C.res->levels.push_back(std::move(L0));
    Level &B0 = C.res->levels.back();
    long long g0 = (n + 255) / 256; if (g0 > 8192) g0 = 8192; if (g0 < 1) g0 = 1;
    DevBuf<trc_source_desc> d_src;
    if (src) {
        double *const col[7] = {B0.x, B0.y, B0.z, B0.dx, B0.dy, B0.dz, B0.e};
        TRC_TRY(source_generate_start(ctx, src, d_src, n, C.seed, ray_offset, col, B0.rid));
        if (spec.desc) {     // level 0 carries the wavelengths the source's spectrum gives its rays, and their index
            TRC_TRY(spectrum_fill(ctx, spec.desc, spec.tab, n, C.seed, ray_offset, B0.wl, B0.ref));
            // ... or, under a carried spectrum, the sample wavelengths and spectra of a polychromatic bundle: the level's own rows
            if (spec.carried() && lay.W == spec.carried())
                TRC_TRY(carried_fill(ctx, spec.desc, spec.tab, n, n, B0.e, B0.pay + (size_t)lay.r_wl() * n, B0.pay + (size_t)lay.r_spec() * n));
        } else { fill_f64(ctx->stream, g0, B0.ref, n, 1.0); fill_f64(ctx->stream, g0, B0.wl, n, 0.0); }
        // (a scene between materials whose tables are on the device: the source's rays start with a real index)
        if (lay.has_im && n > 0 && hipMemsetAsync(B0.pay, 0, (size_t)n * 8, ctx->stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "level 0 setup failed");
    } else {
        TRC_TRY(check_rays(in, n, "trc_trace_ordered"));
        if (!in->e) return trc_fail(TRC_ERR_INVALID, "ray energies are required");
        const hipMemcpyKind kind = in->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        struct { const void *src; void *dst; } col[10] = {{in->x, B0.x}, {in->y, B0.y}, {in->z, B0.z}, {in->dx, B0.dx}, {in->dy, B0.dy}, {in->dz, B0.dz}, {in->e, B0.e},
                                                          {in->ref_index, B0.ref}, {in->wavelength, B0.wl}, {in->rid, B0.rid}};
        for (auto &c : col)
            if (c.src && n > 0 && hipMemcpy(c.dst, c.src, (size_t)n * 8, kind) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "bundle upload failed");
        if (!in->ref_index) fill_f64(ctx->stream, g0, B0.ref, n, 1.0);
        if (!in->wavelength) fill_f64(ctx->stream, g0, B0.wl, n, 0.0);
        if (!in->rid) hipLaunchKernelGGL(k_fill_rid, dim3((unsigned)g0), dim3(256), 0, ctx->stream, B0.rid, (long long)n, (unsigned long long)ray_offset);
        if (lay.rows() > 0 && n > 0) {
            CarriedBlock blk[4];
            carried_blocks(in, lay, blk);
            const int row[4] = {0, lay.r_mat(), lay.r_wl(), lay.r_spec()};
            for (int b = 0; b < 4; ++b)
                if (blk[b].src) TRC_TRY(stage_carried(B0.pay + (size_t)row[b] * n, blk[b].src, blk[b].rows, n, in));
            if (lay.has_im && !in->ref_index_im && hipMemset(B0.pay, 0, (size_t)n * 8) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "bundle upload failed");
        }
    }
    if (n > 0) {
        (void)hipMemsetAsync(B0.parent, 0, (size_t)n * 8, ctx->stream);
        (void)hipMemsetAsync(B0.surf, 0xFF, (size_t)n * 4, ctx->stream);
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "level 0 setup failed");
    return TRC_OK;
}

// k_ord_bounce's instance of an id (trc_ordered_choose, trc_forms.h); null: the library has none
template <bool CHART, bool MAT>
static const void *ord_kernel_of(int mode) {
    return mode == 2 ? (const void *)k_ord_bounce<2, CHART, MAT> : mode == 1 ? (const void *)k_ord_bounce<1, CHART, MAT>
         : mode == 0 ? (const void *)k_ord_bounce<0, CHART, MAT> : nullptr;
}
static const void *ord_kernel_fn(const trc_kernel_id &id) {
    if (id.family != TRC_K_ORD_BOUNCE || (id.a[1] && id.a[2])) return nullptr;
    return id.a[1] ? ord_kernel_of<true, false>(id.a[0]) : id.a[2] ? ord_kernel_of<false, true>(id.a[0]) : ord_kernel_of<false, false>(id.a[0]);
}

// Bounce `it` of the n_cur live rays of the last level into the 2 n_cur slots of the scratch: *m of them occupied (the rays of
// the next level), *n_culled of those below the energy threshold
static int ordered_bounce(OrdCall &C, int it, int64_t n_cur, int64_t *m, int64_t *n_culled) {
    trc_scene *sc = C.sc;
    trc_ctx *ctx = sc->ctx;
    OrdScratch &sx = *C.scratch;
    const Level &cur = C.res->levels.back();
    const int64_t slots = 2 * n_cur;
    TRC_TRY(sx.ensure((size_t)slots, C.lay.rows()));
    const long long nblk = (slots + 255) / 256;

    OrdParams P;
    memset(&P, 0, sizeof(P));
    P.sc = make_dscene(sc);
    P.x = cur.x; P.y = cur.y; P.z = cur.z; P.dx = cur.dx; P.dy = cur.dy; P.dz = cur.dz; P.e = cur.e;
    P.ref = cur.ref; P.wl = cur.wl; P.rid = cur.rid;
    P.n = n_cur; P.event = it + 1; P.flags = C.flags; P.min_energy = C.min_energy; P.seed = C.seed;
    P.ox = sx.o[0].get(); P.oy = sx.o[1].get(); P.oz = sx.o[2].get(); P.odx = sx.o[3].get(); P.ody = sx.o[4].get(); P.odz = sx.o[5].get();
    P.oe = sx.o[6].get(); P.oref = sx.o[7].get(); P.owl = sx.o[8].get(); P.orid = sx.orid.get(); P.key = sx.key.get();
    P.pay = cur.pay; P.pay_stride = cur.n_total; P.opay = sx.opay.get(); P.lay = C.lay;
    P.mat_tab = C.mat_tab;

    void (*kern)(OrdParams) = (void (*)(OrdParams))ord_kernel_fn(trc_ordered_choose(scene_facts(sc, false), C.flags, C.mat_tab != nullptr).id);
    if (!kern) return trc_fail(TRC_ERR_UNSUPPORTED, "the library holds no k_ord_bounce instance for this call");
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_cur + 255) / 256)), dim3(256), 0, ctx->stream, P);
    hipLaunchKernelGGL(k_compact_count, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, sx.key.get(), (long long)slots,
                       sx.blk_cnt.get(), sx.blk_cul.get());
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, ctx->stream, sx.blk_cnt.get(), sx.blk_cul.get(), nblk, sx.blk_off.get(),
                       sx.totals.get());
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    unsigned long long totals[2];
    hipError_t ce = hipMemcpyAsync(totals, sx.totals.get(), sizeof(totals), hipMemcpyDeviceToHost, ctx->stream);
    hipError_t se = hipStreamSynchronize(ctx->stream);
    if (ce != hipSuccess || se != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "bounce %d failed: %s", it, hipGetErrorString(se != hipSuccess ? se : ce));
    float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1); C.total_ms += ms;
    C.s.launches += 3;
    C.s.segments += n_cur;
    C.s.bounces = it + 1;
    *m = (int64_t)totals[0]; *n_culled = (int64_t)totals[1];
    return TRC_OK;
}

// The next level from the m occupied slots of bounce `it`: compacted in slot order, sorted, gathered into a slab of its own
static int ordered_next_level(OrdCall &C, int it, int64_t n_cur, int64_t m, int64_t n_culled) {
    trc_scene *sc = C.sc;
    trc_ctx *ctx = sc->ctx;
    OrdScratch &sx = *C.scratch;
    const int64_t slots = 2 * n_cur;
    hipLaunchKernelGGL(k_compact_scatter, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, ctx->stream, sx.key.get(), (long long)slots,
                       sx.blk_off.get(), sx.ckey.get(), sx.cslot.get());
    // stable sort by (culled, surface, block); slot order (= parent order) is kept inside a key
    size_t tmp_bytes = 0;
    hipError_t re = dev_sort_pairs_u32(nullptr, tmp_bytes, sx.ckey.get(), sx.skey.get(), sx.cslot.get(), sx.sslot.get(), (size_t)m, 31, ctx->stream);
    if (re != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "radix_sort_pairs(size query) failed: %s", hipGetErrorString(re));
    TRC_TRY(sx.sort_tmp.reserve(std::max(tmp_bytes, (size_t)1)));
    re = dev_sort_pairs_u32(sx.sort_tmp.get(), tmp_bytes, sx.ckey.get(), sx.skey.get(), sx.cslot.get(), sx.sslot.get(), (size_t)m, 31, ctx->stream);
    if (re != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "radix_sort_pairs failed: %s", hipGetErrorString(re));
    Level next;
    TRC_TRY(level_alloc(next, m, C.lay.rows()));
    next.n_live = m - n_culled;
    C.res->levels.push_back(std::move(next));
    const Level &Ln = C.res->levels.back();
    GatherParams G;
    G.ox = sx.o[0].get(); G.oy = sx.o[1].get(); G.oz = sx.o[2].get(); G.odx = sx.o[3].get(); G.ody = sx.o[4].get(); G.odz = sx.o[5].get();
    G.oe = sx.o[6].get(); G.oref = sx.o[7].get(); G.owl = sx.o[8].get(); G.orid = sx.orid.get(); G.skey = sx.skey.get(); G.sslot = sx.sslot.get();
    G.m = m; G.n_parent = n_cur;
    G.x = Ln.x; G.y = Ln.y; G.z = Ln.z; G.dx = Ln.dx; G.dy = Ln.dy; G.dz = Ln.dz; G.e = Ln.e; G.ref = Ln.ref;
    G.wl = Ln.wl; G.rid = Ln.rid; G.parent = Ln.parent; G.surf = Ln.surf;
    { const DScene d = make_dscene(sc); G.recs = d.recs; G.stride = d.stride; }
    G.opay = sx.opay.get(); G.pay = Ln.pay; G.n_pay = C.lay.rows();
    hipLaunchKernelGGL(k_ord_gather, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, G);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (se != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "ordering of bounce %d failed: %s", it, hipGetErrorString(se));
    C.s.launches += 3;
    C.s.hits += m;
    return TRC_OK;
}

// level 0, then a level per bounce until none is left or the bundle is depleted
static int ordered_steps(OrdCall &C, const trc_rays *in, const trc_source_desc *src, const SourceSpectrum &spec, int64_t n, int32_t reps, uint64_t ray_offset) {
    TRC_TRY(ordered_level0(C, in, src, spec, n, ray_offset));
    int64_t n_cur = n;
    for (int it = 0; it < reps && n_cur > 0; ++it) {
        int64_t m = 0, n_culled = 0;
        TRC_TRY(ordered_bounce(C, it, n_cur, &m, &n_culled));
        if (m == 0) { n_cur = 0; break; }   // "Ray bundle depleted": nothing recorded (tracer_engine.py:271, :277)
        TRC_TRY(ordered_next_level(C, it, n_cur, m, n_culled));
        n_cur = m - n_culled;
    }
    C.s.rays_left = n_cur;
    C.s.kernel_ms = C.total_ms;
    if (n_cur > 0) {
        // energy of the live part of the last level
        std::vector<double> eh((size_t)n_cur);
        if (hipMemcpy(eh.data(), C.res->levels.back().e, (size_t)n_cur * 8, hipMemcpyDeviceToHost) == hipSuccess)
            for (double v : eh) C.s.energy_left += v;
    }
    return TRC_OK;
}

static int trace_ordered_impl(trc_scene *sc, const trc_rays *in, const trc_source_desc *src, const SourceSpectrum &spec, int64_t n, int32_t reps,
                              double min_energy, uint64_t seed, uint64_t ray_offset, int32_t flags, trc_result **out, trc_trace_stats *stats) {
    if (!sc || !out) return trc_fail(TRC_ERR_INVALID, "trc_trace_ordered: bad arguments");
    *out = nullptr;
    if ((in == nullptr) == (src == nullptr)) return trc_fail(TRC_ERR_INVALID, "exactly one of `in` and `src` must be given");
    if (n < 0 || reps < 0) return trc_fail(TRC_ERR_INVALID, "n and reps must be >= 0");
    trc_source_desc src_res;
    TRC_TRY(source_resolve(sc->ctx, src, src_res, "trc_trace_ordered"));
    if (2 * n >= (int64_t)0xFFFFFFFFll) return trc_fail(TRC_ERR_UNSUPPORTED, "ordered engine handles fewer than 2^31 rays per call");
    if ((flags & TRC_TRACE_ACCEL) && !sc->kd.has()) return trc_fail(TRC_ERR_INVALID, "TRC_TRACE_ACCEL without a Kd-tree on the scene");
    if (sc->n_surf >= (1 << 28)) return trc_fail(TRC_ERR_UNSUPPORTED, "too many surfaces for the ordering key");
    HIP_TRY(hipSetDevice(sc->ctx->device));
    // what the rays carry beyond the nine columns (complex indices, material rows, spectra); rays between materials carry Im of the
    // index whether the bundle brought it or not
    PayLayout lay;
    bool mat_dev = false;
    TRC_TRY(check_carried(sc, in, spec.desc != nullptr, spec.carried(), "trc_trace_ordered", &lay, &mat_dev));
    lay.has_im = ((in && in->ref_index_im) || sc->surfaces.needs().max_mat >= 0) ? 1 : 0;
    std::unique_ptr<trc_result> res(new (std::nothrow) trc_result());
    if (!res) return trc_fail(TRC_ERR_NOMEM, "out of host memory");
    res->ctx = sc->ctx;
    res->lay = lay;
    // the scratch of the bounce loop stays with the scene (an ordered trace of 1e7 rays allocated and freed 3 GB in twenty blocks
    // beyond the pool's sizes per call: 30 of its 45 ms)
    EngineState *E;
    TRC_TRY(engine_state(sc, &E));
    OrdCall C = {sc, &E->ord_scratch, res.get(), lay, flags, min_energy, seed};      // (stats and time: zero)
    C.mat_tab = mat_dev ? sc->d_mat_tab.get() : nullptr;
    const int st = ordered_steps(C, in, src, spec, n, reps, ray_offset);
    if (E->ord_scratch.cap_slots > ORD_SCRATCH_KEEP) E->ord_scratch = OrdScratch();      // (beyond 2^26 slots -- 10 GB -- the scratch goes back after the call)
    if (stats) *stats = C.s;        // what the call gathered is handed back whatever its outcome
    if (st != TRC_OK) return st;
    *out = res.release();
    return TRC_OK;
}

// ================================================================================================
// C-ABI: the trace entry points
// ================================================================================================
extern "C" int trc_trace_fast_x(trc_scene *sc, const trc_rays *in, const trc_source_desc *src, const trc_source_spectrum *spec,
                                int64_t n, int32_t reps, double min_energy, uint64_t seed, uint64_t ray_offset, int32_t flags,
                                trc_rays *last, trc_trace_stats *stats) {
    SourceSpectrum sp;
    TRC_TRY(source_spectrum_make(spec, in, src, "trc_trace_fast_x", &sp));
    return trace_fast_impl(sc, in, src, sp, n, reps, min_energy, seed, ray_offset, flags, last, stats);
}

extern "C" int trc_trace_fast(trc_scene *sc, const trc_rays *in, const trc_source_desc *src, int64_t n, int32_t reps,
                              double min_energy, uint64_t seed, uint64_t ray_offset, int32_t flags, trc_rays *last,
                              trc_trace_stats *stats) {
    return trc_trace_fast_x(sc, in, src, nullptr, n, reps, min_energy, seed, ray_offset, flags, last, stats);
}

extern "C" int trc_trace_ordered_x(trc_scene *sc, const trc_rays *in, const trc_source_desc *src, const trc_source_spectrum *spec,
                                   int64_t n, int32_t reps, double min_energy, uint64_t seed, uint64_t ray_offset, int32_t flags,
                                   trc_result **out, trc_trace_stats *stats) {
    if (out) *out = nullptr;
    SourceSpectrum sp;
    TRC_TRY(source_spectrum_make(spec, in, src, "trc_trace_ordered_x", &sp));
    return trace_ordered_impl(sc, in, src, sp, n, reps, min_energy, seed, ray_offset, flags, out, stats);
}

extern "C" int trc_trace_ordered(trc_scene *sc, const trc_rays *in, const trc_source_desc *src, int64_t n, int32_t reps,
                                 double min_energy, uint64_t seed, uint64_t ray_offset, int32_t flags, trc_result **out,
                                 trc_trace_stats *stats) {
    return trc_trace_ordered_x(sc, in, src, nullptr, n, reps, min_energy, seed, ray_offset, flags, out, stats);
}

extern "C" int trc_result_num_levels(trc_result *res, int32_t *n_levels) {
    if (!res || !n_levels) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    *n_levels = (int32_t)res->levels.size();
    return TRC_OK;
}

extern "C" int trc_result_level_size(trc_result *res, int32_t level, int64_t *n_total, int64_t *n_live) {
    if (!res || level < 0 || level >= (int)res->levels.size()) return trc_fail(TRC_ERR_INVALID, "level out of range");
    if (n_total) *n_total = res->levels[level].n_total;
    if (n_live) *n_live = res->levels[level].n_live;
    return TRC_OK;
}

extern "C" int trc_result_level_get(trc_result *res, int32_t level, trc_rays *out, int32_t *surf) {
    if (!res || level < 0 || level >= (int)res->levels.size() || !out) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    const Level &L = res->levels[level];
    if (out->n < L.n_total) return trc_fail(TRC_ERR_CAPACITY, "output bundle holds %lld rays, level has %lld", (long long)out->n, (long long)L.n_total);
    if (out->on_device) return trc_fail(TRC_ERR_INVALID, "host output expected");
    HIP_TRY(hipSetDevice(res->ctx->device));
    const size_t n = (size_t)L.n_total;
    const int64_t cap = out->n;
    out->n = L.n_total;
    if (n == 0) return TRC_OK;
    struct { void *dst; const void *src; size_t w; } cp[] = {
        {out->x, L.x, 8}, {out->y, L.y, 8}, {out->z, L.z, 8}, {out->dx, L.dx, 8}, {out->dy, L.dy, 8}, {out->dz, L.dz, 8},
        {out->e, L.e, 8}, {out->parent, L.parent, 8}, {out->ref_index, L.ref, 8}, {out->wavelength, L.wl, 8},
        {out->rid, L.rid, 8}, {surf, L.surf, 4}};
    for (auto &c : cp)
        if (c.dst) HIP_TRY(hipMemcpy(c.dst, c.src, n * c.w, hipMemcpyDeviceToHost));
    // what the rays carry beyond that (rows of the caller's 2-D columns: the capacity it handed over apart)
    const PayLayout &lay = res->lay;
    if (out->ref_index_im) {
        if (lay.has_im) HIP_TRY(hipMemcpy(out->ref_index_im, L.pay, n * 8, hipMemcpyDeviceToHost));
        else memset(out->ref_index_im, 0, n * 8);
    }
    if (out->spectra || out->spec_wl) {
        if (out->n_spec != lay.W) return trc_fail(TRC_ERR_INVALID, "the level's rays carry %d spectral samples, the output has room for %d", lay.W, out->n_spec);
        if (out->spec_wl && lay.W) HIP_TRY(hipMemcpy2D(out->spec_wl, (size_t)cap * 8, L.pay + (size_t)lay.r_wl() * n, n * 8, n * 8, (size_t)lay.W, hipMemcpyDeviceToHost));
        if (out->spectra && lay.W) HIP_TRY(hipMemcpy2D(out->spectra, (size_t)cap * 8, L.pay + (size_t)lay.r_spec() * n, n * 8, n * 8, (size_t)lay.W, hipMemcpyDeviceToHost));
    }
    return TRC_OK;
}
