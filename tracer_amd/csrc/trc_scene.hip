// trc_scene.hip -- the scene's part of the C-ABI of include/tracer_amd.h and what stands before it: the error string and the ABI
// version, the context, pinned host memory, and a scene from creation to destruction -- poses, Kd-tree, flux maps, the hit buffer
// and its readers (k_hits_*, k_bin_hits), the tabulated materials (k_material_eval), the tallies.  The parts of a scene and
// struct trc_scene are trc_scene.h, and the member functions that header only declares are defined here.  Nothing here traces a ray:
// the engines are trc_kernels.hip, the histograms of the captured hits trc_hithist.hip, the entry points that take no scene
// trc_protocol.hip.  The scan and the sort of the hit reader are rocprim's, instantiated once for the library (trc_host.h).
//
// No CPU fallback lives here: without a GPU every entry point fails with TRC_ERR_DEVICE.

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>

#include "trc_scene.h"

extern "C" const char *trc_last_error(void) { return g_last_error.c_str(); }
extern "C" int trc_abi_version(void) { return TRC_ABI_VERSION; }

// ================================================================================================
// the search tables (SearchTables, trc_scene.h)
// ================================================================================================
int SearchTables::build(const trc_surface_desc *surfs, int n) {
    const char *ev = getenv("TRC_GRID_FORCE32");      // (measurements: the large grid for a scene the LDS-sized one holds)
    trc_accel_host &A = accel_;
    trc_search_tables_build(surfs, n, ev && atoi(ev), A);
    // conservative single-precision boxes of the bounded surfaces
    TRC_TRY(dev_upload(d_obb_, A.obb.data(), A.obb.size()));
    TRC_TRY(dev_upload(d_bleaf_, A.brute_leaf.data(), A.brute_leaf.size()));
    TRC_TRY(dev_upload(d_sbox_, A.sbox.data(), A.sbox.size()));
    TRC_TRY(dev_upload(d_unbounded_, A.unbounded.data(), A.unbounded.size()));
    if (A.grid_ok) {
        TRC_TRY(dev_upload(d_gapart_, A.grid_apart.data(), A.grid_apart.size()));
        TRC_TRY(dev_upload(d_goff_, A.grid_off.data(), A.grid_off.size()));
        TRC_TRY(dev_upload(d_glist_, A.grid_list.data(), A.grid_list.size()));
        if (A.clear_cones > 0) TRC_TRY(dev_upload(d_clear_, A.clear.data(), A.clear.size()));
    } else if (A.big_ok) {      // a scene the LDS-sized grid cannot hold: the 32-bit grid in global memory
        TRC_TRY(dev_upload(d_bg_off_, A.big_off.data(), A.big_off.size()));
        TRC_TRY(dev_upload(d_bg_ent_, A.big_ent.data(), A.big_ent.size()));
        TRC_TRY(dev_upload(d_bg_occ_, A.big_occ.data(), A.big_occ.size()));
        std::vector<float>().swap(A.big_ent);       // (the host keeps the list itself, not its 48-byte entries)
        TRC_TRY(d_bg_apart_.alloc(A.big_apart.size() + 1));
        if (!A.big_apart.empty())
            HIP_TRY(hipMemcpy(d_bg_apart_.get(), A.big_apart.data(), A.big_apart.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    ok_ = true;
    return TRC_OK;
}

void SearchTables::fill(DScene &d) const {
    if (!ok_) return;
    const trc_accel_host &A = accel_;
    d.a_sbox = d_sbox_.get(); d.a_obb = d_obb_.get(); d.a_nodes = d_nodes_.get(); d.a_leaf = d_leaf_.get(); d.a_unbounded = d_unbounded_.get();
    d.a_n_unbounded = (int32_t)A.unbounded.size(); d.a_kd_depth = A.kd_depth;
    d.a_bleaf = d_bleaf_.get(); d.a_n_bleaf = (int32_t)A.brute_leaf.size();
    d.a_bnodes[0] = A.brute_nodes[0]; d.a_bnodes[1] = A.brute_nodes[1];
    d.a_ok = 1; d.a_kd_ok = kd_ok_ ? 1 : 0;
    d.a_delta = A.delta;
    d.a_goff = d_goff_.get(); d.a_glist = d_glist_.get(); d.a_gapart = d_gapart_.get();
    d.a_bg_off = d_bg_off_.get(); d.a_bg_occ = d_bg_occ_.get(); d.a_bg_ent = d_bg_ent_.get(); d.a_bg_ok = A.big_ok ? 1 : 0;
    d.a_bg_apart = d_bg_apart_.get(); d.a_bg_napart = A.big_ok ? (int32_t)A.big_apart.size() : 0;
    d.a_g_napart = A.grid_ok ? (int32_t)A.grid_apart.size() : 0;
    d.a_g_ok = A.grid_ok ? 1 : 0;
    d.a_g_ncell = A.grid_ok ? (int32_t)A.grid_off.size() - 1 : 0;
    d.a_g_nlist = A.grid_ok ? (int32_t)A.grid_list.size() : 0;
    for (int i = 0; i < 3; ++i) {
        d.a_bg_dim[i] = A.big_ok ? A.big_dim[i] : 1;
        d.a_bg_lo[i] = A.big_lo[i]; d.a_bg_cs[i] = A.big_cs[i]; d.a_bg_inv[i] = A.big_inv[i];
        d.a_gdim[i] = A.grid_ok ? A.grid_dim[i] : 1;
        d.a_glo[i] = A.grid_lo[i]; d.a_gcs[i] = A.grid_cs[i]; d.a_ginv[i] = A.grid_inv[i];
        d.a_cen[i] = A.cen[i]; d.a_slo[i] = A.slo[i]; d.a_shi[i] = A.shi[i];
    }
    for (int i = 0; i < 6; ++i) {
        d.a_broot[i] = A.brute_root[i]; d.a_root[i] = A.root[i];
        d.a_bg_root[i] = A.big_ok ? A.big_root[i] : 0.0f; d.a_groot[i] = A.grid_ok ? A.grid_root[i] : 0.0f;
    }
}

// ================================================================================================
// C-ABI: context
// ================================================================================================
extern "C" int trc_ctx_create(int device_id, trc_ctx **out) {
    if (!out) return trc_fail(TRC_ERR_INVALID, "trc_ctx_create: out is NULL");
    *out = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev == 0)
        return trc_fail(TRC_ERR_DEVICE, "no HIP device available (%s): this library has no CPU path",
                        e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n_dev)
        return trc_fail(TRC_ERR_INVALID, "device %d out of range (%d devices)", device_id, n_dev);
    HIP_TRY(hipSetDevice(device_id));
    trc_ctx *c = new (std::nothrow) trc_ctx();
    if (!c) return trc_fail(TRC_ERR_NOMEM, "out of host memory");
    c->device = device_id;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    c->n_cu = prop.multiProcessorCount;
    *out = c;
    return TRC_OK;
}

extern "C" int trc_ctx_destroy(trc_ctx *ctx) {
    if (!ctx) return TRC_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipEventDestroy(ctx->ev0);
    (void)hipEventDestroy(ctx->ev1);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    dev_cache().trim();   // blocks kept for reuse go back to the driver with the context
    return TRC_OK;
}

extern "C" int trc_ctx_synchronize(trc_ctx *ctx) {
    if (!ctx) return trc_fail(TRC_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TRC_OK;
}

extern "C" int trc_ctx_device_name(trc_ctx *ctx, char *buf, int buflen) {
    if (!ctx || !buf || buflen <= 0) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return TRC_OK;
}

// ================================================================================================
// C-ABI: scene
// ================================================================================================
int SceneSurfaces::create(const trc_surface_desc *surfs, int32_t n, int32_t n_extra, const double *extra) {
    stride_ = trc_scene_stride(surfs, n);
    trc_scene_scan(surfs, n, &splits_, &needs_);
    n_extra_ = n_extra;
    surfs_.assign(surfs, surfs + n);
    if (n_extra > 0 && extra) extra_h_.assign(extra, extra + n_extra);
    TRC_TRY(d_recs_.alloc((size_t)n * stride_));
    TRC_TRY(d_opt_.alloc((size_t)n * 8));
    TRC_TRY(d_sflags_.alloc((size_t)n));
    TRC_TRY(d_extra_.alloc((size_t)n_extra));
    if (n_extra > 0 && hipMemcpy(d_extra_.get(), extra_h_.data(), (size_t)n_extra * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return trc_fail(TRC_ERR_DEVICE, "extra upload failed");
    return upload();
}

int SceneSurfaces::upload() {
    const size_t n = surfs_.size();
    std::vector<double> recs(n * stride_), opt(n * 8);
    std::vector<int32_t> flags(n);
    for (size_t i = 0; i < n; ++i) {
        trc_pack_record(surfs_[i], recs.data() + i * stride_, stride_);
        for (int k = 0; k < 8; ++k) opt[i * 8 + k] = surfs_[i].opt[k];
        flags[i] = surfs_[i].flags & 0xFFFF;
        if (surface_ends_every_ray(surfs_[i])) flags[i] |= TRC_SURF_TERMINAL;
        flags[i] |= trc_shade_class_of(surfs_[i]) << TRC_SURF_CLS_SHIFT;      // which shading kernel of the streaming engine serves the surface
    }
    HIP_TRY(hipMemcpy(d_recs_.get(), recs.data(), recs.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_opt_.get(), opt.data(), opt.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_sflags_.get(), flags.data(), flags.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return TRC_OK;
}

extern "C" int trc_scene_create(trc_ctx *ctx, int32_t n_surf, const trc_surface_desc *surfs, int32_t n_extra,
                                const double *extra, trc_scene **out) {
    if (!ctx || !out || n_surf <= 0 || !surfs) return trc_fail(TRC_ERR_INVALID, "trc_scene_create: bad arguments");
    if (n_surf >= (1 << 28)) return trc_fail(TRC_ERR_INVALID, "too many surfaces");
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    for (int i = 0; i < n_surf; ++i) TRC_TRY(validate_surface(surfs[i], i, n_extra));
    std::unique_ptr<trc_scene> sc(new (std::nothrow) trc_scene());
    if (!sc) return trc_fail(TRC_ERR_NOMEM, "out of host memory");
    sc->ctx = ctx;
    sc->n_surf = n_surf;
    TRC_TRY(sc->counters.alloc());
    TRC_TRY(sc->surfaces.create(surfs, n_surf, n_extra, extra));
    TRC_TRY(sc->search.rebuild(surfs, n_surf));
    TRC_TRY(sc->tally.create(n_surf));
    *out = sc.release();
    return TRC_OK;
}

extern "C" int trc_scene_destroy(trc_scene *sc) {
    if (!sc) return TRC_OK;
    (void)hipSetDevice(sc->ctx->device);
    (void)hipStreamSynchronize(sc->ctx->stream);
    delete sc;
    return TRC_OK;
}

extern "C" int trc_scene_update_frames(trc_scene *sc, int32_t n_surf, const double *frames12) {
    if (!sc || !frames12 || n_surf != sc->n_surf) return trc_fail(TRC_ERR_INVALID, "trc_scene_update_frames: bad arguments");
    TRC_TRY(scene_quiet(sc));
    sc->surfaces.set_frames(frames12);
    sc->kd.clear();            // a Kd-tree set before described the old poses: the caller sets a new one (or does without)
    TRC_TRY(sc->surfaces.upload());
    return sc->search.rebuild(sc->surfaces.data(), n_surf);
}

extern "C" int trc_scene_set_kdtree(trc_scene *sc, const trc_kdtree_desc *kd) {
    if (!sc) return trc_fail(TRC_ERR_INVALID, "scene is NULL");
    TRC_TRY(scene_quiet(sc));
    sc->kd.clear();
    sc->search.drop_kd();
    if (!kd) return TRC_OK;
    char why[160] = "";
    int depth = 0;
    const int st = trc_kd_check(kd, sc->n_surf, &depth, why, sizeof(why));
    if (st != TRC_OK) return trc_fail(st, "trc_scene_set_kdtree: %s", why);
    if (depth > TRC_KD_STACK) return trc_fail(TRC_ERR_UNSUPPORTED, "Kd-tree depth %d exceeds the traversal stack (%d)", depth, TRC_KD_STACK);
    TRC_TRY(sc->kd.set(kd));
    return sc->search.pack_kd(kd);
}

extern "C" int trc_scene_set_fluxmap(trc_scene *sc, int32_t surf, int32_t nu, int32_t nv, const double *u_edges,
                                           const double *v_edges, const double *proj12) {
    return trc_scene_set_fluxmap_chart(sc, surf, TRC_FM_XY, nu, nv, u_edges, v_edges, proj12);
}

extern "C" int trc_scene_set_fluxmap_chart(trc_scene *sc, int32_t surf, int32_t chart, int32_t nu, int32_t nv, const double *u_edges,
                                                 const double *v_edges, const double *proj12) {
    if (!sc || surf < 0 || surf >= sc->n_surf || nu <= 0 || nv <= 0 || !u_edges || !v_edges || !proj12)
        return trc_fail(TRC_ERR_INVALID, "trc_scene_set_fluxmap_chart: bad arguments");
    if (chart < 0 || chart >= TRC_FM_CHARTS) return trc_fail(TRC_ERR_INVALID, "trc_scene_set_fluxmap_chart: unknown chart %d", chart);
    TRC_TRY(scene_quiet(sc));
    for (int i = 0; i < nu; ++i) if (!(u_edges[i + 1] > u_edges[i])) return trc_fail(TRC_ERR_INVALID, "u edges must increase");
    for (int i = 0; i < nv; ++i) if (!(v_edges[i + 1] > v_edges[i])) return trc_fail(TRC_ERR_INVALID, "v edges must increase");
    return sc->tally.add_map(surf, chart, nu, nv, u_edges, v_edges, proj12);     // resets the tallies
}

extern "C" int trc_scene_set_hit_capacity(trc_scene *sc, int64_t capacity) {
    if (!sc || capacity < 0) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    TRC_TRY(scene_quiet(sc));
    TRC_TRY(sc->counters.restart_hits());
    return sc->hits.set_capacity(capacity);
}

int HitBuffer::set_capacity(int64_t capacity) {
    // the same capacity again (an engine sizes the buffer before every trace): the buffer is kept and emptied -- freeing and
    // allocating 15 GB per call was a tenth of a second at 1e8 rays
    if (capacity > 0 && capacity == cap_user) return reset();
    const uint32_t e = epoch + 1;
    *this = HitBuffer();      // (spectral columns are made again by the next call that brings spectra)
    epoch = e;
    if (capacity == 0) return TRC_OK;
    // The streaming engine appends in chunks that stay open between launches: room for what they can leave unused.  The chunk
    // follows the buffer -- 1024 entries per atomic for the buffers of full-size runs (the cursor is one word), less for modest
    // ones -- and the slack is what every wave that can hold an open chunk may leave unused of one: a call whose hits fit the
    // capacity asked for never drops one, whatever its size.
    int64_t ch = 64;          // (never below a wave's worth: one append of a wave must fit a fresh chunk)
    while (ch < SQ_HIT_CHUNK && 2048 * (ch * 2) <= capacity) ch *= 2;
    chunk = (uint32_t)ch;
    return allocate(capacity, TRC_HIT_HOLDERS * ch + 64, 0);
}

// Columns for `capacity` hits + `slack`, holding entries [0, keep) of the present ones, spectral ones included.
int HitBuffer::allocate(int64_t capacity, int64_t slack, int64_t keep) {
    const int64_t alloc = capacity + slack;
    // the new columns join the buffer once they hold its hits
    DevBuf<int32_t> n_surf;
    DevBuf<double> n_col[8], n_x;
    TRC_TRY(n_surf.alloc((size_t)alloc));
    for (auto &c : n_col) TRC_TRY(c.alloc((size_t)alloc));
    if (x_cols > 0) TRC_TRY(n_x.alloc((size_t)x_cols * (size_t)alloc));
    HIP_TRY(unwrite(n_surf.get(), alloc));
    if (keep > 0) {
        HIP_TRY(hipMemcpy(n_surf.get(), surf.get(), (size_t)keep * sizeof(int32_t), hipMemcpyDeviceToDevice));
        for (int i = 0; i < 8; ++i) HIP_TRY(hipMemcpy(n_col[i].get(), col[i].get(), (size_t)keep * sizeof(double), hipMemcpyDeviceToDevice));
        if (x_cols > 0)
            HIP_TRY(hipMemcpy2D(n_x.get(), (size_t)alloc * sizeof(double), x.get(), (size_t)cap * sizeof(double), (size_t)keep * sizeof(double),
                                (size_t)x_cols, hipMemcpyDeviceToDevice));
    }
    surf = std::move(n_surf);
    for (int i = 0; i < 8; ++i) col[i] = std::move(n_col[i]);
    x = std::move(n_x);
    dirty_to = keep;
    cap = alloc;
    cap_user = capacity;
    return TRC_OK;
}

// A buffer of at least `capacity` hits that keeps what it holds: the accountants of a script that traces again before it has
// read the hits of its last call (optics_callables.py:1577-1643 accumulate over calls) are served from the device when they are
// read at last.
extern "C" int trc_scene_reserve_hits(trc_scene *sc, int64_t capacity) {
    if (!sc || capacity < 0) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    if (sc->hits.cap_user == 0) return trc_scene_set_hit_capacity(sc, capacity);
    if (capacity <= sc->hits.cap_user) return TRC_OK;
    unsigned long long cursor;
    TRC_TRY(scene_hit_cursor(sc, &cursor));
    return sc->hits.grow(capacity, cursor);
}

// entries of the hit buffer reserved so far (written ones and the unused parts of chunks still open) and its capacity
extern "C" int trc_scene_hits_reserved(trc_scene *sc, int64_t *reserved, int64_t *capacity) {
    if (!sc) return trc_fail(TRC_ERR_INVALID, "scene is NULL");
    if (reserved) {
        unsigned long long c;
        TRC_TRY(sc->counters.stale() ? scene_hit_cursor(sc, &c) : sc->counters.hit_cursor(&c));      // (no wait while the mirror is valid)
        *reserved = (int64_t)c;
    }
    if (capacity) *capacity = sc->hits.cap_user;
    return TRC_OK;
}

// Page-locked host memory for large results (hit lists, levels of the ray tree): a device-to-host copy into pageable memory is
// staged through the driver's own bounce buffers at a third of the rate.  The same block cache as device memory, under a policy of
// its own: every block classed, at most 4 GiB idle, nothing to wait for, and a pointer that is not one of its blocks refused.
struct HostBackend {
    static inline thread_local hipError_t err = hipSuccess;
    void *alloc(size_t bytes) {
        void *p = nullptr;
        err = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (err == hipSuccess) return p;
        (void)hipGetLastError();
        return nullptr;
    }
    void release(void *p) { (void)hipHostFree(p); }
    void quiesce() {}
    int device() { return 0; }
};
static trc_block_cache<HostBackend> g_host_cache({SIZE_MAX, (size_t)4 << 30, 0, false, false}, true);

extern "C" int trc_host_alloc(int64_t bytes, void **out) {
    if (!out || bytes < 0) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    *out = g_host_cache.alloc((size_t)bytes);
    if (!*out) return trc_fail(TRC_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", trc_pool_class((size_t)bytes), hipGetErrorString(HostBackend::err));
    return TRC_OK;
}

extern "C" int trc_host_free(void *p) {
    if (p && g_host_cache.free(p) == TRC_POOL_UNKNOWN) return trc_fail(TRC_ERR_INVALID, "trc_host_free: not a block of trc_host_alloc");
    return TRC_OK;
}

extern "C" int trc_scene_clear_hits(trc_scene *sc) {
    if (!sc) return trc_fail(TRC_ERR_INVALID, "scene is NULL");
    return trc_scene_set_hit_capacity(sc, sc->hits.cap_user);       // (the same capacity: the buffer is kept and emptied)
}

extern "C" int trc_scene_reset_tallies(trc_scene *sc) {
    if (!sc) return trc_fail(TRC_ERR_INVALID, "scene is NULL");
    TRC_TRY(scene_quiet(sc));
    TRC_TRY(sc->tally.zero());
    TRC_TRY(sc->counters.zero());
    return sc->hits.reset();
}

extern "C" int trc_scene_get_tallies(trc_scene *sc, double *absorbed, double *received, int64_t *hits) {
    if (!sc) return trc_fail(TRC_ERR_INVALID, "scene is NULL");
    TRC_TRY(scene_quiet(sc));
    const int S = sc->n_surf;
    std::vector<double> t((size_t)3 * S);
    HIP_TRY(hipMemcpy(t.data(), sc->tally.device(), t.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < S; ++i) {
        if (absorbed) absorbed[i] = t[i];
        if (received) received[i] = t[S + i];
        if (hits) hits[i] = (int64_t)(t[2 * S + i] + 0.5);
    }
    return TRC_OK;
}

extern "C" int trc_scene_get_fluxmap(trc_scene *sc, int32_t surf, double *out) {
    if (!sc || surf < 0 || surf >= sc->n_surf || !out) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    const FluxMapDev *m = sc->tally.map_of(surf);
    if (!m) return trc_fail(TRC_ERR_INVALID, "surface %d has no flux map", surf);
    TRC_TRY(scene_quiet(sc));
    HIP_TRY(hipMemcpy(out, sc->tally.device() + m->bins, (size_t)m->nu * m->nv * sizeof(double), hipMemcpyDeviceToHost));
    return TRC_OK;
}

// written entries of the hit buffer (surface >= 0) packed to the front, in buffer order: flags -> exclusive scan -> scatter
__global__ __launch_bounds__(256) void k_hits_flag(const int32_t *surf, long long n, uint32_t *flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = surf[i] >= 0 ? 1u : 0u;
}
struct HitPack {
    const int32_t *surf;
    const double *col[8];
    int32_t *o_surf;
    double *o_col[8];
    int want[8];
    const int32_t *sflags;      // TRC_SURF_CAPTURE_LEAN: columns 1 (incident energy) and 5-7 (direction) of the hit were not written
    const double *x;            // n_x more columns (spectra), column k at x + k * x_cap; packed to o_x + k * o_cnt
    double *o_x;
    int n_x;
    long long x_cap, o_cnt;
};
// entry i of the buffer, of surface s, to place o of the output: the wanted columns, those a lean capture left unwritten made up
// (the incident energy is the absorbed one, the direction zero), the spectral columns
__device__ __forceinline__ void hits_copy_entry(const HitPack &H, long long i, long long o, int32_t s) {
    H.o_surf[o] = s;
#pragma unroll
    for (int k = 0; k < 8; ++k) if (H.want[k]) H.o_col[k][o] = H.col[k][i];
    if (H.sflags[s] & TRC_SURF_CAPTURE_LEAN) {
        if (H.want[1]) H.o_col[1][o] = H.col[0][i];
#pragma unroll
        for (int k = 5; k < 8; ++k) if (H.want[k]) H.o_col[k][o] = 0.0;
    }
    for (int k = 0; k < H.n_x; ++k) H.o_x[(long long)k * H.o_cnt + o] = H.x[(long long)k * H.x_cap + i];
}
__global__ __launch_bounds__(256) void k_hits_pack(HitPack H, const uint32_t *offs, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s = H.surf[i];
    if (s < 0) return;
    hits_copy_entry(H, i, offs[i], s);
}

// The same, surface by surface: entry src[o] of the buffer goes to place o (src = the entries sorted by surface, stably).
__global__ __launch_bounds__(256) void k_hits_keys(const int32_t *surf, long long n, uint32_t none, uint32_t *key, uint32_t *entry) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s = surf[i];
    key[i] = s < 0 ? none : (uint32_t)s;          // unwritten entries of open chunks sort behind every surface
    entry[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_hits_gather(HitPack H, const uint32_t *src, long long cnt) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= cnt) return;
    const uint32_t i = src[o];
    hits_copy_entry(H, i, o, H.surf[i]);
}

static int scene_get_hits(trc_scene *sc, int64_t *n, int32_t *surf, double *e_abs, double *e_in, double *px,
                          double *py, double *pz, double *dx, double *dy, double *dz, int32_t n_x, double *x_out) {
    if (!sc || !n) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    if (n_x < 0 || (n_x > 0 && (!x_out || n_x != sc->hits.x_cols)))
        return trc_fail(TRC_ERR_INVALID, "trc_scene_get_hits_x: the hit buffer holds %d spectral columns, %d asked for", sc->hits.x_cols, n_x);
    unsigned long long cursor;
    TRC_TRY(scene_hit_cursor(sc, &cursor));
    double *const dst[8] = {e_abs, e_in, px, py, pz, dx, dy, dz};
    return sc->hits.read(sc->ctx->stream, sc->surfaces.all(), make_dscene(sc).sflags, cursor, n, surf, dst, n_x, x_out);
}

// the written entries of [0, cursor): n of them, and the columns whose destinations are given
int HitBuffer::read(hipStream_t stream, const std::vector<trc_surface_desc> &surfs, const int32_t *d_sflags, unsigned long long cursor,
                    int64_t *n, int32_t *surf_out, double *const dst[8], int32_t n_x, double *x_out) const {
    const int64_t reserved = used(cursor);
    *n = 0;
    if (reserved == 0) return TRC_OK;
    if (reserved >= (1ll << 32)) return trc_fail(TRC_ERR_CAPACITY, "more than 2^32 entries in the hit buffer");
    // The reserved range holds unwritten entries (surface -1) where the streaming engine's chunks are still open: the caller
    // gets the written ones, in buffer order (one capturing surface) or surface by surface (several).  They are packed on the device (copying the whole range and picking on the
    // host was 0.11 s for the 6.5e6 receiver hits of an NSTTF step).
    DevBuf<uint32_t> d_flag, d_off, d_key[2], d_ent[2];
    DevBuf<char> d_tmp;
    DevBuf<int32_t> o_surf;
    DevBuf<double> o_col[8], o_x;
    // declared after the temporaries, so it runs before they are freed: nothing queued on the stream may still use them
    struct StreamWait { hipStream_t s; ~StreamWait() { (void)hipStreamSynchronize(s); } } wait_before_free{stream};
    TRC_TRY(d_flag.alloc((size_t)reserved));
    TRC_TRY(d_off.alloc((size_t)reserved));
    const unsigned nblk = (unsigned)((reserved + 255) / 256);
    hipLaunchKernelGGL(k_hits_flag, dim3(nblk), dim3(256), 0, stream, surf.get(), (long long)reserved, d_flag.get());
    size_t tmp_bytes = 0;
    if (dev_exclusive_scan_u32(nullptr, tmp_bytes, d_flag.get(), d_off.get(), (size_t)reserved, stream) != hipSuccess)
        return trc_fail(TRC_ERR_DEVICE, "exclusive_scan (size query) failed");
    TRC_TRY(d_tmp.alloc(tmp_bytes ? tmp_bytes : 1));
    if (dev_exclusive_scan_u32(d_tmp.get(), tmp_bytes, d_flag.get(), d_off.get(), (size_t)reserved, stream) != hipSuccess)
        return trc_fail(TRC_ERR_DEVICE, "exclusive_scan failed");
    uint32_t last_off = 0, last_flag = 0;
    if (hipMemcpyAsync(&last_off, d_off.get() + (reserved - 1), 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(&last_flag, d_flag.get() + (reserved - 1), 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "hit count readback failed");
    const int64_t cnt = (int64_t)last_off + (int64_t)last_flag;
    *n = cnt;
    if (cnt == 0 || (!surf_out && !dst[0] && !dst[1] && !dst[2] && !dst[3] && !dst[4] && !dst[5] && !dst[6] && !dst[7])) return TRC_OK;
    HitPack H;
    memset(&H, 0, sizeof(H));
    H.surf = surf.get();
    H.sflags = d_sflags;
    TRC_TRY(o_surf.alloc((size_t)cnt));
    H.o_surf = o_surf.get();
    for (int k = 0; k < 8; ++k) {
        H.col[k] = col[k].get();
        H.want[k] = dst[k] ? 1 : 0;
        if (dst[k]) { TRC_TRY(o_col[k].alloc((size_t)cnt)); H.o_col[k] = o_col[k].get(); }
    }
    if (n_x > 0) {
        H.x = x.get(); H.n_x = n_x; H.x_cap = cap; H.o_cnt = cnt;
        TRC_TRY(o_x.alloc((size_t)cnt * (size_t)n_x));
        H.o_x = o_x.get();
    }
    int n_capture = 0;
    for (const trc_surface_desc &d : surfs) if (d.flags & TRC_SURF_CAPTURE_HITS) ++n_capture;
    if (n_capture <= 1) {
        hipLaunchKernelGGL(k_hits_pack, dim3(nblk), dim3(256), 0, stream, H, (const uint32_t *)d_off.get(), (long long)reserved);
    } else {
        // Several capturing surfaces: the caller wants each one's hits together (accountants), and regrouping eight columns
        // on the host cost 60 ms per 1e6 hits.  A stable radix sort of (surface, entry) pairs over the bits a surface index
        // needs, then one gather: surface by surface, buffer order inside a surface, unwritten entries behind all of them.
        TRC_TRY(d_key[0].alloc((size_t)reserved));
        TRC_TRY(d_key[1].alloc((size_t)reserved));
        TRC_TRY(d_ent[0].alloc((size_t)reserved));
        TRC_TRY(d_ent[1].alloc((size_t)reserved));
        uint32_t *key0 = d_key[0].get(), *key1 = d_key[1].get(), *ent0 = d_ent[0].get(), *ent1 = d_ent[1].get();
        hipLaunchKernelGGL(k_hits_keys, dim3(nblk), dim3(256), 0, stream, surf.get(), (long long)reserved, (uint32_t)surfs.size(),
                           key0, ent0);
        unsigned bits = 1;
        while ((1u << bits) <= (unsigned)surfs.size()) ++bits;
        size_t sort_bytes = 0;
        if (dev_sort_pairs_u32(nullptr, sort_bytes, key0, key1, ent0, ent1, (size_t)reserved, bits, stream) != hipSuccess)
            return trc_fail(TRC_ERR_DEVICE, "radix_sort_pairs (size query) failed");
        TRC_TRY(d_tmp.alloc(sort_bytes ? sort_bytes : 1));
        if (dev_sort_pairs_u32(d_tmp.get(), sort_bytes, key0, key1, ent0, ent1, (size_t)reserved, bits, stream) != hipSuccess)
            return trc_fail(TRC_ERR_DEVICE, "radix_sort_pairs failed");
        hipLaunchKernelGGL(k_hits_gather, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, H, (const uint32_t *)ent1, (long long)cnt);
    }
    // one copy per column, all behind the packing on the context's stream (page-locked destinations -- trc_host_alloc -- take
    // them at the rate of the link), one wait
    if (surf_out && hipMemcpyAsync(surf_out, H.o_surf, (size_t)cnt * 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "memcpy failed");
    for (int k = 0; k < 8; ++k)
        if (dst[k] && hipMemcpyAsync(dst[k], H.o_col[k], (size_t)cnt * 8, hipMemcpyDeviceToHost, stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "memcpy failed");
    if (n_x > 0 && hipMemcpyAsync(x_out, H.o_x, (size_t)cnt * (size_t)n_x * 8, hipMemcpyDeviceToHost, stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "memcpy failed");
    if (hipStreamSynchronize(stream) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "fetching the hits failed");
    return TRC_OK;
}

extern "C" int trc_scene_get_hits(trc_scene *sc, int64_t *n, int32_t *surf, double *e_abs, double *e_in, double *px,
                                  double *py, double *pz, double *dx, double *dy, double *dz) {
    return scene_get_hits(sc, n, surf, e_abs, e_in, px, py, pz, dx, dy, dz, 0, nullptr);
}

extern "C" int trc_scene_get_hits_x(trc_scene *sc, int64_t *n, int32_t *surf, double *e_abs, double *e_in, double *px,
                                    double *py, double *pz, double *dx, double *dy, double *dz, int32_t n_x, double *x) {
    return scene_get_hits(sc, n, surf, e_abs, e_in, px, py, pz, dx, dy, dz, n_x, x);
}

extern "C" int trc_scene_hit_spectral_columns(trc_scene *sc, int32_t *n_x) {
    if (!sc || !n_x) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    *n_x = sc->hits.x_cols;
    return TRC_OK;
}

// ---- the scene's tabulated materials on the device ----------------------------------------------------------------------------
// m_k(wl[i]) of every material of the table: Re at out[2k * n + i], Im at out[(2k + 1) * n + i] (the layout of trc_rays.mat)
__global__ __launch_bounds__(256) void k_material_eval(const double *tab, int n_mat, const double *wl, long long n, double *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = wl[i];
    for (int k = 0; k < n_mat; ++k) {
        double re, im;
        trc_material_index(tab, k, x, &re, &im);
        out[(long long)(2 * k) * n + i] = re;
        out[(long long)(2 * k + 1) * n + i] = im;
    }
}

extern "C" int trc_scene_set_materials(trc_scene *sc, int32_t n_mat, const int32_t *n_points, const double *packed) {
    if (!sc) return trc_fail(TRC_ERR_INVALID, "scene is NULL");
    if (n_mat < 0 || n_mat > TRC_MATERIAL_MAX) return trc_fail(TRC_ERR_INVALID, "trc_scene_set_materials: between 0 and %d materials", TRC_MATERIAL_MAX);
    TRC_TRY(scene_quiet(sc));
    if (n_mat == 0) { sc->mat_tab_n = 0; sc->d_mat_tab.reset(); return TRC_OK; }
    if (!n_points || !packed) return trc_fail(TRC_ERR_INVALID, "trc_scene_set_materials: n_points and packed are required");
    // the caller's wl[n] | re[n] | im[n] per material, one after the other -> trc_material_index's table
    std::vector<double> tab((size_t)1 + 2 * n_mat);
    tab[0] = (double)n_mat;
    const double *p = packed;
    for (int k = 0; k < n_mat; ++k) {
        const int n = n_points[k];
        if (n < 2 || n > TRC_MATERIAL_MAX_POINTS) return trc_fail(TRC_ERR_INVALID, "material %d: a table has 2 to %d points (%d given)", k, TRC_MATERIAL_MAX_POINTS, n);
        for (int j = 0; j < 3 * n; ++j)
            if (!std::isfinite(p[j])) return trc_fail(TRC_ERR_INVALID, "material %d: the table holds a value that is not finite", k);
        for (int j = 1; j < n; ++j)
            if (!(p[j] > p[j - 1])) return trc_fail(TRC_ERR_INVALID, "material %d: wavelengths must increase strictly", k);
        tab[1 + 2 * k] = (double)tab.size();
        tab[2 + 2 * k] = (double)n;
        tab.push_back((double)n);
        tab.insert(tab.end(), p, p + 3 * n);
        p += 3 * n;
    }
    sc->mat_tab_n = 0;
    TRC_TRY(sc->d_mat_tab.alloc(tab.size()));
    HIP_TRY(hipMemcpy(sc->d_mat_tab.get(), tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    sc->mat_tab_n = n_mat;
    return TRC_OK;
}

extern "C" int trc_scene_eval_materials(trc_scene *sc, int64_t n, const double *wl, double *out) {
    if (!sc || n < 0 || (n > 0 && (!wl || !out))) return trc_fail(TRC_ERR_INVALID, "trc_scene_eval_materials: bad arguments");
    if (sc->mat_tab_n <= 0) return trc_fail(TRC_ERR_INVALID, "trc_scene_eval_materials: the scene has no material tables (trc_scene_set_materials)");
    if (n == 0) return TRC_OK;
    HIP_TRY(hipSetDevice(sc->ctx->device));
    DevBuf<double> d_wl, d_out;
    TRC_TRY(d_wl.alloc((size_t)n));
    TRC_TRY(d_out.alloc((size_t)n * 2 * (size_t)sc->mat_tab_n));
    HIP_TRY(hipMemcpy(d_wl.get(), wl, (size_t)n * 8, hipMemcpyHostToDevice));
    TRC_TRY(launch_wait(sc->ctx, "k_material_eval", k_material_eval, n, 0, sc->d_mat_tab.get(), sc->mat_tab_n, d_wl.get(), n, d_out.get()));
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)n * 2 * (size_t)sc->mat_tab_n * 8, hipMemcpyDeviceToHost));
    return TRC_OK;
}

#define BIN_TILE 256
__global__ __launch_bounds__(256) void k_bin_hits(long long n_hits, const int32_t *h_surf, const double *h_e, const double *hx,
                                                  const double *hy, const double *hz, int n_bins, const int32_t *surf_lo,
                                                  const int32_t *surf_hi, const double *ranges6, const int32_t *mode, double *out) {
    __shared__ double l_rng[BIN_TILE * 6];
    __shared__ double l_sum[BIN_TILE];
    __shared__ int32_t l_lo[BIN_TILE], l_hi[BIN_TILE], l_mode[BIN_TILE];
    for (int i = threadIdx.x; i < n_bins; i += blockDim.x) {
        l_lo[i] = surf_lo[i]; l_hi[i] = surf_hi[i]; l_mode[i] = mode[i]; l_sum[i] = 0.0;
        for (int k = 0; k < 6; ++k) l_rng[6 * i + k] = ranges6[6 * i + k];
    }
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_hits; i += (long long)gridDim.x * blockDim.x) {
        const int s = h_surf[i];
        if (s < 0) continue;                       // reserved but unwritten entry of an open chunk
        const double x = hx[i], y = hy[i], z = hz[i], e = h_e[i];
        double ang = atan2(y, x);
        if (ang < 0.0) ang += TRC_TWO_PI;
        const double rad = sqrt(x * x + y * y);
        const double rad9 = rint(rad * 1e9) / 1e9, z9 = rint(z * 1e9) / 1e9;
        for (int j = 0; j < n_bins; ++j) {
            if (s < l_lo[j] || s > l_hi[j]) continue;
            const int m = l_mode[j];
            const double *g = l_rng + 6 * j;
            const double hh = (m & TRC_BIN_ROUND9) ? z9 : z, rr = (m & TRC_BIN_ROUND9) ? rad9 : rad;
            bool in = true;
            if (m & TRC_BIN_ANGLE) in = in && ang >= g[0] && ang <= g[1];
            if (m & TRC_BIN_HEIGHT) in = in && hh >= g[2] && hh <= g[3];
            if (m & TRC_BIN_RADIUS) in = in && rr >= g[4] && ((m & TRC_BIN_RADIUS_HALF_OPEN) ? rr < g[5] : rr <= g[5]);
            if (in) atomicAdd(&l_sum[j], e);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_bins; i += blockDim.x)
        if (l_sum[i] != 0.0) atomicAdd(&out[i], l_sum[i]);
}

extern "C" int trc_scene_bin_hits(trc_scene *sc, int32_t n_bins, const int32_t *surf_lo, const int32_t *surf_hi,
                                  const double *ranges6, const int32_t *mode, double *out) {
    if (!sc || n_bins < 0 || (n_bins > 0 && (!surf_lo || !surf_hi || !ranges6 || !mode || !out))) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    if (n_bins == 0) return TRC_OK;
    trc_ctx *ctx = sc->ctx;
    unsigned long long cursor;
    TRC_TRY(scene_hit_cursor(sc, &cursor));
    const HitBuffer &hb = sc->hits;
    const long long reserved = hb.used(cursor);
    for (int i = 0; i < n_bins; ++i) out[i] = 0.0;
    if (reserved == 0) return TRC_OK;
    const size_t per_bin = 2 * sizeof(int32_t) + 6 * sizeof(double) + sizeof(int32_t) + sizeof(double);
    DevBuf<char> d_buf;
    TRC_TRY(d_buf.alloc((size_t)BIN_TILE * per_bin));
    double *d_rng = (double *)d_buf.get(), *d_out = d_rng + 6 * BIN_TILE;
    int32_t *d_lo = (int32_t *)(d_out + BIN_TILE), *d_hi = d_lo + BIN_TILE, *d_mode = d_hi + BIN_TILE;
    int st = TRC_OK;
    unsigned grid = (unsigned)((reserved + 255) / 256);
    if (grid > (unsigned)(ctx->n_cu * 8)) grid = (unsigned)(ctx->n_cu * 8);
    for (int b0 = 0; b0 < n_bins && st == TRC_OK; b0 += BIN_TILE) {
        const int nb = n_bins - b0 < BIN_TILE ? n_bins - b0 : BIN_TILE;
        hipError_t e = hipMemcpyAsync(d_rng, ranges6 + 6 * (size_t)b0, (size_t)nb * 48, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_lo, surf_lo + b0, (size_t)nb * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_hi, surf_hi + b0, (size_t)nb * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_mode, mode + b0, (size_t)nb * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, (size_t)nb * 8, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_bin_hits, dim3(grid), dim3(256), 0, ctx->stream, reserved, hb.surf.get(), hb.col[0].get(), hb.col[2].get(), hb.col[3].get(),
                               hb.col[4].get(), nb, d_lo, d_hi, d_rng, d_mode, d_out);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out + b0, d_out, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) st = trc_fail(TRC_ERR_DEVICE, "trc_scene_bin_hits: %s", hipGetErrorString(e));
    }
    return st;
}


#define TRC_TRANSFER_MAX_SURF 1024     /* (S+1) x S doubles, kept in every private copy of the tally buffer too */
extern "C" int trc_scene_enable_transfer(trc_scene *sc, int32_t on) {
    if (!sc) return trc_fail(TRC_ERR_INVALID, "scene is NULL");
    if (on && sc->n_surf > TRC_TRANSFER_MAX_SURF)
        return trc_fail(TRC_ERR_CAPACITY, "the transfer matrix is offered up to %d surfaces (scene has %d)", TRC_TRANSFER_MAX_SURF, sc->n_surf);
    TRC_TRY(scene_quiet(sc));
    return sc->tally.set_transfer(on != 0);       // (a change resets the tallies)
}

extern "C" int trc_scene_get_transfer(trc_scene *sc, double *out) {
    if (!sc || !out) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    if (sc->tally.transfer_offset() < 0) return trc_fail(TRC_ERR_INVALID, "the transfer matrix is not enabled (trc_scene_enable_transfer)");
    TRC_TRY(scene_quiet(sc));
    HIP_TRY(hipMemcpy(out, sc->tally.device() + sc->tally.transfer_offset(), (size_t)(sc->n_surf + 1) * sc->n_surf * sizeof(double), hipMemcpyDeviceToHost));
    return TRC_OK;
}

extern "C" int trc_scene_tally_size(trc_scene *sc, int64_t *n_doubles) {
    if (!sc || !n_doubles) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    *n_doubles = sc->tally.size();
    return TRC_OK;
}

extern "C" int trc_scene_export_tallies(trc_scene *sc, double *dst, int32_t on_device) {
    if (!sc || !dst) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    TRC_TRY(scene_quiet(sc));
    HIP_TRY(hipMemcpy(dst, sc->tally.device(), (size_t)sc->tally.size() * sizeof(double),
                      on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return TRC_OK;
}

extern "C" int trc_scene_import_tallies(trc_scene *sc, const double *src, int32_t on_device) {
    if (!sc || !src) return trc_fail(TRC_ERR_INVALID, "bad arguments");
    TRC_TRY(scene_quiet(sc));
    HIP_TRY(hipMemcpy(sc->tally.device(), src, (size_t)sc->tally.size() * sizeof(double),
                      on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return TRC_OK;
}

