// trc_kernels.hip -- CDNA4 (gfx950) kernels of the engines and the scene's part of the C-ABI of include/tracer_amd.h: the context,
// the scene and its owners (surfaces, search tables, Kd-tree, tallies, hit buffer, materials, histograms), the trace entry points
// and their results.  The entry points that take a context and no scene -- source tables, source generation, the per-object
// protocol -- are trc_protocol.hip; the host plumbing both units share is trc_host.h.
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
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>      // (wants <cstring> before it)

#include "trc_core.h"
#include "trc_bounds.h"
#include "trc_footprint.h"
#include "trc_device.h"
#include "trc_pool.h"
#include "trc_scene_host.h"
#include "trc_host.h"
#include "trc_hithist.h"

extern "C" const char *trc_last_error(void) { return g_last_error.c_str(); }
extern "C" int trc_abi_version(void) { return TRC_ABI_VERSION; }

// ================================================================================================
// host-side objects
// ================================================================================================
// The fast engine's hit buffer, where the hits on capturing surfaces wait until a script reads them: eight columns (absorbed and
// incident energy, hit point, direction) and the surface of every entry, -1 for an entry not written.  Hits of polychromatic rays
// bring 3 W spectral columns more: per hit the W sample wavelengths, the W samples of the spectrum that arrived and the W that left
// (k_s_shade_x).  All pending hits have the same spectral shape, and spectral columns, when there are any, have the `cap` rows of
// the others.  The cursor (entries reserved so far) and the count of dropped hits are words 0 and 1 of the scene's counter block:
// the methods that need the cursor are handed it.
struct HitBuffer {
    DevBuf<int32_t> surf;
    DevBuf<double> col[8];
    DevBuf<double> x;        // x_cols spectral columns, column k at x + k * cap
    int x_cols = 0;
    int64_t cap = 0;         // entries allocated: the capacity asked for + room for what the streaming engine's open chunks leave unused
    int64_t cap_user = 0;    // the capacity asked for
    uint32_t epoch = 0;      // bumped whenever the cursor is reset or wound back: chunks left open by earlier launches are stale
    uint32_t chunk = 0;      // entries a wave of the streaming engine's shading kernels reserves per atomic (set with the capacity)
    int64_t dirty_to = 0;    // entries [0, dirty_to) may have been written since the buffer was last emptied: emptying 2e8 entries
                             // for the 6e6 a trace used was 0.9 GB of memset, twice per call of the public entry point

    // surface -1 (not written) over n entries from s: the only writer of that mark on the host
    static hipError_t unwrite(int32_t *s, int64_t n) { return n > 0 ? hipMemset(s, 0xFF, (size_t)n * sizeof(int32_t)) : hipSuccess; }
    int64_t used(unsigned long long cursor) const { return cursor < (unsigned long long)cap ? (int64_t)cursor : cap; }
    unsigned chunk_size() const { return chunk ? chunk : SQ_HIT_CHUNK; }
    int set_capacity(int64_t capacity);
    int allocate(int64_t capacity, int64_t slack, int64_t keep);
    // room for at least `capacity` hits, half as much again at least, keeping entries [0, cursor); the chunk size stays (chunks
    // left open by earlier launches go on being filled)
    int grow(int64_t capacity, unsigned long long cursor) {
        return allocate(capacity > cap_user + cap_user / 2 ? capacity : cap_user + cap_user / 2, cap - cap_user, used(cursor));
    }
    // forget the captured hits (the caller zeroes the cursor): every entry unwritten, open chunks stale
    int reset() {
        epoch += 1;
        HIP_TRY(unwrite(surf.get(), dirty_to < cap ? dirty_to : cap));
        dirty_to = 0;
        return TRC_OK;
    }
    // a fast call may write any entry until it says how far it got: what begin_call returns goes to end_call with the cursor then
    int64_t begin_call() { const int64_t before = dirty_to; dirty_to = cap; return before; }
    void end_call(int64_t before, unsigned long long cursor) {      // (every entry written lies below the cursor: chunks are reserved by advancing it)
        const int64_t cur = used(cursor);
        dirty_to = cur > before ? cur : before;
    }
    // the call that found the cursor at `cursor` failed part way: the hits its completed bounces captured are unwritten again, the
    // cursor (d_cursor) goes back and the chunks they left open are stale
    void rollback(unsigned long long *d_cursor, unsigned long long cursor) {
        unsigned long long now = 0;
        (void)hipDeviceSynchronize();
        if (cap > 0 && hipMemcpy(&now, d_cursor, sizeof(now), hipMemcpyDeviceToHost) == hipSuccess && now > cursor) {
            const int64_t end = used(now);
            if (end > (int64_t)cursor) (void)unwrite(surf.get() + cursor, end - (int64_t)cursor);
            (void)hipMemcpy(d_cursor, &cursor, sizeof(cursor), hipMemcpyHostToDevice);
        }
        epoch += 1;
    }
    // the spectral columns for a call whose hits carry `cols` of them (0: none), made or dropped as the call needs: a call whose
    // hits would differ in shape from those the buffer holds (cursor > 0) is refused
    int spectra_for(int cols, unsigned long long cursor, double **out) {
        *out = nullptr;
        if (cols != x_cols) {
            if (cursor != 0)
                return trc_fail(TRC_ERR_INVALID, "the hit buffer holds hits with %d spectral columns, this call's would have %d: read or clear them first", x_cols, cols);
            x.reset(); x_cols = 0;
            if (cols > 0) { TRC_TRY(x.alloc((size_t)cols * (size_t)cap)); x_cols = cols; }
        }
        *out = x.get();
        return TRC_OK;
    }
    void fill(DScene &d) const {
        d.hit_cap = cap; d.h_surf = surf.get();
        d.h_eabs = col[0].get(); d.h_ein = col[1].get(); d.h_px = col[2].get(); d.h_py = col[3].get(); d.h_pz = col[4].get();
        d.h_dx = col[5].get(); d.h_dy = col[6].get(); d.h_dz = col[7].get();
    }
    int read(hipStream_t stream, const std::vector<trc_surface_desc> &surfs, const int32_t *d_sflags, unsigned long long cursor,
             int64_t *n, int32_t *surf_out, double *const dst[8], int32_t n_x, double *x_out) const;
};

// The scene's counter block: eight 64-bit words the fast engine's kernels count into (DScene.counters, DScene.energy_left),
// CNT_ENERGY_LEFT holding the bits of a double.  A call reads all 64 bytes back once, when it ends, and the host keeps that copy
// (the mirror): the next call knows where its counts start without a read before it runs.  Every write to the block from the host
// is a method here and leaves the mirror in step; only HitBuffer::rollback winds the hit cursor back through device(), after a
// failed call, when the mirror is stale anyway.
enum CounterWord { CNT_HIT_CURSOR = 0, CNT_DROPPED = 1, CNT_LAST_CURSOR = 2, CNT_RAYS_LEFT = 3, CNT_ENERGY_LEFT = 5, CNT_WORDS = 8 };

struct CounterValues { unsigned long long hit_cursor, dropped, last_cursor, rays_left; double energy_left; };

class CounterBlock {
    DevBuf<unsigned long long> d_;
    unsigned long long mirror_[CNT_WORDS] = {};
    bool mirror_ok_ = false;      // false from a call's snapshot() until its read_back(): the kernels are counting

    CounterValues values() const {
        CounterValues v = {mirror_[CNT_HIT_CURSOR], mirror_[CNT_DROPPED], mirror_[CNT_LAST_CURSOR], mirror_[CNT_RAYS_LEFT], 0.0};
        memcpy(&v.energy_left, &mirror_[CNT_ENERGY_LEFT], sizeof(double));
        return v;
    }
    int fetch() {
        if (hipMemcpy(mirror_, d_.get(), sizeof(mirror_), hipMemcpyDeviceToHost) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "counter readback failed");
        return TRC_OK;
    }
    // words [first, first + n) to zero, here and on the device (the context's stream is idle)
    int clear(int first, int n) {
        HIP_TRY(hipMemset(d_.get() + first, 0, (size_t)n * sizeof(unsigned long long)));
        memset(mirror_ + first, 0, (size_t)n * sizeof(unsigned long long));
        return TRC_OK;
    }
public:
    int alloc() { TRC_TRY(d_.alloc(CNT_WORDS)); return zero(); }
    unsigned long long *device() const { return d_.get(); }
    void fill(DScene &d) const { d.counters = d_.get(); d.energy_left = (double *)(d.counters + CNT_ENERGY_LEFT); }     // one 64-byte block: one read-back gets both
    // the block as a call finds it (read from the device only when the mirror is stale); the mirror is stale from here on
    int snapshot(CounterValues *v) {
        if (!mirror_ok_) TRC_TRY(fetch());
        mirror_ok_ = false;
        *v = values();
        return TRC_OK;
    }
    // ... and as the call left it: the one read-back of a call
    int read_back(CounterValues *v) {
        TRC_TRY(fetch());
        mirror_ok_ = true;
        *v = values();
        return TRC_OK;
    }
    int zero() { return clear(0, CNT_WORDS); }
    int restart_hits() { return clear(CNT_HIT_CURSOR, 2); }     // cursor and dropped count start over
    // the `last` cursor restarts for every call: written only where the snapshot found it moved
    int restart_last(const CounterValues &before) {
        const unsigned long long zero = 0;
        if (before.last_cursor == 0ull) return TRC_OK;
        if (hipMemcpy(d_.get() + CNT_LAST_CURSOR, &zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "memcpy failed");
        mirror_[CNT_LAST_CURSOR] = 0ull;
        return TRC_OK;
    }
    bool stale() const { return !mirror_ok_; }
    // entries of the hit buffer reserved so far: the mirror's when it is valid; when it is stale() the caller has waited for the
    // context's stream and word 0 is read from the device
    int hit_cursor(unsigned long long *cursor) const {
        if (mirror_ok_) { *cursor = mirror_[CNT_HIT_CURSOR]; return TRC_OK; }
        HIP_TRY(hipMemcpy(cursor, d_.get() + CNT_HIT_CURSOR, sizeof(*cursor), hipMemcpyDeviceToHost));
        return TRC_OK;
    }
};

// The parts of a scene, one owner each.  A part keeps its device buffers to itself and is present whole or absent whole: a method
// that changes one builds the new state beside the old -- host tables in copies, device buffers in locals -- and moves it in when
// all of it is there, so a call that fails half way (out of memory) leaves the part as it was or empty, never new counts beside old
// pointers.  fill() writes the part's slice of DScene and nothing else, facts() its slice of the facts trc_forms.h decides on; the
// arithmetic they share with the host checks is trc_scene_host.h.

// The surfaces as the caller described them, and their records, optics and flags on the device.
class SceneSurfaces {
    std::vector<trc_surface_desc> surfs_;
    std::vector<double> extra_h_;
    int32_t stride_ = 0, n_extra_ = 0;
    bool splits_ = false;   // some optics can emit two rays per hit
    CarryNeeds needs_;      // needs.any(): some optics read what only rays of a given bundle carry (complex indices, spectra)
    DevBuf<double> d_recs_, d_opt_, d_extra_;
    DevBuf<int32_t> d_sflags_;
public:
    int create(const trc_surface_desc *surfs, int32_t n, int32_t n_extra, const double *extra);
    int upload();           // the records, optics and flags of the present poses
    void set_frames(const double *frames12) {
        for (size_t i = 0; i < surfs_.size(); ++i) memcpy(surfs_[i].frame, frames12 + 12 * i, 12 * sizeof(double));
    }
    const std::vector<trc_surface_desc> &all() const { return surfs_; }
    const trc_surface_desc *data() const { return surfs_.data(); }
    const trc_surface_desc &operator[](int i) const { return surfs_[i]; }
    bool splits() const { return splits_; }
    const CarryNeeds &needs() const { return needs_; }
    void fill(DScene &d) const {
        d.recs = d_recs_.get(); d.opt = d_opt_.get(); d.sflags = d_sflags_.get(); d.extra = d_extra_.get();
        d.stride = stride_; d.n_surf = (int32_t)surfs_.size(); d.n_extra = n_extra_;
    }
    void facts(trc_scene_facts &s) const { s.stride = stride_; s.n_extra = n_extra_; s.splits = splits_; }
};

// The single-precision search tables of the fast engine (trc_bounds.h) on the host and on the device, and the caller's Kd-tree packed
// beside them.  Absent (after a rebuild that failed): ok() false, every pointer null, and trc_forms.h decides for a scene without.
class SearchTables {
    trc_accel_host accel_{};
    bool ok_ = false, kd_ok_ = false;
    uint64_t geom_version_ = 0;     // bumped whenever the tables are rebuilt: what others derived from the old poses is stale
    DevBuf<float> d_sbox_, d_obb_, d_bg_ent_, d_clear_;
    DevBuf<uint32_t> d_nodes_, d_bg_off_, d_bg_occ_;
    DevBuf<uint16_t> d_leaf_, d_bleaf_, d_goff_, d_glist_;
    DevBuf<int32_t> d_unbounded_, d_gapart_, d_bg_apart_;
    int build(const trc_surface_desc *surfs, int n);
public:
    // the tables of the surfaces' present poses; the packed Kd-tree described the old ones and goes
    int rebuild(const trc_surface_desc *surfs, int n) {
        const uint64_t version = geom_version_ + 1;
        SearchTables t;
        const int st = t.build(surfs, n);
        *this = st == TRC_OK ? std::move(t) : SearchTables();
        geom_version_ = version;
        return st;
    }
    // the packed form of a tree trc_kd_check accepted, where it has one (else the float64 tree alone serves)
    int pack_kd(const trc_kdtree_desc *kd) {
        drop_kd();
        if (!ok_ || !trc_accel_build_kd(kd, accel_)) return TRC_OK;
        DevBuf<uint32_t> nodes;
        DevBuf<uint16_t> leaf;
        TRC_TRY(dev_upload(nodes, accel_.nodes.data(), accel_.nodes.size()));
        TRC_TRY(dev_upload(leaf, accel_.leaf_surfs.data(), accel_.leaf_surfs.size()));
        d_nodes_ = std::move(nodes); d_leaf_ = std::move(leaf);
        kd_ok_ = true;
        return TRC_OK;
    }
    void drop_kd() { d_nodes_.reset(); d_leaf_.reset(); kd_ok_ = false; }
    const trc_accel_host &host() const { return accel_; }
    uint64_t geom_version() const { return geom_version_; }
    // the clear cones of the present poses (trc_clear_build), TRC_CLEAR_T x TRC_CLEAR_T tiles per surface; null: no surface has one
    const float *clear_cones() const { return ok_ && accel_.clear_cones > 0 ? d_clear_.get() : nullptr; }
    void fill(DScene &d) const;
    void facts(trc_scene_facts &s) const { s.accel_ok = ok_; s.accel_kd_ok = kd_ok_; }
};

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

// The caller's Kd-tree as the float64 walks read it (k_trace_fast, k_ord_bounce): set() takes a tree trc_kd_check accepted.
class KdTables {
    DevBuf<int32_t> d_a_, d_b_, d_leaf_, d_always_;
    DevBuf<double> d_split_;
    int32_t nodes_ = 0, nleaf_ = 0, nalways_ = 0;
    double bounds_[6] = {};
    bool has_ = false;
public:
    int set(const trc_kdtree_desc *kd) {
        std::vector<int32_t> a, b;
        trc_kd_pack(kd, a, b);
        KdTables t;
        TRC_TRY(dev_upload(t.d_a_, a.data(), a.size()));
        TRC_TRY(dev_upload(t.d_b_, b.data(), b.size()));
        TRC_TRY(dev_upload(t.d_split_, kd->split, (size_t)kd->n_nodes));
        TRC_TRY(dev_upload(t.d_leaf_, kd->leaf_surfs, (size_t)kd->n_leaf_surfs));
        TRC_TRY(dev_upload(t.d_always_, kd->always_relevant, (size_t)kd->n_always));
        t.nodes_ = kd->n_nodes; t.nleaf_ = kd->n_leaf_surfs; t.nalways_ = kd->n_always;
        memcpy(t.bounds_, kd->bounds, sizeof(t.bounds_));
        t.has_ = true;
        *this = std::move(t);
        return TRC_OK;
    }
    void clear() { *this = KdTables(); }
    bool has() const { return has_; }
    void fill(DScene &d) const {
        d.has_kd = has_ ? 1 : 0;
        d.kd_a = d_a_.get(); d.kd_b = d_b_.get(); d.kd_leaf = d_leaf_.get(); d.kd_always = d_always_.get();
        d.kd_split = d_split_.get();
        d.kd_nodes = nodes_; d.kd_nleaf = nleaf_; d.kd_nalways = nalways_;
        for (int i = 0; i < 3; ++i) { d.kd_bmin[i] = bounds_[i]; d.kd_bmax[i] = bounds_[3 + i]; }
    }
    void facts(trc_scene_facts &s) const { s.has_kd = has_; s.kd_nodes = nodes_; s.kd_nleaf = nleaf_; s.kd_nalways = nalways_; }
};

// The tallies and the flux maps binned into them: the buffer (trc_tally_layout), the maps' descriptors, edges and surfaces on the
// host and on the device.  add_map and set_transfer give a new buffer, zeroed; when they fail everything is as it was.
class TallyBuffer {
    DevBuf<double> d_tally_, d_fm_edges_;
    int64_t n_ = 0, tr_off_ = -1;
    std::vector<FluxMapDev> fms_h_;
    std::vector<double> fm_edges_h_;
    std::vector<int32_t> fm_of_surf_h_;
    DevBuf<int32_t> d_fm_of_surf_;
    DevBuf<FluxMapDev> d_fms_;
    // these maps and this choice for the matrix: laid out, brought to the device, then taken
    int commit(std::vector<FluxMapDev> fms, std::vector<double> edges, std::vector<int32_t> of_surf, bool transfer) {
        const trc_tally_plan L = trc_tally_layout((int)of_surf.size(), fms.data(), fms.size(), transfer);
        for (size_t k = 0; k < fms.size(); ++k) fms[k].bins = L.bins[k];
        DevBuf<double> tally, d_edges;
        DevBuf<int32_t> d_of;
        DevBuf<FluxMapDev> d_fms;
        TRC_TRY(tally.alloc((size_t)L.total));
        HIP_TRY(hipMemset(tally.get(), 0, (size_t)L.total * sizeof(double)));
        if (!fms.empty()) {
            TRC_TRY(dev_upload(d_fms, fms.data(), fms.size()));
            TRC_TRY(dev_upload(d_edges, edges.data(), edges.size()));
        }
        TRC_TRY(dev_upload(d_of, of_surf.data(), of_surf.size(), "upload failed"));
        d_tally_ = std::move(tally); d_fm_edges_ = std::move(d_edges); d_fm_of_surf_ = std::move(d_of); d_fms_ = std::move(d_fms);
        fms_h_.swap(fms); fm_edges_h_.swap(edges); fm_of_surf_h_.swap(of_surf);
        n_ = L.total; tr_off_ = L.tr_off;
        return TRC_OK;
    }
public:
    int create(int32_t n_surf) { return commit({}, {}, std::vector<int32_t>((size_t)n_surf, -1), false); }
    int add_map(int32_t surf, int32_t chart, int32_t nu, int32_t nv, const double *u_edges, const double *v_edges, const double *proj12) {
        if (fm_of_surf_h_[surf] >= 0) return trc_fail(TRC_ERR_INVALID, "surface %d already has a flux map", surf);
        std::vector<FluxMapDev> fms = fms_h_;
        std::vector<double> edges = fm_edges_h_;
        std::vector<int32_t> of_surf = fm_of_surf_h_;
        FluxMapDev m;
        m.surf = surf; m.nu = nu; m.nv = nv; m.chart = chart;
        m.edges_u = (int64_t)edges.size();
        edges.insert(edges.end(), u_edges, u_edges + nu + 1);
        m.edges_v = (int64_t)edges.size();
        edges.insert(edges.end(), v_edges, v_edges + nv + 1);
        memcpy(m.proj, proj12, sizeof(m.proj));
        m.bins = 0;
        of_surf[surf] = (int32_t)fms.size();
        fms.push_back(m);
        return commit(std::move(fms), std::move(edges), std::move(of_surf), tr_off_ >= 0);
    }
    // flux-map bins keep their offsets (the matrix comes last)
    int set_transfer(bool on) { return on == (tr_off_ >= 0) ? TRC_OK : commit(fms_h_, fm_edges_h_, fm_of_surf_h_, on); }
    int zero() { HIP_TRY(hipMemset(d_tally_.get(), 0, (size_t)n_ * sizeof(double))); return TRC_OK; }
    double *device() const { return d_tally_.get(); }
    int64_t size() const { return n_; }
    int64_t transfer_offset() const { return tr_off_; }     // -1: the matrix is not kept
    const FluxMapDev *map_of(int32_t surf) const { return fm_of_surf_h_[surf] >= 0 ? &fms_h_[fm_of_surf_h_[surf]] : nullptr; }
    // some flux map bins in another chart than XY: the call runs the CHART instances of the kernels that finish hits
    bool has_chart() const { return std::any_of(fms_h_.begin(), fms_h_.end(), [](const FluxMapDev &m) { return m.chart != TRC_FM_XY; }); }
    void fill(DScene &d) const {
        d.tally = d_tally_.get();
        d.fm_of_surf = d_fm_of_surf_.get(); d.fms = d_fms_.get(); d.fm_edges = d_fm_edges_.get();
        d.tr_off = tr_off_;
        d.n_fm = (int32_t)fms_h_.size(); d.n_fm_edges = (int32_t)fm_edges_h_.size();
    }
    void facts(trc_scene_facts &s) const {
        s.n_fm_edges = (int)fm_edges_h_.size(); s.fms_bytes = (int)(fms_h_.size() * sizeof(FluxMapDev));
        for (auto &m : fms_h_) s.fm_bins += (long long)m.nu * m.nv;
        s.chart = has_chart();
        s.transfer = tr_off_ >= 0;
    }
};

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

struct trc_scene {
    trc_ctx *ctx;
    int32_t n_surf;
    SceneSurfaces surfaces;
    SearchTables search;
    KdTables kd;
    TallyBuffer tally;
    StagedSource staged;
    // the tabulated materials of the scene's optics on the device (trc_scene_set_materials; trc_material_index's packed table, in
    // global memory: part of no LDS image), mat_tab_n of them (0: none).  A call that brings no trc_rays.mat reads them.
    DevBuf<double> d_mat_tab;
    int32_t mat_tab_n = 0;
    bool mat_tab_serves() const { return surfaces.needs().max_mat >= 0 && mat_tab_n > surfaces.needs().max_mat; }
    std::unique_ptr<struct StreamEngine> stream_eng;   // slots of the streaming fast engine (trc_stream.inc), allocated on first use
    std::unique_ptr<struct OrdScratch> ord_scratch;    // scratch of the ordered engine's bounce loop, kept between calls
    CounterBlock counters;
    GrowBuf<double> d_last[7];        // device side of trc_trace_fast's `last` bundle, kept between calls (seven hipMalloc / hipFree per
                                      // call were a millisecond of a Monte-Carlo loop's 1e6-ray calls)
    GrowBuf<double> d_last_x;         // ... and the spectra of the rays a source that carries its spectrum leaves (W rows)
    HitBuffer hits;
    double hist_ms = 0.0;             // device time of the last k_hist_hits (trc_scene_histogram_hits_ms)
};

// the device of the scene's context current and its stream idle: what every entry point that touches the scene's buffers from the
// host begins with
static int scene_quiet(const trc_scene *sc) {
    HIP_TRY(hipSetDevice(sc->ctx->device));
    HIP_TRY(hipStreamSynchronize(sc->ctx->stream));
    return TRC_OK;
}

// the device view of the scene: every part writes its own slice
static DScene make_dscene(const trc_scene *sc) {
    DScene d;
    memset(&d, 0, sizeof(d));
    sc->surfaces.fill(d); sc->kd.fill(d); sc->search.fill(d); sc->tally.fill(d); sc->counters.fill(d); sc->hits.fill(d);
    return d;
}

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

// the cursor of the hit buffer once the context's stream has finished, for what goes on to work on the buffer
static int scene_hit_cursor(trc_scene *sc, unsigned long long *cursor) {
    TRC_TRY(scene_quiet(sc));
    return sc->counters.hit_cursor(cursor);
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
__global__ __launch_bounds__(256) void k_hits_pack(HitPack H, const uint32_t *offs, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s = H.surf[i];
    if (s < 0) return;
    const uint32_t o = offs[i];
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
    const int32_t s = H.surf[i];
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
    if (rocprim::exclusive_scan(nullptr, tmp_bytes, d_flag.get(), d_off.get(), 0u, (size_t)reserved, rocprim::plus<uint32_t>(), stream) != hipSuccess)
        return trc_fail(TRC_ERR_DEVICE, "exclusive_scan (size query) failed");
    TRC_TRY(d_tmp.alloc(tmp_bytes ? tmp_bytes : 1));
    if (rocprim::exclusive_scan(d_tmp.get(), tmp_bytes, d_flag.get(), d_off.get(), 0u, (size_t)reserved, rocprim::plus<uint32_t>(), stream) != hipSuccess)
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
        if (rocprim::radix_sort_pairs(nullptr, sort_bytes, key0, key1, ent0, ent1, (size_t)reserved, 0, bits, stream) != hipSuccess)
            return trc_fail(TRC_ERR_DEVICE, "radix_sort_pairs (size query) failed");
        TRC_TRY(d_tmp.alloc(sort_bytes ? sort_bytes : 1));
        if (rocprim::radix_sort_pairs(d_tmp.get(), sort_bytes, key0, key1, ent0, ent1, (size_t)reserved, 0, bits, stream) != hipSuccess)
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

// The captured hits binned where they lie (k_hist_hits, trc_hithist.hip): edges up, one pass over the reserved entries, planes down.
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

extern "C" int trc_scene_histogram_hits(trc_scene *sc, const trc_hit_hist_desc *d, double *sum, double *sum_sq, int64_t *count, double *outside) {
    if (!sc || !d || !sum) return trc_fail(TRC_ERR_INVALID, "trc_scene_histogram_hits: bad arguments");
    TRC_TRY(hit_hist_check("trc_scene_histogram_hits", sc, d, true));

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
    if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
    if (e == hipSuccess) e = trc_hit_hist_launch(ctx->stream, ctx->n_cu, A);
    if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back.data(), A.sum, back.size() * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);      // (always: nothing queued may outlive the buffers it uses)
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "trc_scene_histogram_hits: %s", hipGetErrorString(e));
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) sc->hist_ms = ms;
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
    if (e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
    if (e == hipSuccess) e = trc_hit_hist_x_launch(ctx->stream, ctx->n_cu, X);
    if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back.data(), A.sum, tail * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);      // (always: nothing queued may outlive the buffers it uses)
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) sc->hist_ms = ms;
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

// ================================================================================================
// what a call brings: the source's spectrum, the columns rays carry beyond the nine (both engines)
// ================================================================================================
// The spectrum travels to the fast engine as FastParams.spec (trc_spectrum_of layout: n, constant wavelength, index, then the
// table), in a buffer kept on the scene between calls.  The SPEC instances of the kernels draw the wavelength where a source ray
// first needs one.
static int scene_stage_spectrum(trc_scene *sc, const SourceSpectrum &sp, const double **d_spec) {
    const int n_tab = sp.desc->kind != TRC_SPECTRUM_CONSTANT ? sp.desc->n : 0;
    std::vector<double> packed((size_t)3 + sp.tab.size());
    packed[0] = (double)n_tab; packed[1] = sp.desc->wavelength; packed[2] = sp.desc->ref_index;
    std::copy(sp.tab.begin(), sp.tab.end(), packed.begin() + 3);
    return sc->staged.spectrum(packed, d_spec);
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
        if (C.spec->desc) TRC_TRY(scene_stage_spectrum(C.sc, *C.spec, &C.d_spec));
        TRC_TRY(source_kind_check(C.src));
        return C.sc->staged.source(C.src, &C.d_src);
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
    trc_scene *sc = C.sc;
    const trc_rays *last = C.last;
    if (!(C.flags & TRC_TRACE_KEEP_LAST)) return TRC_OK;
    if (!last || !last->x || !last->y || !last->z || !last->dx || !last->dy || !last->dz || !last->e || last->on_device)
        return trc_fail(TRC_ERR_INVALID, "TRC_TRACE_KEEP_LAST needs a host `last` bundle with x..e");
    C.last_cap = last->n;
    for (int i = 0; i < 7; ++i) {
        if (C.last_cap > 0) TRC_TRY(sc->d_last[i].reserve((size_t)C.last_cap));
        C.d_last[i] = sc->d_last[i].get();
    }
    // the rays left by a source that carries its spectrum bring their spectra back, when the caller made room for them
    const int W = C.spec->carried();
    if (W > 0 && last->spectra && last->n_spec == W && C.last_cap > 0) {
        const size_t need = (size_t)W * (size_t)C.last_cap;
        TRC_TRY(sc->d_last_x.reserve(need));
        C.d_last_x = sc->d_last_x.get();
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
        if (!sc->stream_eng) {
            sc->stream_eng.reset(new (std::nothrow) StreamEngine());
            if (!sc->stream_eng) return trc_fail(TRC_ERR_NOMEM, "out of host memory");
        }
        if (int e = stream_trace(sc, P, carry_in, engine.plan, C.facts, C.src, *sc->stream_eng, &C.s, &C.stream_seg, &C.stream_hits)) {
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
    trc_scene *sc; trc_result *res; PayLayout lay; int32_t flags; double min_energy; uint64_t seed;
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
    OrdScratch &sx = *sc->ord_scratch;
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
    OrdScratch &sx = *sc->ord_scratch;
    const int64_t slots = 2 * n_cur;
    hipLaunchKernelGGL(k_compact_scatter, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, ctx->stream, sx.key.get(), (long long)slots,
                       sx.blk_off.get(), sx.ckey.get(), sx.cslot.get());
    // stable sort by (culled, surface, block); slot order (= parent order) is kept inside a key
    size_t tmp_bytes = 0;
    hipError_t re = rocprim::radix_sort_pairs(nullptr, tmp_bytes, sx.ckey.get(), sx.skey.get(), sx.cslot.get(), sx.sslot.get(), (size_t)m, 0, 31, ctx->stream);
    if (re != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "radix_sort_pairs(size query) failed: %s", hipGetErrorString(re));
    TRC_TRY(sx.sort_tmp.reserve(std::max(tmp_bytes, (size_t)1)));
    re = rocprim::radix_sort_pairs(sx.sort_tmp.get(), tmp_bytes, sx.ckey.get(), sx.skey.get(), sx.cslot.get(), sx.sslot.get(), (size_t)m, 0, 31, ctx->stream);
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
    if (!sc->ord_scratch) { sc->ord_scratch.reset(new (std::nothrow) OrdScratch()); if (!sc->ord_scratch) return trc_fail(TRC_ERR_NOMEM, "out of host memory"); }
    OrdCall C = {sc, res.get(), lay, flags, min_energy, seed};      // (stats and time: zero)
    C.mat_tab = mat_dev ? sc->d_mat_tab.get() : nullptr;
    const int st = ordered_steps(C, in, src, spec, n, reps, ray_offset);
    if (sc->ord_scratch->cap_slots > ORD_SCRATCH_KEEP) *sc->ord_scratch = OrdScratch();      // (beyond 2^26 slots -- 10 GB -- the scratch goes back after the call)
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
