// trc_scene.h -- the scene as the library's units see it: its parts, one owner each (hit buffer, counter block, surfaces, search
// tables, Kd-tree, tallies), struct trc_scene, and the three functions every unit that is handed a scene begins with.  A host header
// that needs HIP, as trc_host.h does: the parts own device memory (DevBuf) and write their slice of DScene (trc_device.h).  What of a
// scene is plain host arithmetic is trc_scene_host.h, which g++ compiles for the host checks.  The member functions declared here
// and not defined are trc_scene.hip's; the engines' own per-scene state (EngineState) is trc_kernels.hip's, and a scene only holds it.
#ifndef TRC_SCENE_H
#define TRC_SCENE_H

#include <algorithm>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "trc_core.h"
#include "trc_bounds.h"
#include "trc_device.h"
#include "trc_scene_host.h"
#include "trc_host.h"

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
// What the engines keep on a scene between calls (trc_kernels.hip: the streaming engine's slots, the ordered engine's scratch, the
// staged source, the device side of the `last` bundle).  The scene holds it and names nothing in it: made by the first trace, it
// goes with the scene through a deleter the engines' unit defines.
struct EngineState;
struct EngineStateDelete { void operator()(EngineState *e) const; };

struct trc_scene {
    trc_ctx *ctx;
    int32_t n_surf;
    SceneSurfaces surfaces;
    SearchTables search;
    KdTables kd;
    TallyBuffer tally;
    // the tabulated materials of the scene's optics on the device (trc_scene_set_materials; trc_material_index's packed table, in
    // global memory: part of no LDS image), mat_tab_n of them (0: none).  A call that brings no trc_rays.mat reads them.
    DevBuf<double> d_mat_tab;
    int32_t mat_tab_n = 0;
    bool mat_tab_serves() const { return surfaces.needs().max_mat >= 0 && mat_tab_n > surfaces.needs().max_mat; }
    std::unique_ptr<EngineState, EngineStateDelete> engine;     // null until the first trace
    CounterBlock counters;
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

// the cursor of the hit buffer once the context's stream has finished, for what goes on to work on the buffer
static int scene_hit_cursor(trc_scene *sc, unsigned long long *cursor) {
    TRC_TRY(scene_quiet(sc));
    return sc->counters.hit_cursor(cursor);
}

#endif  // TRC_SCENE_H
