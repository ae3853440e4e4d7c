// trc_device.h -- device-side types and helpers shared by the translation units of the library (trc_kernels.hip, trc_shade.hip; trc_scene.h):
// the device view of a scene, the parameter blocks of the fast engine and of its streaming form, the chunked list appends and the
// per-hit bookkeeping.  Moved here unchanged from trc_kernels.hip / trc_stream.inc when the class-split shading kernels got a
// translation unit of their own (round 3).
#ifndef TRC_DEVICE_H
#define TRC_DEVICE_H

#include <hip/hip_runtime.h>
#include "trc_core.h"
#include "trc_bounds.h"
#include "trc_footprint.h"
#include "trc_forms.h"

struct FluxMapDev {
    int32_t surf, nu, nv, chart;   // chart: the coordinates the map bins in (TRC_FM_*, trc_core.h)
    int64_t edges_u, edges_v;  // offsets into fm_edges
    int64_t bins;              // offset into the tally buffer
    double proj[12];           // global -> local (rows 0..2 of round(inv(frame), 9), surface.py:125; row 2 is read by the charts other than XY)
};
static_assert(sizeof(FluxMapDev) == 136, "tests/shade_cases.py (SIZEOF_FLUXMAPDEV) restates this size in the sums of the LDS images");

// device view of a scene, passed by value to kernels
struct DScene {
    const double *recs;
    const double *opt;       // n_surf * 8
    const int32_t *sflags;   // n_surf
    const double *extra;
    int32_t stride, n_surf, n_extra, has_kd;
    // Kd-tree
    const int32_t *kd_a, *kd_b, *kd_leaf, *kd_always;
    const double *kd_split;
    int32_t kd_nodes, kd_nleaf, kd_nalways, kd_pad;
    double kd_bmin[3], kd_bmax[3];
    // single-precision acceleration data (trc_bounds.h)
    const float *a_sbox;
    const float *a_obb;        // TRC_OBB_STRIDE floats per surface: oriented boxes (trc_obb_hit32)
    const uint32_t *a_nodes;
    const uint16_t *a_leaf;
    const int32_t *a_unbounded;
    const uint16_t *a_bleaf;
    int32_t a_n_unbounded, a_kd_depth, a_ok, a_kd_ok;
    int32_t a_n_bleaf, a_pad2;
    uint32_t a_bnodes[2];
    float a_broot[6];
    float a_root[6];
    float a_delta, a_pad;
    double a_cen[3], a_slo[3], a_shi[3];
    // uniform grid (streaming engine)
    const uint16_t *a_goff, *a_glist;
    const int32_t *a_gapart;    // bounded surfaces kept out of the grid (box-tested for every ray)
    int32_t a_g_ok, a_g_ncell, a_g_nlist, a_g_napart, a_gdim[3];
    float a_glo[3], a_gcs[3], a_ginv[3], a_groot[6];
    // the grid of scenes too large for LDS (trc_accel_build_grid32): 32-bit offsets and lists in global memory
    const uint32_t *a_bg_off, *a_bg_occ;    // first entry of every cell; one bit per cell that lists anything
    const float *a_bg_ent;                  // TRC_BG_ENT floats per listed surface (trc_bounds.h)
    const int32_t *a_bg_apart;  // bounded surfaces kept out of that grid (box-tested for every ray)
    int32_t a_bg_napart, a_bg_pad;
    int32_t a_bg_ok, a_bg_dim[3];
    float a_bg_lo[3], a_bg_cs[3], a_bg_inv[3], a_bg_root[6];
    // tallies: [absorbed S | received S | count S | segments, hits | flux bins ... | transfer (S+1) x S]
    double *tally;
    long long tr_off;           // offset of the surface-to-surface transfer matrix in `tally`, -1 when it is not kept
    // flux maps
    int32_t n_fm, n_fm_edges;   // flux maps and the total length of their edge arrays
    const int32_t *fm_of_surf;  // n_surf, -1 = none
    const FluxMapDev *fms;
    const double *fm_edges;
    // hit capture
    unsigned long long *counters;  // [0] hit cursor, [1] hits dropped, [2] last cursor, [3] rays left
    double *energy_left;
    long long hit_cap;
    int32_t *h_surf;
    double *h_eabs, *h_ein, *h_px, *h_py, *h_pz, *h_dx, *h_dy, *h_dz;
};


// ================================================================================================
// device helpers
// ================================================================================================
struct LocalKdStack {
    int node[TRC_KD_STACK];
    float tmax[TRC_KD_STACK];
    __device__ __forceinline__ void push(int sp, int n, double t) {
        node[sp] = n;
        tmax[sp] = __double2float_ru(t);  // rounded up: the interval only ever grows (conservative)
    }
    __device__ __forceinline__ void pop(int sp, int *n, double *t) {
        *n = node[sp];
        *t = (double)tmax[sp];
    }
};

__device__ __forceinline__ trc_kd_view make_kd_view(const DScene &sc, const int32_t *a, const int32_t *b,
                                                    const double *split, const int32_t *leaf,
                                                    const int32_t *always) {
    trc_kd_view kd;
    kd.node_a = a; kd.node_b = b; kd.split = split; kd.leaf_surfs = leaf; kd.always = always;
    kd.n_always = sc.kd_nalways;
#pragma unroll
    for (int i = 0; i < 3; ++i) { kd.bmin[i] = sc.kd_bmin[i]; kd.bmax[i] = sc.kd_bmax[i]; }
    return kd;
}

__device__ __forceinline__ unsigned lane_id() { return __lane_id(); }

// wave-level sum of a double (64 lanes)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Queue append without a hot atomic: a wave reserves CHUNK entries at a time from the global counter (one atomic per
// chunk; a single word sustains only ~88 returning atomics per microsecond) and fills them; what is left of a chunk
// when the wave moves on is marked invalid and skipped by the consumers.  base/used are wave-uniform.
#ifndef SQ_CHUNK
#define SQ_CHUNK 256
#endif
#define SQ_INVALID 0xFFFFFFFFu

#define SQ_CHUNK_MAX 1024        /* large launches reserve more per atomic; queue slack is sized for this */

struct WaveChunk {
    unsigned long long base;
    unsigned used;
    unsigned open;
    unsigned size;      // entries reserved per atomic (SQ_CHUNK, or up to SQ_CHUNK_MAX in the largest launches)
};

__device__ __forceinline__ WaveChunk chunk_init(unsigned size = SQ_CHUNK) {
    WaveChunk c;
    c.base = 0; c.used = size; c.open = 0; c.size = size;
    return c;
}

// The first chunk of a wave can be handed out without an atomic: chunk number `wave` of a queue whose counter the host
// starts at (number of waves) * size.  Every wave of a launch reserving its first chunk at the same moment is otherwise
// thousands of atomics on one word before any work starts (~88 per microsecond).  A wave that never appends leaves the
// whole chunk marked invalid (chunk_close).
__device__ __forceinline__ WaveChunk chunk_init_static(unsigned size, unsigned long long wave) {
    WaveChunk c;
    c.base = wave * size; c.used = 0; c.open = 1; c.size = size;
    return c;
}

// the same with the chunk's first entry given (chunks of different sizes pre-assigned in one list)
__device__ __forceinline__ WaveChunk chunk_init_static_at(unsigned size, unsigned long long base) {
    WaveChunk c;
    c.base = base; c.used = 0; c.open = 1; c.size = size;
    return c;
}

// after a chunk_append made by a subset of the lanes: every lane takes the state of `lane` (one that took part)
__device__ __forceinline__ void chunk_rebroadcast(WaveChunk &c, int lane) {
    c.base = __shfl(c.base, lane, 64);
    c.used = (unsigned)__shfl((int)c.used, lane, 64);
    c.open = (unsigned)__shfl((int)c.open, lane, 64);
    c.size = (unsigned)__shfl((int)c.size, lane, 64);
}

// marks the unused tail of the current chunk invalid (wave-uniform call)
__device__ __forceinline__ void chunk_close(WaveChunk &c, uint32_t *tag, long long cap) {
    if (c.open) {
        for (unsigned k = c.used + lane_id(); k < c.size; k += 64)
            if ((long long)(c.base + k) < cap) tag[c.base + k] = SQ_INVALID;
    }
    c.open = 0;
    c.used = c.size;
}

// returns this lane's index in the queue (meaningful when `want`).  Call it with the whole wave, or -- inside a
// divergent region -- re-broadcast the chunk afterwards from a lane that took part (chunk_rebroadcast).  A request that does not fit the
// open chunk fills it up and continues in a new one, so entries are only wasted at the end of a kernel (< CHUNK per wave).
__device__ __forceinline__ unsigned long long chunk_append(unsigned long long *counter, WaveChunk &c, bool want, uint32_t *tag,
                                                           long long cap) {
    unsigned long long m = __ballot(want);
    if (!m) return 0;
    const unsigned need = (unsigned)__popcll(m);
    const unsigned rank = (unsigned)__popcll(m & ((1ull << lane_id()) - 1ull));
    unsigned long long idx;
    if (c.used + need > c.size) {
        const unsigned rem = c.open ? c.size - c.used : 0u;
        const unsigned long long old_pos = c.base + c.used;
        const int leader = __ffsll((long long)m) - 1;          // a lane that is certainly active here
        unsigned long long b = 0;
        if ((int)lane_id() == leader) b = atomicAdd(counter, (unsigned long long)c.size);
        c.base = __shfl(b, leader, 64);
        c.used = need - rem;
        c.open = 1;
        idx = rank < rem ? old_pos + rank : c.base + (rank - rem);
    } else {
        idx = c.base + c.used + rank;
        c.used += need;
    }
    (void)tag; (void)cap;
    return idx;
}

#define SHADE_MAX_WAVES 5120     /* waves of one launch of a shading kernel (at most n_cu * 2 workgroups of 10 waves, n_cu <= 256) */
#define SQ_HIT_CHUNK 1024        /* entries of the hit buffer a wave of k_s_shade reserves per atomic: the cursor is one word (~88 returning
                                    atomics per microsecond), and at 256 the 12 000 reservations of an NSTTF batch were half of the kernel */
#define TRC_HIT_HOLDERS (4ll * SHADE_MAX_WAVES)   /* waves that can hold an open chunk of the hit buffer: SHADE_MAX_WAVES per slot (the shading
                                                    kernels of a slot run one after another, wave w of each continues the chunk wave w of the
                                                    one before left open), four slots at most */
// The open chunk of the hit buffer a wave of a shading kernel carries to the next launch, in two words of its state `st`: the
// chunk's base, and epoch << 32 | used << 1 | open.  A chunk left open under another epoch (the buffer was emptied or wound back
// since) is stale.  Each kernel calls these under its own gate: capturing, and the wave is one that keeps its chunk.
__device__ __forceinline__ void hit_chunk_resume(WaveChunk &hc, const unsigned long long *st, unsigned epoch) {
    const unsigned long long w = st[1];
    if ((unsigned)(w >> 32) == epoch && (w & 1ull)) { hc.base = st[0]; hc.used = (unsigned)(w >> 1) & 0x7FFFFFFFu; hc.open = 1; }
}
__device__ __forceinline__ void hit_chunk_suspend(const WaveChunk &hc, unsigned long long *st, unsigned epoch) {
    st[0] = hc.base;
    st[1] = ((unsigned long long)epoch << 32) | ((unsigned long long)hc.used << 1) | (hc.open ? 1ull : 0ull);
}

#define TRC_SURF_TERMINAL 0x10000   /* device copy of the surface flags only: every ray that lands here ends here -- the optics absorb all of
                                       it whatever the angle (absorptivity 1, no incidence-angle factor): no direction needs to be drawn */

// a captured hit on surface s (flags fl) into entry `slot` of the hit buffer, or counted as dropped beyond its end.  A lean capture
// (TRC_SURF_CAPTURE_LEAN) writes neither the incident energy (column 1) nor the direction (columns 5-7).
__device__ __forceinline__ void hit_store(const DScene &sc, unsigned long long slot, int s, int fl, double e_in, double e_abs, double hx,
                                          double hy, double hz, double dx, double dy, double dz) {
    if ((long long)slot < sc.hit_cap) {
        sc.h_surf[slot] = s;
        sc.h_eabs[slot] = e_abs;
        sc.h_px[slot] = hx; sc.h_py[slot] = hy; sc.h_pz[slot] = hz;
        if (!(fl & TRC_SURF_CAPTURE_LEAN)) { sc.h_ein[slot] = e_in; sc.h_dx[slot] = dx; sc.h_dy[slot] = dy; sc.h_dz[slot] = dz; }
    } else {
        atomicAdd(&sc.counters[1], 1ull);
    }
}

// per-hit bookkeeping shared by both engines: tallies, flux map, hit capture
// CHART: the instance knows the flux-map charts other than XY (trc_fluxmap_uv: a float64 atan2, an acos and a square root).  Compiled
// apart, as SPEC and SUN are: the host picks the CHART instances of a kernel only for a scene that holds such a map, and the others
// are the code they were.
template <bool LDS_TALLY, bool CHART = false>
__device__ __forceinline__ void record_hit(const DScene &sc, double *lds_tally, int s, double e_in,
                                           double e_abs, double hx, double hy, double hz, double dx,
                                           double dy, double dz, bool capture_enabled, int prev, WaveChunk *hc = nullptr,
                                           double *lds_fm = nullptr, bool volume = false, bool tallied = false,
                                           unsigned long long *slot_out = nullptr) {
    // slot_out: where the hit went in the hit buffer (~0: not captured) -- chunked appends only
    // tallied: the caller has added the three per-surface sums itself (k_s_absorb: once per wave)
    // volume: the ray was scattered in the medium before it reached the surface -- nothing is recorded, but the lane takes part
    // in the appends of the wave below (their bookkeeping is per wave)
    const int S = sc.n_surf;
    // energy carried from the surface the ray left (S = the source) to the one it lands on
    if (sc.tr_off >= 0 && !volume) atomicAdd(&sc.tally[sc.tr_off + (long long)prev * S + s], e_in);
    if (volume || tallied) {
    } else if (LDS_TALLY) {
        atomicAdd(&lds_tally[s], e_abs);
        atomicAdd(&lds_tally[S + s], e_in);
        atomicAdd(&lds_tally[2 * S + s], 1.0);
    } else {
        atomicAdd(&sc.tally[s], e_abs);
        atomicAdd(&sc.tally[S + s], e_in);
        atomicAdd(&sc.tally[2 * S + s], 1.0);
    }
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
        if (iu >= 0 && iv >= 0) {
            // lds_fm: the workgroup's private copy of all flux-map bins (they follow the 3S+2 per-surface sums in the tally buffer);
            // scattered global float64 atomics run at ~1/17 of the rate of the contiguous ones the copy is flushed with
            if (lds_fm) atomicAdd(&lds_fm[m.bins - (3 * (int64_t)S + 2) + (int64_t)iu * m.nv + iv], e_abs);
            else atomicAdd(&sc.tally[m.bins + (int64_t)iu * m.nv + iv], e_abs);
        }
    }
    if (capture_enabled && hc) {
        // chunked append (streaming engine): one atomic per 256 captured hits instead of one per wave and iteration --
        // the cursor of the hit buffer is a single word, and a word sustains only ~88 returning atomics per microsecond
        const int fl = sc.sflags[s];
        bool want = !volume && (fl & TRC_SURF_CAPTURE_HITS) != 0;
        unsigned long long slot = chunk_append(&sc.counters[0], *hc, want, nullptr, 0);
        if (slot_out) *slot_out = (want && (long long)slot < sc.hit_cap) ? slot : ~0ull;
        if (want) {
            hit_store(sc, slot, s, fl, e_in, e_abs, hx, hy, hz, dx, dy, dz);
        }
    } else if (capture_enabled) {
        // wave-aggregated append: one atomic per wave per iteration
        const int fl = sc.sflags[s];
        bool want = !volume && (fl & TRC_SURF_CAPTURE_HITS) != 0;
        unsigned long long mask = __ballot(want);
        if (mask) {
            int leader = __ffsll((long long)mask) - 1;
            unsigned long long base = 0;
            if ((int)lane_id() == leader) base = atomicAdd(&sc.counters[0], (unsigned long long)__popcll(mask));
            base = __shfl(base, leader, 64);
            if (want) {
                unsigned long long slot = base + __popcll(mask & ((1ull << lane_id()) - 1ull));
                hit_store(sc, slot, s, fl, e_in, e_abs, hx, hy, hz, dx, dy, dz);
            }
        }
    }
}

// ================================================================================================
// fast engine
// ================================================================================================
// what the rays of a given bundle carry beyond the fast engine's record (streaming form only, k_s_shade_x): Im of the refractive
// index (n), the materials at each ray's wavelength (2 n_mat x n), sample wavelengths and spectra of polychromatic bundles
// (n_spec x n).  Kept out of FastParams and at the end of StreamParams: the kernels of the other scenes never read it, and six
// more words in the middle of their arguments cost the NSTTF bench 4 % (scalar loads regrouped).
struct CarryIn {
    const double *ref_im, *mat, *spec_wl, *spec;
    int n_mat, n_spec;
    double *slot_spec;      // the slot's table of spectra under way: sample w of the ray in slot s at slot_spec[w * room + s] (null: none)
    double *hit_x;          // 3 n_spec columns beside the hit buffer, hit_x_cap entries each (null: no spectra per captured hit):
    long long hit_x_cap;    // sample wavelengths, spectrum that arrived, spectrum that left
    // a scene whose optics split rays (k_s_shade_x<.., SPLIT>): the Philox stream of the ray in every slot of the ray table, which
    // is no function of SRayGeo.idx once a hit has sent two rays on (trc_child_rid); null for every other call.  Last, for the
    // reason given above.
    unsigned long long *slot_rid;
    // the scene's tabulated materials (trc_material_index's packed table, trc_scene_set_materials) for a call that brings no rows
    // of them: read by the MAT instances of k_s_shade_x alone, null for every other call.  The very last word, for the same reason.
    const double *mat_tab;
    // a source that carries its spectrum (TRC_SPECTRUM_CARRIED): read by k_s_shade_p alone, zero for every other call, and behind
    // everything else for the same reason.  spec_wl and spec above are null then (grid and values come from FastParams.spec) and
    // n_spec is the table's W.  last_spec / last_wl: spectra and sample wavelengths of the rays left, sample w of ray q at
    // [w * last_cap + q] (null: not asked for).  poly_cells: the polychromatic walls whose lambda cells the LDS instances stage (0: none)
    double *last_spec, *last_wl;
    int poly_cells;
};

struct FastParams {
    DScene sc;
    // given bundle (NULL when a source descriptor is used)
    const double *x, *y, *z, *dx, *dy, *dz, *e, *ref, *wl;
    const uint64_t *rid;
    const trc_source_desc *src;  // device copy
    long long n;
    int reps;
    int flags;
    double min_energy;
    unsigned long long seed, ray_offset;
    // rays left after `reps` bounces
    double *lx, *ly, *lz, *ldx, *ldy, *ldz, *le;
    long long last_cap;
    // LDS carve-up (in doubles / flags)
    int lds_scene;    // surfaces (+ Kd arrays) staged in LDS
    int lds_tally;    // tallies privatised in LDS
    int capture;      // some surface captures hits
    // source spectrum (trc_spectrum_of layout) when the rays of `src` draw wavelengths; read only by the SPEC instances
    const double *spec;
};


// shading + bookkeeping of one hit, shared by the two fast kernels.  Returns false when the ray stops here.
// SIMPLE promises a flat geometry kind and an optics kind of TRC_OPT_SIMPLE_MASK on every surface: the compiler drops the rest.
template <bool LDS_TALLY, bool SIMPLE = false, bool CHART = false>
__device__ __forceinline__ bool fast_shade(const FastParams &P, const double *recs, double *l_tally, double t, int s, double &px,
                                           double &py, double &pz, double &dx, double &dy, double &dz, double &e, double &ref,
                                           double wl, unsigned long long rid, int &bounce, int &prev, WaveChunk *hc = nullptr,
                                           double *lds_fm = nullptr, bool tallied = false, bool *was_volume = nullptr) {
    // tallied: the caller adds the three per-surface sums itself (k_s_shade: per wave), unless *was_volume comes back true
    const DScene &sc = P.sc;
    bounce += 1;
    const double *rec = recs + (size_t)s * sc.stride;
    double hx = px + t * dx, hy = py + t * dy, hz = pz + t * dz;
    double nx, ny, nz;
    if (SIMPLE && !trc_gm_is_flat(trc_rec_gm_kind(rec))) __builtin_unreachable();
    trc_normal(rec, hx, hy, hz, dx, dy, dz, &nx, &ny, &nz);
    trc_ray_out out[2];
    const double path = sqrt((hx - px) * (hx - px) + (hy - py) * (hy - py) + (hz - pz) * (hz - pz));
    if (SIMPLE && !((TRC_OPT_SIMPLE_MASK >> trc_rec_opt_kind(rec)) & 1u)) __builtin_unreachable();
    int n_out = trc_shade(trc_rec_opt_kind(rec), sc.opt + (size_t)s * 8, sc.extra, trc_rec_extra_off(rec), trc_rec_extra_len(rec),
                          rec[2], rec[5], rec[8], dx, dy, dz, e, ref, wl, path, nx, ny, nz, P.seed, rid, (uint32_t)bounce, out);
    (void)n_out;  // scenes whose optics split rays are routed to the ordered engine by the host
    // a volume event (scattering in the medium): the ray never reached the surface -- it goes on from a point before the hit,
    // the surface records nothing, the surface the ray left stays the one it left
    const bool volume = out[0].back > 0.0;
    if (was_volume) *was_volume = volume;
    if (volume) { hx -= out[0].back * dx; hy -= out[0].back * dy; hz -= out[0].back * dz; }
    double e_abs = e - out[0].e;
    record_hit<LDS_TALLY, CHART>(sc, l_tally, s, e, e_abs, hx, hy, hz, dx, dy, dz, P.capture != 0, prev, hc, lds_fm, volume, tallied);
    if (!volume) prev = s;
    px = hx + out[0].shift * nx; py = hy + out[0].shift * ny; pz = hz + out[0].shift * nz;      // (PeriodicBoundary: one period along the normal)
    dx = out[0].dx; dy = out[0].dy; dz = out[0].dz;
    e = out[0].e; ref = out[0].ref;
    if (e <= P.min_energy) return false;                      // tracer_engine.py:242
    if (bounce >= P.reps) {                                   // still alive after the last iteration
        atomicAdd(&sc.counters[3], 1ull);
        atomicAdd(sc.energy_left, e);
        if (P.flags & TRC_TRACE_KEEP_LAST) {
            unsigned long long slot = atomicAdd(&sc.counters[2], 1ull);
            if ((long long)slot < P.last_cap) {
                P.lx[slot] = px; P.ly[slot] = py; P.lz[slot] = pz;
                P.ldx[slot] = dx; P.ldy[slot] = dy; P.ldz[slot] = dz; P.le[slot] = e;
            }
        }
        return false;
    }
    return true;
}


// One ray of the table, split by use: what the search reads and updates is exactly one 64-byte sector, the rest
// (needed by shading only) another 32 bytes.  A structure-of-arrays table costs one sector per *field* on the gathers
// by slot of k_s_exact / k_s_shade (8x the useful bytes).
// Slots are handed out densely, in the order in which rays turn out to have a candidate (a chunked counter, CN(CW_SLOTS)): of the
// 1e8 source rays of an NSTTF step 6.5e6 ever need a record, and a table indexed by ray number spread those over 6.4 GB --
// every access of the later bounces a DRAM page of its own.  The ray's number in its batch travels in the record (idx).
#define SQ_SKIP_SELF 0x80000000u    /* tail, high word: the ray cannot meet the (flat) surface it left again -- its exact test would
                                       return t < 1e-7 (flat_surface.py:50): the searches leave that surface out */
struct __attribute__((aligned(64))) SRayGeo {
    double px, py, pz, dx, dy, dz;
    uint32_t head;                  // index in Q3 of the last finite candidate linked so far, SQ_INVALID = none (general path)
    uint32_t idx;                   // the ray's number in its batch: stream id = ray_offset + base + idx
    unsigned long long tail;        // bounce (low word) and the surface the ray left (high word, | SQ_SKIP_SELF)
};
__device__ __forceinline__ unsigned long long sray_tail(int bounce, uint32_t prev) { return (unsigned long long)(uint32_t)bounce | ((unsigned long long)prev << 32); }
// result of one exact test, linked per ray
struct __attribute__((aligned(16))) SCand {
    double t;
    uint32_t surf;
    uint32_t next;                  // the ray's previous finite candidate (index in Q3) or SQ_INVALID
};
struct __attribute__((aligned(32))) SRayAux {
    double e, ref, wl;
    double pad;
};

// Workgroups of k_s_shade add into one of TALLY_PARTS copies of the tally buffer (copy = workgroup number mod TALLY_PARTS):
// the end-of-workgroup flush of ~3S sums and the flux-map bins would otherwise be thousands of atomics per 128-byte line,
// which serialise at ~88 per microsecond.
#ifndef TALLY_PARTS
#define TALLY_PARTS 16          /* (the mesh of 1e5 faces, sums added per hit in global memory: 2 copies 12.6 ms per 1e7 rays, 4: 10.1, 16: 8.8, 32: 8.6, 64: 8.8) */
#endif

// counters live 128 bytes apart: atomics on words of one cache line serialise in the same L2 bank
#define CN(k) ((k) << 4)
#define CN_WORDS (32 << 4)
// the words of a slot's counter block (StreamWs::cnt[CN(word)]): lengths are entries reserved, unused tails of chunks included
enum StreamCounter {
    CW_Q1 = 0,            // walker queue
    CW_Q3 = 1,            // candidate queue
    CW_HIT_LIST = 2,      // hit list
    CW_ACT_OUT = 3,       // next active list
    CW_OVERFLOW = 4,      // overflow flag: 0 or a StreamOverflow
    CW_ACT_IN = 5,        // entries of the active list coming in
    CW_HITS = 6,          // hits (real count)
    CW_ALIVE = 7,         // rays going on (real count)
    CW_SLOTS = 8,         // slots of the ray table handed out
    CW_GEN_LIST = 9,      // general-path list of k_s_cull
    CW_FP_LIST = 10,      // footprint list of k_s_cull
    CW_TERM_LIST = 11,    // hits on terminal surfaces (k_s_bounce -> k_s_absorb)
    CW_TERM_HITS = 12,    // ... and their real count
    CW_CLS_HITS = 13,     // + class: hits shaded per class (TRC_CLS_COUNT words)
    CW_STATS = 16,        // first of the seven words of SW_STATS
    CW_AHEAD = 23,        // continued rays whose next segment k_s_shade_c finished itself (StreamParams::ahead): they are not in CW_ALIVE
    CW_CLS_LIST = 24,     // + class: entries of the class lists of k_s_partition (TRC_CLS_COUNT words)
    CW_AHEAD_HITS = 27    // ... and those of them that hit (the others left the scene): counted in CW_HITS and CW_TERM_HITS too
};
enum StreamOverflow : unsigned long long {
    CW_OVF_RETRY = 1,     // the candidate queue was too small: nothing of the bounce is committed, the host doubles it and runs the bounce again
    CW_OVF_FAIL = 2       // a list overflowed: the call fails
};

struct StreamWs {
    long long cap;      // rays per batch
    long long room;     // entries of the ray table and of every list of slots / ray numbers: cap + room for the unused tails of the
                        // chunks (SQ_CHUNK_MAX * 16384 entries; TRC_STREAM_ROOM sets the whole: tests make the lists overflow with it)
    long long q3_cap;   // candidate pairs per bounce
    long long act_room; // entries of the two active lists: several shading kernels append to one list, each behind chunks sized for what
                        // it is expected to keep alive -- room for every ray of the batch behind pre-assigned chunks for every ray
    SRayGeo *geo;
    SRayAux *aux;
    uint32_t *q1_slot;
    float4 *q1_a, *q1_b;   // (ox, oy, oz, ix), (iy, iz, tmin, tmax)
    uint32_t *q3_slot, *q3_surf;
    SCand *q3n;
    uint32_t *hit_slot;        // the hit list: slot of every ray that hit something, with -- when the kernel that found the hit
    uint32_t *hit_surf;        // resolved it itself (k_s_fresh, k_s_bounce) -- the surface and the distance; SQ_INVALID in hit_surf:
    double *hit_t;             // k_s_shade picks the nearest of the ray's linked candidates (general path, k_s_exact)
    uint32_t *gen_list;        // fresh rays that k_s_cull leaves to the general path (ray numbers in the batch)
    uint32_t *fq_ray, *fq_cell;   // fresh rays that start inside a footprint: ray number, mask cell (k_s_cull -> k_s_fresh; k_s_ucull writes no cell)
    uint32_t *act[2];
    double *tally_part;        // TALLY_PARTS private copies of the scene's tally buffer (merged at the end of the call)
    long long tally_n;
    unsigned long long *hit_state;   // per wave of k_s_shade: open chunk of the scene's hit buffer, kept across launches
    // the hit list of a bounce parted by optics class (k_s_partition; scenes with more than one shading class): list c holds the
    // hits on surfaces of class c, resolved (surface and distance), pl_room entries each; null for classes the scene does not have
    uint32_t *pl_slot[3], *pl_surf[3];
    double *pl_t[3];
    long long pl_room;
    unsigned long long *cnt;   // CN_WORDS counters, word k at cnt[CN(k)]: see StreamCounter
};

// the footprint map of the call's source on the device (trc_footprint.h)
struct FpDev {
    trc_fp_params P;
    const uint32_t *mask, *coff, *clist;     // lists: 32-bit in global memory; k_s_fresh's LDS copies are 16-bit
    long long n_list;          // entries of clist
};

struct StreamParams {
    FastParams P;
    StreamWs W;
    long long base;      // index of the batch's first ray in the call
    long long nb;        // rays in the batch
    const uint32_t *act_in;
    uint32_t *act_out;
    unsigned hit_epoch;  // generation of the scene's hit buffer: open chunks of an older one are stale
    unsigned chunk_q1, chunk_q3;   // entries reserved per atomic in the walker / candidate queues of this launch
    long long q3_gen_chunk0;   // >= 0: k_s_gen<false> takes pre-assigned first chunks of Q3 from this chunk number on (behind k_s_walk's)
    const uint32_t *gen_list;  // k_s_gen<true>: the rays to generate (numbers in the batch, CN(CW_GEN_LIST) entries), null = all nb rays
    // A single counter word sustains ~88 returning atomics per microsecond, and the waves of a kernel run out of their chunks at
    // about the same time: 8192 waves fetching a second chunk are 0.1 ms.  So every list that a bounce fills gets ONE pre-assigned
    // chunk per appending wave, sized by the host for what the wave is expected to append (+ margin); the atomic is the rare path.
    unsigned chunk_hit;        // hit list: k_s_fresh / k_s_bounce
    unsigned chunk_slot;       // slots of the ray table: k_s_fresh
    unsigned chunk_act;        // next active list: k_s_shade
    unsigned chunk_first;      // slots and hit list: k_s_bounce<.., FRESH>
    long long slot_base0, hit_base0;   // first entry of the pre-assigned chunks of k_s_gen<true> (slots) and of k_s_exact (hit list):
                                       // behind those of k_s_fresh
    int static_general;        // the kernels of the general path have pre-assigned first chunks (not behind k_s_cull: few rays)
    FpDev fp;
    int static_first;    // the first chunk of every wave is pre-assigned (chunk_init_static): Q1 in k_s_gen, Q3 in k_s_walk,
                         // hit list in k_s_exact, active list in k_s_shade; the host starts the counters accordingly
    int lds_recs;        // k_s_exact / k_s_shade stage the surface records in LDS
    int lds_tables;      // k_s_shade also stages optics parameters, flux-map tables and capture flags
    int lds_fm_bins;     // k_s_shade: flux-map bins privatised in LDS (all of them, or 0)
    int lds_extra;       // k_s_shade: the scene's table values (optics tables: absorptance over angle / wavelength, complex indices) in LDS
                         // too -- an interpolation is a binary search, every step a dependent load
    int bounce_no;       // the bounce this launch belongs to (every ray of a launch is at the same bounce)
    int bg_occ_words;    // k_s_bounce<2>: the occupancy bits of the large grid staged in LDS (this many words), 0 = read from global memory
    int split_terminal;  // k_s_bounce lists the hits on surfaces that end every ray (TRC_SURF_TERMINAL) apart, for k_s_absorb: CN(CW_TERM_LIST),
                         // entries in the arrays of the walker queue, which is idle in a bounce that k_s_bounce serves
    unsigned chunk_thit; // ... one pre-assigned chunk per wave of k_s_bounce
    int search;          // candidate search: 0 all boxes (one leaf), 1 packed Kd-tree, 2 uniform grid
    // Shading is split by optics class (trc_shade.hip): every shading kernel of a bounce walks the same hit list and takes the
    // hits on surfaces of its class (TRC_SURF_CLS_* bits of the device copy of the surface flags).
    int shade_cls;             // the class this launch of a shading kernel serves (k_s_shade: TRC_CLS_GENERAL)
    int shade_term_cls;        // >= 0: hits on surfaces that end every ray (TRC_SURF_TERMINAL) go to the kernel of this class whatever
                               // their own, and are finished there without optics (e_out = 0 <= min_energy); -1: no such shortcut
    long long act_base0;       // first entry of the pre-assigned chunks of the active list that belong to this launch (the shading
                               // kernels of a bounce append to one list; wave w starts at act_base0 + w * chunk_act)
    unsigned chunk_hitbuf;     // entries of the scene's hit buffer a wave reserves per atomic (<= SQ_HIT_CHUNK; small buffers: less)
    // the list a shading kernel walks: the bounce's hit list (counter CN(CW_HIT_LIST)), or its class's part of it (k_s_partition, CN(CW_CLS_LIST + class))
    const uint32_t *hl_slot, *hl_surf;
    const double *hl_t;
    long long hl_room;
    int hl_cn;                 // index of the counter word that holds the list's length (CN(...) applied)
    // k_s_partition: per class, entries pre-assigned to every wave (0: the waves reserve as they go) and where those chunks start
    unsigned part_chunk[3];
    int part_static[3];
    CarryIn carry;      // (last: see CarryIn)
    // the clear cones of the scene (trc_clear_tile, trc_core.h): read by k_s_bounce for the continued rays on the LDS-sized grid alone,
    // null for a scene without them and with TRC_STREAM_CLEAR=0.  Behind everything else, for the reason given at CarryIn.
    const float *clear_tab;
    // k_s_shade_c<MIRROR, flat, LDS> finishes the next segment of a continued ray inside its clear cone itself (trc_stream_form_ahead,
    // trc_forms.h): only with split_terminal == 2 and clear_tab.  Behind everything else, for the same reason.
    int ahead;
};

// The kernel's argument block read again where it stands in the kernel-argument segment.  What a kernel reads from its by-value
// argument the compiler loads once, at the top, and keeps -- in scalar registers, and beyond ~100 of them in lanes of a vector
// register, every use then a v_readlane_b32: a vector instruction.  Read through this pointer the values are fetched by scalar
// loads where they are used, from the scalar cache, and are dead at the end of the loop body; k_s_bounce and k_s_fresh2
// call it at the top of every turn of their loops.
// It holds for a kernel whose ONLY explicit argument is one ARGS by value: the explicit arguments start at offset 0 of the segment.
// The effect (not the result) rests on the compiler not seeing through the empty asm, so that it cannot tell that the address is
// the same in every turn; a compiler that does would load the arguments once again, as before.  Figures: profiles/lean_args.txt
// (hipcc of ROCm 7.2).
template <class ARGS>
__device__ __forceinline__ const ARGS *kernel_args_again() {
    static_assert(std::is_trivially_copyable<ARGS>::value, "the block is read as the bytes the launch copied into the segment");
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const ARGS *)p;
}

// optics classes of the shading stage.  MIRROR and DIFFUSE are served by lean kernels (trc_shade.hip: <= 128 registers, four
// waves per SIMD and more); everything else -- refraction, media, conductors, incidence-angle modifiers -- by k_s_shade
// (TRC_CLS_*, trc_shade_class_of: trc_forms.h).
#define TRC_SURF_CLS_SHIFT 17  /* device copy of the surface flags only: bits 17-18 = class */
#define TRC_SURF_CLS_MASK 0x3
// ================================================================================================
// hit bookkeeping of the streaming kernels that finish hits (k_s_shade, k_s_shade_c, k_s_shade_x, k_s_absorb, k_s_bounce)
// ================================================================================================
// the next index of a loop over the threads of a workgroup of THREADS threads (0: blockDim.x, read where the loop steps)
template <int THREADS>
__device__ __forceinline__ int wg_next(int i) {
    if constexpr (THREADS > 0) return i + THREADS;
    else return i + blockDim.x;
}

// the nearest of a ray's linked candidates (general path: from `k`, its last one, through q3n); on equal t the lowest surface index
// (tracer_engine.py:58-63).  t and s come in as the best so far (TRC_INF and 0x7FFFFFFF: none).
__device__ __forceinline__ void nearest_linked(const SCand *q3n, uint32_t k, double &t, int &s) {
    while (k != SQ_INVALID) {
        const SCand c = q3n[k];
        if (c.t < t || (c.t == t && (int)c.surf < s)) { t = c.t; s = (int)c.surf; }
        k = c.next;
    }
}

// leaving the flat surface `rec` from (hx, hy, hz) along (ox, oy, oz), the ray cannot meet it again when its own plane test is certain
// to give t < 1e-7 (flat_surface.py:39-51: t = -((p - c).n) / (d.n), the hit point p is on the plane up to rounding): SQ_SKIP_SELF
__device__ __forceinline__ bool leaves_flat(const double *rec, double hx, double hy, double hz, double ox, double oy, double oz) {
    if (!trc_gm_is_flat(trc_rec_gm_kind(rec))) return false;
    const double dtn = ox * rec[2] + oy * rec[5] + oz * rec[8];
    const double vt = rec[2] * (hx - rec[9]) + rec[5] * (hy - rec[10]) + rec[8] * (hz - rec[11]);
    const double scale = 1.0 + fabs(hx) + fabs(hy) + fabs(hz) + fabs(rec[9]) + fabs(rec[10]) + fabs(rec[11]);
    return fabs(dtn) > 1e-6 && fabs(vt) + 1e-12 * scale < 5e-8 * fabs(dtn);
}

// The real (unpadded) counts of a kernel that finishes hits, one atomic per counter word and workgroup -- they all land on the same
// words at the end of the kernel: every wave adds its hits and its rays that go on into the two spare words `spare` in LDS, then
// thread 0 adds the hits to c_hit and c_hit2 and the rays to c_alive (null: the kernel keeps no ray alive).  IF_ANY: only counts
// that are not 0.
template <bool IF_ANY>
__device__ __forceinline__ void flush_counts(double *spare, unsigned n_hit, unsigned n_alive, unsigned long long *c_hit,
                                             unsigned long long *c_hit2, unsigned long long *c_alive) {
    const double h = wave_sum((double)n_hit), a = wave_sum((double)n_alive);
    if (lane_id() == 0) { atomicAdd(&spare[0], h); if (c_alive) atomicAdd(&spare[1], a); }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (!IF_ANY || spare[0] > 0.0) { atomicAdd(c_hit, (unsigned long long)(spare[0] + 0.5)); atomicAdd(c_hit2, (unsigned long long)(spare[0] + 0.5)); }
        if (c_alive && (!IF_ANY || spare[1] > 0.0)) atomicAdd(c_alive, (unsigned long long)(spare[1] + 0.5));
    }
}

// adds what the workgroup summed in LDS to its copy of the tally buffer, each word that is not 0: the n_sums per-surface sums, then
// the private copy of the flux-map bins (fm_bins of them at l_fm, null: none), which follow the 3S+2 sums in the tally buffer
template <int THREADS = 0>
__device__ __forceinline__ void flush_sums(double *tally, const double *l_sums, int n_sums, const double *l_fm, int fm_bins, int n_surf) {
    for (int i = threadIdx.x; i < n_sums; i = wg_next<THREADS>(i)) {
        const double v = l_sums[i];
        if (v != 0.0) atomicAdd(&tally[i], v);
    }
    if (l_fm) {
        double *gt = tally + 3 * n_surf + 2;
        for (int i = threadIdx.x; i < fm_bins; i = wg_next<THREADS>(i)) {
            const double v = l_fm[i];
            if (v != 0.0) atomicAdd(&gt[i], v);
        }
    }
}

// The three sums of a surface (absorbed, incident, hits) for the hit of every lane (ts: its surface, < 0: none): 64 lanes adding to one
// word take 64 turns, in LDS and in global memory alike.  While at least `share` lanes are on the surface of the first lane still to
// be served, they are summed in registers and added once, for ROUNDS surfaces at most; the other lanes add for themselves.
// share == 0: no lanes to share with (a field of hundreds of mirrors), every lane adds for itself.
template <int ROUNDS>
__device__ __forceinline__ void tally_by_wave(double *tl, int Sn, int ts, double tea, double tei, int share) {
    unsigned long long todo = share > 0 ? __ballot(ts >= 0) : 0ull;
    for (int round = 0; round < ROUNDS && todo; ++round) {
        const int s0 = __shfl(ts, __ffsll((long long)todo) - 1, 64);
        const bool in = ts == s0;
        const unsigned long long m = __ballot(in);
        if (__popcll(m) < share) break;
        const double a = wave_sum(in ? tea : 0.0), b = wave_sum(in ? tei : 0.0);
        if (lane_id() == 0) { atomicAdd(&tl[s0], a); atomicAdd(&tl[Sn + s0], b); atomicAdd(&tl[2 * Sn + s0], (double)__popcll(m)); }
        if (in) ts = -1;
        todo &= ~m;
    }
    if (ts >= 0) { atomicAdd(&tl[ts], tea); atomicAdd(&tl[Sn + ts], tei); atomicAdd(&tl[2 * Sn + ts], 1.0); }
}

// the lean shading kernels (trc_shade.hip): kernel of a class for a scene of flat surfaces only (flat) with its tables in LDS (lds)
// chart: the instance that knows every flux-map chart (record_hit<.., CHART>) -- of the lean kernels the ones for any geometry only
const void *trc_shade_carry_kernel(bool lds, bool chart = false, bool split = false, bool mat = false);      // k_s_shade_x (trc_shade.hip): every optics kind, with what the rays carry;
                                                                                            // split: its form for scenes whose optics send two rays on from a hit
const void *trc_shade_lean_kernel(int cls, bool flat, bool lds, bool spec = false, bool chart = false);
const void *trc_shade_poly_kernel(bool lds, bool chart, bool split);        // k_s_shade_p (trc_shade.hip): k_s_shade_x for a source that carries its spectrum

__device__ __forceinline__ trc_accel_view stream_accel_global(const DScene &sc, int mode) {
    const bool kd32 = mode == 1;
    trc_accel_view A;
    A.sbox = sc.a_sbox; A.nodes = kd32 ? sc.a_nodes : nullptr; A.leaf_surfs = kd32 ? sc.a_leaf : sc.a_bleaf;
    // surfaces tested for every ray besides the search structure: the Kd-tree's always-relevant ones, or those set apart
    // from the grid
    A.always = mode == 2 ? sc.a_gapart : sc.kd_always; A.unbounded = sc.a_unbounded;
    A.n_always = kd32 ? sc.kd_nalways : (mode == 2 ? sc.a_g_napart : 0); A.n_unbounded = sc.a_n_unbounded; A.n_surf = sc.n_surf; A.has_kd = 1;
#pragma unroll
    for (int i = 0; i < 6; ++i) A.root[i] = kd32 ? sc.a_root[i] : (mode == 2 ? sc.a_groot[i] : sc.a_broot[i]);
    A.delta = sc.a_delta;
#pragma unroll
    for (int i = 0; i < 3; ++i) { A.cen[i] = sc.a_cen[i]; A.slo[i] = sc.a_slo[i]; A.shi[i] = sc.a_shi[i]; }
    return A;
}

// Nearest hit of ONE ray through the large grid, one lane per ray (the ordered engine on a scene that stands on the large grid:
// a mesh of 1e5 faces, where testing every surface for every ray -- what the engine did -- took 370 ms per 2e5 rays).  The cells
// of the DDA with the occupancy bits, the listed faces from their 48-byte entries (trc_tri_hit32 / box and oriented box), the exact
// test at once; the walk ends at the first cell behind the nearest hit.  Same candidates, same exact test and tie rule as
// k_s_bounce<2> and trc_nearest_brute: t > 0, the lowest index among equal distances.  *s_out < 0: no hit.
__device__ __forceinline__ void trc_nearest_grid32(const DScene &sc, double px, double py, double pz, double dx, double dy, double dz,
                                                    double *t_out, int *s_out) {
    trc_accel_view A = stream_accel_global(sc, 0);
#pragma unroll
    for (int i = 0; i < 6; ++i) A.root[i] = sc.a_bg_root[i];
    trc_grid_view32 G;
    memset(&G, 0, sizeof(G));
    G.off = sc.a_bg_off; G.list = nullptr;
    G.nx = sc.a_bg_dim[0]; G.ny = sc.a_bg_dim[1]; G.nz = sc.a_bg_dim[2];
    G.lox = sc.a_bg_lo[0]; G.loy = sc.a_bg_lo[1]; G.loz = sc.a_bg_lo[2];
    G.csx = sc.a_bg_cs[0]; G.csy = sc.a_bg_cs[1]; G.csz = sc.a_bg_cs[2];
    G.ivx = sc.a_bg_inv[0]; G.ivy = sc.a_bg_inv[1]; G.ivz = sc.a_bg_inv[2];
    double tb = TRC_INF;
    int sb = 0x7FFFFFFF;
    auto exact = [&](int s) __attribute__((always_inline)) {
        const double t = trc_intersect(sc.recs + (size_t)s * sc.stride, sc.extra, px, py, pz, dx, dy, dz);
        if (t > 0.0 && t < TRC_INF && (t < tb || (t == tb && s < sb))) { tb = t; sb = s; }
    };
    for (int k = 0; k < A.n_unbounded; ++k) exact(A.unbounded[k]);
    trc_ray32 r;
    double t0 = 0.0;
    if (trc_ray32_prepare(A.slo, A.shi, A.cen, px, py, pz, dx, dy, dz, &r, &t0)) {
        for (int k = 0; k < sc.a_bg_napart; ++k) {        // surfaces set apart from the grid
            const int sidx = sc.a_bg_apart[k];
            const float *b = A.sbox + 6 * (size_t)sidx;
            if (b[3] == TRC_INF && b[0] == -TRC_INF) continue;
            if (trc_box_hit32(b, r) && trc_obb_hit32(sc.a_obb + (size_t)TRC_OBB_STRIDE * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz)) exact(sidx);
        }
        float tmin = 1.0f, tmax = 0.0f;
        if (trc_kd32_root(A.root, r, &tmin, &tmax)) {
            const float4 *ent = (const float4 *)sc.a_bg_ent;
            trc_dda dd;
            trc_dda_start(G, r, tmin, &dd);
            float t_enter = tmin;
            bool walk = true;
            while (walk) {
                if (sb != 0x7FFFFFFF) {
                    const float tbr = (float)(tb - t0);
                    if (tbr < t_enter - (1e-3f + 1e-4f * fabsf(tbr))) break;      // every cell from here on starts behind the best hit
                }
                const int cell = trc_dda_cell(G, dd);
                if ((sc.a_bg_occ[cell >> 5] >> (cell & 31)) & 1u) {
                    const uint32_t k1 = G.off[cell + 1];
                    for (uint32_t k = G.off[cell]; k < k1; ++k) {
                        const float4 c0 = ent[3 * (size_t)k], c1 = ent[3 * (size_t)k + 1], c2 = ent[3 * (size_t)k + 2];
                        const uint32_t w = __float_as_uint(c0.x);
                        const int sidx = (int)(w & 0x7FFFFFFFu);
                        bool pass;
                        if (!(w & 0x80000000u)) pass = trc_tri_hit32(c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, A.delta, r);
                        else {
                            const float b[6] = {c0.y, c0.z, c0.w, c1.x, c1.y, c1.z};
                            pass = trc_box_hit32(b, r) && trc_obb_hit32(sc.a_obb + (size_t)TRC_OBB_STRIDE * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
                        }
                        if (pass) exact(sidx);
                    }
                }
                t_enter = fminf(dd.tnx, fminf(dd.tny, dd.tnz));
                walk = trc_dda_next(G, r, tmax, &dd);
            }
        }
    }
    *t_out = sb != 0x7FFFFFFF ? tb : 0.0;
    *s_out = sb != 0x7FFFFFFF ? sb : -1;
}

// ---------------------------------------------------------------------------------------------------------------
// capacity of the ray table and of the lists of slots / ray numbers: rays per batch + room for the unused tails of the chunks
#define SQ_ROOM(W) ((W).room)

// ================================================================================================
// shared pieces of the streaming kernels that find a ray's first or next surface (k_s_fresh, k_s_fresh2, k_s_bounce)
// ================================================================================================
// Copies the parts of the search tables' LDS image that `p` names (trc_search_lds_layout, trc_bounds.h) from global memory, in the
// order of the image; every thread of the workgroup calls it, the caller's next barrier makes the copies visible.  The footprint
// lists are 32-bit in global memory and 16-bit here.
template <int THREADS>
__device__ __forceinline__ void stage_search_tables(char *lds, const trc_lds_layout &L, const trc_lds_parts &p, const DScene &sc, const FpDev &fp,
                                                    int tid) {
    const int Sn = p.n_surf;
    if (p.occ_words > 0) {
        uint32_t *l_occ = (uint32_t *)(lds + L.occ);
        for (int i = tid; i < p.occ_words; i += THREADS) l_occ[i] = sc.a_bg_occ[i];
    }
    if (p.tables) {
        double *lr = (double *)(lds + L.recs);
        for (int i = tid; i < Sn * p.stride; i += THREADS) lr[i] = sc.recs[i];
        float *lb = (float *)(lds + L.obb);
        for (int i = tid; i < Sn * TRC_OBB_STRIDE; i += THREADS) lb[(i / TRC_OBB_STRIDE) * TRC_OBB_LSTRIDE + i % TRC_OBB_STRIDE] = sc.a_obb[i];
    }
    if (p.sbox) {
        float *ls = (float *)(lds + L.sbox);
        for (int i = tid; i < Sn * 6; i += THREADS) ls[i] = sc.a_sbox[i];
    }
    if (p.flags) {
        int32_t *lf = (int32_t *)(lds + L.flags);
        for (int i = tid; i < Sn; i += THREADS) lf[i] = sc.sflags[i];
    }
    if (p.fp_offs) {
        uint16_t *lo = (uint16_t *)(lds + L.fp_off), *ll = (uint16_t *)(lds + L.fp_list);
        for (int i = tid; i < p.fp_offs; i += THREADS) lo[i] = (uint16_t)fp.coff[i];
        for (int i = tid; i < p.fp_list; i += THREADS) ll[i] = (uint16_t)fp.clist[i];
    }
    if (p.grid_cells) {
        uint16_t *l_goff = (uint16_t *)(lds + L.grid_off), *l_list = (uint16_t *)(lds + L.grid_list);
        for (int i = tid; i < p.grid_cells + 1; i += THREADS) l_goff[i] = sc.a_goff[i];
        for (int i = tid; i < p.grid_list; i += THREADS) l_list[i] = sc.a_glist[i];
    }
}

// The two passes of the Buie table's LDS form (trc_buie_fast_fill) with the barrier behind each: every thread of the workgroup
// reaches both barriers, whatever `want` says (the source is a Buie one and the kernel samples it).
__device__ __forceinline__ void buie_tables_fill(const trc_source_desc *src, trc_buie_fast *l_bf, int tid, int nth, bool want) {
    if (want) trc_buie_fast_fill(src->buie, l_bf, 0, tid, nth);
    __syncthreads();
    if (want) trc_buie_fast_fill(src->buie, l_bf, 1, tid, nth);
    __syncthreads();
}

// A fresh ray takes `slot` of the ray table: no candidate linked, bounce 0, left no surface.  Rays of a source descriptor all
// carry (energy, 1, 0), written at their first hit; given rays bring their own (the second form).
__device__ __forceinline__ void store_fresh_ray(const StreamWs &W, unsigned long long slot, uint32_t ri, double px, double py, double pz,
                                                double dx, double dy, double dz) {
    SRayGeo g;
    g.px = px; g.py = py; g.pz = pz; g.dx = dx; g.dy = dy; g.dz = dz;
    g.head = SQ_INVALID;
    g.idx = ri;
    g.tail = sray_tail(0, 0u);
    W.geo[slot] = g;
}
__device__ __forceinline__ void store_fresh_ray(const StreamWs &W, unsigned long long slot, uint32_t ri, double px, double py, double pz,
                                                double dx, double dy, double dz, double e, double ref, double wl) {
    store_fresh_ray(W, slot, ri, px, py, pz, dx, dy, dz);
    SRayAux a;
    a.e = e; a.ref = ref; a.wl = wl; a.pad = 0.0;
    W.aux[slot] = a;
}

// entry q of the hit list: the ray in `slot` hits surface `surf` at distance t
__device__ __forceinline__ void store_hit(const StreamWs &W, unsigned long long q, uint32_t slot, int surf, double t) {
    W.hit_slot[q] = slot; W.hit_surf[q] = (uint32_t)surf; W.hit_t[q] = t;
}
// One listed fresh ray per lane (k_s_fresh's loop body, k_s_fresh2's second phase): ray `ri` of the batch, whose start point lies in
// mask cell `cell` of the footprint map, or an inactive lane.  The float64 ray exactly as k_s_gen makes it (trc_source_ray_t, same
// stream), the surfaces listed for its cell, their oriented boxes in float32, 32 at a time, then the exact float64 tests of those
// that pass -- each lane pops its own -- with the reference's tie rule: nearest, lowest surface index on equal t.  A ray that hits
// takes the next slot of the ray table (cs) and goes to the hit list (ch) with its surface and distance.  Called by the whole wave.
// LDS: records, boxes and lists are the LDS copies (16-bit lists), else the global tables (32-bit lists).
template <bool LDS> using fp_list_t = typename std::conditional<LDS, uint16_t, uint32_t>::type;
template <int KIND, bool FLAT, bool LDS>
__device__ __forceinline__ void listed_ray_search(const StreamParams &S, const trc_buie_fast *l_bf, const double *recs, const float *obb,
                                                  const fp_list_t<LDS> *l_coff, const fp_list_t<LDS> *clist, WaveChunk &cs, WaveChunk &ch,
                                                  bool active, uint32_t ri, uint32_t cell) {
    const FastParams &P = S.P;
    const DScene &sc = P.sc;
    const StreamWs &W = S.W;
    const trc_fp_params &F = S.fp.P;
    double px = 0, py = 0, pz = 0, dx = 0, dy = 0, dz = 1;
    double tb = TRC_INF;
    int sb = 0x7FFFFFFF;
    if (active) {
        const unsigned long long rid = P.ray_offset + (unsigned long long)(S.base + ri);
        trc_source_ray_t<KIND>(P.src, nullptr, nullptr, P.seed, rid, &px, &py, &pz, &dx, &dy, &dz, l_bf);
    }
    // float32 copy for the box tests, taken after an advance that no surface is nearer than, relative to the scene centre
    const float ox = (float)(px + F.t_adv * dx - sc.a_cen[0]), oy = (float)(py + F.t_adv * dy - sc.a_cen[1]), oz = (float)(pz + F.t_adv * dz - sc.a_cen[2]);
    const float ex = (float)dx, ey = (float)dy, ez = (float)dz;
    uint32_t k0 = 0, k1 = 0;
    if (active) {
        const uint32_t c = ((cell >> 16) >> TRC_FP_SHIFT) * (uint32_t)F.Mc + ((cell & 0xFFFFu) >> TRC_FP_SHIFT);
        if (LDS) { k0 = l_coff[c]; k1 = l_coff[c + 1]; }
        else { k0 = S.fp.coff[c]; k1 = S.fp.coff[c + 1]; }
    }
    for (uint32_t kb = k0; __ballot(kb < k1); kb += 32) {
        unsigned hits = 0;
        for (uint32_t k = kb; k < kb + 32 && k < k1; ++k) {
            const uint32_t sidx = clist[k];
            if (trc_obb_hit32(obb + (size_t)(LDS ? TRC_OBB_LSTRIDE : TRC_OBB_STRIDE) * sidx, ox, oy, oz, ex, ey, ez)) hits |= 1u << (k - kb);
        }
        while (__ballot(hits != 0)) {
            if (hits != 0) {
                const int sidx = (int)clist[kb + (uint32_t)__ffs((int)hits) - 1u];
                const double *rec = recs + (size_t)sidx * sc.stride;
                double t = FLAT ? trc_intersect_flat(trc_rec_gm_kind(rec), rec, sc.extra, px, py, pz, dx, dy, dz)
                                : trc_intersect(rec, sc.extra, px, py, pz, dx, dy, dz);
                if (!(t > 0.0) || !(t < TRC_INF)) t = TRC_INF;      // t == 0 is not a hit (tracer_engine.py:58)
                if (t < tb || (t == tb && t < TRC_INF && sidx < sb)) { tb = t; sb = sidx; }      // tracer_engine.py:58-63
                hits &= hits - 1u;
            }
        }
    }
    const bool hit = active && tb < TRC_INF;
    const unsigned long long sl = chunk_append(&W.cnt[CN(CW_SLOTS)], cs, hit, nullptr, 0);
    const unsigned long long qh = chunk_append(&W.cnt[CN(CW_HIT_LIST)], ch, hit, W.hit_slot, SQ_ROOM(W));
    if (hit) {
        if ((long long)sl < SQ_ROOM(W) && (long long)qh < SQ_ROOM(W)) {
            store_fresh_ray(W, sl, ri, px, py, pz, dx, dy, dz);
            store_hit(W, qh, (uint32_t)sl, sb, tb);
        } else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL;
    }
}

#endif
