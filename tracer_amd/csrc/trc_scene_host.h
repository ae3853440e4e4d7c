// trc_scene_host.h -- the arithmetic of a scene's host side, free of HIP: the record stride and what the optics ask of the rays, the
// order in which the search tables are built, the one validation of a caller's Kd-tree with its packing, and the layout of the
// tally buffer.  The library (trc_scene.h: the owners inside trc_scene, which hold device memory and so need HIP) and the host
// checks (tests/hostcheck, tests/scenecheck) read the same functions.
#ifndef TRC_SCENE_HOST_H
#define TRC_SCENE_HOST_H

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <vector>
#include "trc_bounds.h"

// what the scene's optics read that rays carry beyond the nine columns: the highest material row named by a surface between
// tabulated materials (-1: none) and whether some wall is polychromatic.  Found once: optics do not change after creation.
struct CarryNeeds {
    int max_mat = -1;
    bool poly = false;
    bool any() const { return max_mat >= 0 || poly; }
};

// the reason of a refusal into msg, its status returned
static inline int trc_refuse(char *msg, size_t len, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, len, fmt, ap);
    va_end(ap);
    return code;
}

// surface idx of a scene with n_extra extra values, before anything is built from it: TRC_OK, or the status and the reason in msg
static inline int trc_surface_check(const trc_surface_desc &s, int idx, int n_extra, char *msg, size_t len) {
#define TRC_REFUSE(code, ...) return trc_refuse(msg, len, code, __VA_ARGS__)
    if (s.gm_kind < 0 || s.gm_kind >= TRC_GM_KIND_COUNT)
        TRC_REFUSE(TRC_ERR_UNSUPPORTED, "surface %d: geometry kind %d is not in the native table", idx, s.gm_kind);
    if (s.optics_kind < 0 || s.optics_kind >= TRC_OPT_KIND_COUNT)
        TRC_REFUSE(TRC_ERR_UNSUPPORTED, "surface %d: optics kind %d is not in the native table", idx, s.optics_kind);
    if (s.optics_kind == TRC_OPT_REFRACTIVE_SCATTERING) {
        if (s.opt[2] == 0.0) TRC_REFUSE(TRC_ERR_UNSUPPORTED, "surface %d: scattering optics emit one ray per interaction (single_ray)", idx);
        if (s.extra_off < 0 || s.extra_len < 4 || s.extra_off + s.extra_len > n_extra)
            TRC_REFUSE(TRC_ERR_INVALID, "surface %d: scattering optics need s_c1, s_c2, g1, g2 in the extra values", idx);
        if (s.gm_kind == TRC_GM_RECT_PERFORATED || s.gm_kind == TRC_GM_POLYGON)
            TRC_REFUSE(TRC_ERR_UNSUPPORTED, "surface %d: scattering optics share the extra range with the geometry", idx);
    }
    bool opt_table = s.optics_kind == TRC_OPT_REFLECTIVE_SPECTRAL || s.optics_kind == TRC_OPT_LAMBERTIAN_DIRECTIONAL ||
                     s.optics_kind == TRC_OPT_LAMBERTIAN_DIRECTIONAL_SPECTRAL || s.optics_kind == TRC_OPT_FRESNEL_CONDUCTOR ||
                     s.optics_kind == TRC_OPT_LAMBERTIAN_POLYCHROMATIC;
    if (s.optics_kind == TRC_OPT_REFRACTIVE_MATERIAL && (s.opt[4] < 0 || s.opt[5] < 0 || s.opt[4] >= 64 || s.opt[5] >= 64))
        TRC_REFUSE(TRC_ERR_INVALID, "surface %d: material rows out of range", idx);
    bool needs_extra = s.gm_kind == TRC_GM_RECT_PERFORATED || opt_table;
    if (needs_extra && (s.extra_off < 0 || s.extra_len <= 0 || s.extra_off + s.extra_len > n_extra))
        TRC_REFUSE(TRC_ERR_INVALID, "surface %d: extra range [%d,+%d) outside the %d extra values", idx, s.extra_off, s.extra_len, n_extra);
    if (s.gm_kind == TRC_GM_RECT_PERFORATED && opt_table)
        TRC_REFUSE(TRC_ERR_UNSUPPORTED, "surface %d: perforated plate with spectral optics shares one extra range", idx);
    // reference argument checks (flat_surface.py:192-195, :470-480; sphere_surface.py:31-32; cone.py:82-83)
    const double *g = s.gm;
    switch (s.gm_kind) {
    case TRC_GM_RECT: case TRC_GM_RECT_EXTRUDED: case TRC_GM_RECT_PERFORATED:
        if (!(g[0] > 0) || !(g[1] > 0)) TRC_REFUSE(TRC_ERR_INVALID, "surface %d: width and height must be positive", idx);
        break;
    case TRC_GM_ROUND: case TRC_GM_ROUND_CUT:
        if (!(g[0] > 0)) TRC_REFUSE(TRC_ERR_INVALID, "surface %d: radius must be positive", idx);
        if (g[1] >= 0 && !(g[1] < g[0])) TRC_REFUSE(TRC_ERR_INVALID, "surface %d: inner radius must be lower than the outer one", idx);
        break;
    case TRC_GM_SPHERE: case TRC_GM_HEMISPHERE: case TRC_GM_SPHERE_RECT: case TRC_GM_SPHERE_CUT:
        if (!(g[0] > 0)) TRC_REFUSE(TRC_ERR_INVALID, "surface %d: radius must be positive", idx);
        break;
    default: break;
    }
    return TRC_OK;
}

// doubles per surface record: the header and the longest parameter list, made odd (spreads records over LDS banks)
static inline int trc_scene_stride(const trc_surface_desc *surfs, int n) {
    int max_np = 0;
    for (int i = 0; i < n; ++i) max_np = std::max(max_np, trc_gm_nparams(surfs[i].gm_kind));
    return (TRC_REC_HDR + max_np) | 1;
}

// a surface's record of `stride` doubles: the frame (rotation, then translation), four 32-bit words (kinds, extra range), the geometry
static inline void trc_pack_record(const trc_surface_desc &s, double *rec, int stride) {
    for (int i = 0; i < stride; ++i) rec[i] = 0.0;
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) rec[3 * r + k] = s.frame[4 * r + k];
        rec[9 + r] = s.frame[4 * r + 3];
    }
    int32_t *h = (int32_t *)(rec + 12);
    h[0] = s.gm_kind; h[1] = s.optics_kind; h[2] = s.extra_off; h[3] = s.extra_len;
    int np = trc_gm_nparams(s.gm_kind);
    for (int i = 0; i < np; ++i) rec[TRC_REC_HDR + i] = s.gm[i];
}

// *splits: some optics can emit two rays per hit; *needs: see CarryNeeds
static inline void trc_scene_scan(const trc_surface_desc *surfs, int n, bool *splits, CarryNeeds *needs) {
    *splits = false;
    *needs = CarryNeeds();
    for (int i = 0; i < n; ++i) {
        const trc_surface_desc &s = surfs[i];
        if (s.optics_kind == TRC_OPT_REFRACTIVE_HOMOGENOUS && s.opt[2] == 0.0) *splits = true;
        if (s.optics_kind == TRC_OPT_REFRACTIVE_MATERIAL && s.opt[0] == 0.0) *splits = true;
        if (s.optics_kind == TRC_OPT_REFRACTIVE_MATERIAL) needs->max_mat = std::max(needs->max_mat, std::max((int)s.opt[4], (int)s.opt[5]));
        if (s.optics_kind == TRC_OPT_LAMBERTIAN_POLYCHROMATIC) needs->poly = true;
    }
}

// The search tables of a scene, in the order every scene gets them: the boxes, the LDS-sized grid with the clear cones of the surfaces
// listed in it, and the 32-bit grid for a scene the LDS-sized one cannot hold.  force32 (TRC_GRID_FORCE32, for measurements): the large grid for a scene the small one holds.
static inline void trc_search_tables_build(const trc_surface_desc *surfs, int n, bool force32, trc_accel_host &A) {
    trc_accel_build_surfaces(surfs, n, A);
    trc_accel_build_grid(A, n);
    if (force32) A.grid_ok = false;
    trc_clear_build(surfs, n, TRC_CLEAR_T, A);      // (the clear cones belong to the LDS-sized grid: none without it)
    if (!A.grid_ok) trc_accel_build_grid32(surfs, n, A);
}

// A caller's Kd-tree before anything indexes it: counts non-negative and below 2^29, every array there when its count is positive,
// flags 0..3, children in range and behind their parent, leaf ranges (in 64 bits) inside leaf_surfs, every listed surface in
// [0, n_surf).  TRC_OK and the tree's depth, or TRC_ERR_INVALID and the reason in msg.
#define TRC_KD_MAX_COUNT (1 << 29)
static inline int trc_kd_check(const trc_kdtree_desc *kd, int n_surf, int *max_depth_out, char *msg, size_t len) {
    *max_depth_out = 0;
    if (kd->n_nodes <= 0 || kd->n_leaf_surfs < 0 || kd->n_always < 0) TRC_REFUSE(TRC_ERR_INVALID, "incomplete tree (%d nodes, %d leaf entries, %d always relevant)", kd->n_nodes, kd->n_leaf_surfs, kd->n_always);
    if (kd->n_nodes >= TRC_KD_MAX_COUNT || kd->n_leaf_surfs >= TRC_KD_MAX_COUNT || kd->n_always >= TRC_KD_MAX_COUNT) TRC_REFUSE(TRC_ERR_INVALID, "tree too large");
    if (!kd->flag || !kd->split || !kd->child || !kd->leaf_off || !kd->leaf_cnt || (kd->n_leaf_surfs > 0 && !kd->leaf_surfs) ||
        (kd->n_always > 0 && !kd->always_relevant)) TRC_REFUSE(TRC_ERR_INVALID, "incomplete tree (an array is missing)");
    std::vector<int32_t> depth((size_t)kd->n_nodes, 0);
    for (int i = 0; i < kd->n_nodes; ++i) {
        const int f = kd->flag[i];
        if (f < 0 || f > 3) TRC_REFUSE(TRC_ERR_INVALID, "node %d: flag %d", i, f);
        if (f == 3) {
            const int64_t off = kd->leaf_off[i], cnt = kd->leaf_cnt[i];
            if (off < 0 || cnt < 0 || off + cnt > (int64_t)kd->n_leaf_surfs) TRC_REFUSE(TRC_ERR_INVALID, "node %d: leaf range", i);
        } else {
            const int64_t c = kd->child[i];
            if (c <= i || c + 1 >= (int64_t)kd->n_nodes) TRC_REFUSE(TRC_ERR_INVALID, "node %d: child %d out of range", i, (int)c);
            depth[c] = depth[c + 1] = depth[i] + 1;
            if (depth[c] > *max_depth_out) *max_depth_out = depth[c];
        }
    }
    for (int i = 0; i < kd->n_leaf_surfs; ++i)
        if (kd->leaf_surfs[i] < 0 || kd->leaf_surfs[i] >= n_surf) TRC_REFUSE(TRC_ERR_INVALID, "leaf entry %d: surface %d out of range", i, kd->leaf_surfs[i]);
    for (int i = 0; i < kd->n_always; ++i)
        if (kd->always_relevant[i] < 0 || kd->always_relevant[i] >= n_surf) TRC_REFUSE(TRC_ERR_INVALID, "always-relevant surface %d out of range", kd->always_relevant[i]);
    return TRC_OK;
}

#undef TRC_REFUSE

// the two words per node the float64 walk reads (k_trace_fast, k_ord_bounce), of a tree trc_kd_check accepted:
// a = child << 2 | axis, b = 0 of an interior node; a = leaf_off << 2 | 3, b = leaf_cnt of a leaf
static inline void trc_kd_pack(const trc_kdtree_desc *kd, std::vector<int32_t> &a, std::vector<int32_t> &b) {
    a.assign((size_t)kd->n_nodes, 0);
    b.assign((size_t)kd->n_nodes, 0);
    for (int i = 0; i < kd->n_nodes; ++i) {
        const int f = kd->flag[i];
        if (f == 3) { a[i] = (kd->leaf_off[i] << 2) | 3; b[i] = kd->leaf_cnt[i]; }
        else a[i] = (kd->child[i] << 2) | f;
    }
}

// The tally buffer of S surfaces: [absorbed S | received S | count S | segments, hits | bins of every flux map ... | transfer (S+1) x S].
// bins[k]: where map k's nu * nv bins start; tr_off: where the transfer matrix starts, -1 when it is not kept (it comes last: the
// bins keep their offsets when it is toggled); total: doubles in all.  Map: anything with nu and nv.
struct trc_tally_plan {
    std::vector<int64_t> bins;
    int64_t tr_off, total;
};
template <class Map>
static inline trc_tally_plan trc_tally_layout(int n_surf, const Map *maps, size_t n_maps, bool transfer) {
    trc_tally_plan L;
    int64_t n = 3 * (int64_t)n_surf + 2;
    for (size_t k = 0; k < n_maps; ++k) { L.bins.push_back(n); n += (int64_t)maps[k].nu * maps[k].nv; }
    L.tr_off = -1;
    if (transfer) { L.tr_off = n; n += ((int64_t)n_surf + 1) * n_surf; }
    L.total = n;
    return L;
}

#endif
