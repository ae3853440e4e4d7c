// trc_bounds.h -- host-side construction of the single-precision acceleration data used by
// trc_nearest_accel32 (trc_core.h): a conservative axis-aligned box for every bounded surface, derived from
// the surface's own geometry (never from user-declared BoundaryBoxes), the scene box and centre, the
// inflation `delta`, and the packed Kd nodes.  Plain C++ so that the test-only host build can use it too.
#ifndef TRC_BOUNDS_H
#define TRC_BOUNDS_H

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "trc_core.h"

// Box of a surface in its own frame (l, h).  Returns false for unbounded kinds.  The sphere kinds work in the global
// frame (sphere_surface.py:58-66): their box is centred on the frame's origin with the GLOBAL axes (*global_axes = true).
// Every point the exact test of the kind can return lies inside the box (aperture rules of trc_core.h).
static inline bool trc_surface_local_box(const trc_surface_desc &s, double l[3], double h[3], bool *global_axes) {
    const double *g = s.gm;
    *global_axes = false;
    switch (s.gm_kind) {
    case TRC_GM_RECT: case TRC_GM_RECT_EXTRUDED: case TRC_GM_RECT_PERFORATED:
        l[0] = -g[0]; h[0] = g[0]; l[1] = -g[1]; h[1] = g[1]; l[2] = h[2] = 0.0; break;
    case TRC_GM_ROUND: case TRC_GM_ROUND_CUT:
        l[0] = l[1] = -g[0]; h[0] = h[1] = g[0]; l[2] = h[2] = 0.0; break;
    case TRC_GM_TRIANGLE:
        for (int i = 0; i < 3; ++i) { l[i] = std::fmin(0.0, std::fmin(g[i], g[3 + i])); h[i] = std::fmax(0.0, std::fmax(g[i], g[3 + i])); }
        break;
    case TRC_GM_POLYGON:
        l[0] = g[2]; h[0] = g[3]; l[1] = g[4]; h[1] = g[5]; l[2] = h[2] = 0.0; break;
    case TRC_GM_PARAB_DISH: {
        double rx = std::sqrt(g[2] / g[0]), ry = std::sqrt(g[2] / g[1]);
        l[0] = -rx; h[0] = rx; l[1] = -ry; h[1] = ry; l[2] = 0.0; h[2] = g[2]; break;
    }
    case TRC_GM_PARAB_HEX:
        l[0] = l[1] = -g[2]; h[0] = h[1] = g[2]; l[2] = 0.0; h[2] = (g[0] + g[1]) * g[2] * g[2]; break;
    case TRC_GM_PARAB_RECT:
        l[0] = -g[2]; h[0] = g[2]; l[1] = -g[3]; h[1] = g[3]; l[2] = 0.0; h[2] = g[0] * g[2] * g[2] + g[1] * g[3] * g[3]; break;
    case TRC_GM_PARAB_TROUGH: {
        double rx = std::sqrt(g[2] / g[0]);
        l[0] = -rx; h[0] = rx; l[1] = -g[1]; h[1] = g[1]; l[2] = 0.0; h[2] = g[2]; break;
    }
    case TRC_GM_SPHERE: case TRC_GM_HEMISPHERE: case TRC_GM_SPHERE_RECT: case TRC_GM_SPHERE_CUT:
        for (int i = 0; i < 3; ++i) { l[i] = -g[0]; h[i] = g[0]; }
        *global_axes = true;
        break;
    case TRC_GM_CYL_FINITE: case TRC_GM_CYL_RECTCUT:
        l[0] = l[1] = -g[0]; h[0] = h[1] = g[0]; l[2] = -g[1]; h[2] = g[1]; break;
    case TRC_GM_CONE_FINITE: {
        double r = std::fabs(g[0]) * std::fmax(std::fabs(0.0 - g[1]), std::fabs(g[2] - g[1]));
        l[0] = l[1] = -r; h[0] = h[1] = r; l[2] = 0.0; h[2] = g[2]; break;
    }
    case TRC_GM_FRUSTUM: case TRC_GM_FRUSTUM_RECTCUT: {
        double r = std::fabs(g[0]) * std::fmax(std::fabs(g[2] - g[1]), std::fabs(g[3] - g[1]));
        l[0] = l[1] = -r; h[0] = h[1] = r; l[2] = g[2]; h[2] = g[3];
        if (s.gm_kind == TRC_GM_FRUSTUM_RECTCUT) { l[0] = -std::fmin(r, g[4]); h[0] = -l[0]; l[1] = -std::fmin(r, g[5]); h[1] = -l[1]; }
        break;
    }
    case TRC_GM_QUADRATIC_RECT: {
        double w = g[6], hh = g[7];
        double m = std::fabs(g[0]) * w * w + std::fabs(g[1]) * hh * hh + std::fabs(g[2]) * w * hh + std::fabs(g[3]) * w +
                   std::fabs(g[4]) * hh + std::fabs(g[5]);
        l[0] = -w; h[0] = w; l[1] = -hh; h[1] = hh; l[2] = -m; h[2] = m; break;
    }
    case TRC_GM_ELLIPSOID: case TRC_GM_ELLIPSOID_CUT:
        for (int i = 0; i < 3; ++i) { double r = 1.0 / std::sqrt(g[i]); l[i] = -r; h[i] = r; }
        if (s.gm_kind == TRC_GM_ELLIPSOID_CUT)
            for (int i = 0; i < 3; ++i) { l[i] = std::fmax(l[i], g[3 + 2 * i]); h[i] = std::fmin(h[i], g[4 + 2 * i]); }
        break;
    default:
        return false;   // FLAT_INF, PARABOLOID, PARAB_RECT_OFFAXIS, PARAB_CYL, CYL_INF, CONE_INF, QUADRATIC
    }
    for (int i = 0; i < 3; ++i) if (!(l[i] <= h[i]) || !std::isfinite(l[i]) || !std::isfinite(h[i])) return false;
    return true;
}

// corner c (0..7) of a surface's local box in global coordinates
static inline void trc_surface_box_corner(const trc_surface_desc &s, const double l[3], const double h[3], bool global_axes, int c,
                                          double q[3]) {
    const double p[3] = {(c & 1) ? h[0] : l[0], (c & 2) ? h[1] : l[1], (c & 4) ? h[2] : l[2]};
    for (int i = 0; i < 3; ++i)
        q[i] = global_axes ? p[i] + s.frame[4 * i + 3]
                           : s.frame[4 * i] * p[0] + s.frame[4 * i + 1] * p[1] + s.frame[4 * i + 2] * p[2] + s.frame[4 * i + 3];
}

// Box of a surface in global coordinates.  Returns false for unbounded kinds.
static inline bool trc_surface_bounds(const trc_surface_desc &s, double lo[3], double hi[3]) {
    double l[3], h[3];
    bool global_axes;
    if (!trc_surface_local_box(s, l, h, &global_axes)) return false;
    for (int i = 0; i < 3; ++i) { lo[i] = std::numeric_limits<double>::infinity(); hi[i] = -lo[i]; }
    for (int c = 0; c < 8; ++c) {
        double q[3];
        trc_surface_box_corner(s, l, h, global_axes, c, q);
        for (int i = 0; i < 3; ++i) { lo[i] = std::fmin(lo[i], q[i]); hi[i] = std::fmax(hi[i], q[i]); }
    }
    return true;
}

static inline float trc_f32_down(double x) { float f = (float)x; return ((double)f > x) ? std::nextafterf(f, -INFINITY) : f; }
static inline float trc_f32_up(double x) { float f = (float)x; return ((double)f < x) ? std::nextafterf(f, INFINITY) : f; }

// Oriented box of a surface for the single-precision candidate test (trc_obb_hit32, trc_core.h): the surface's own box in
// its own frame, inflated by delta, with the rotation global -> local and the frame origin relative to the scene centre.
// For a flat surface the box is the plate itself +- delta: a ray that passes this test nearly always passes the exact one.
#define TRC_BG_ENT 12      /* floats per entry of the large grid's lists */
#define TRC_OBB_STRIDE 20   /* [A0 A1 A2 c0 | A3 A4 A5 c1 | A6 A7 A8 c2 | lo0 lo1 lo2 hi0 | hi1 hi2 - -]; A = R^T */
#ifndef TRC_OBB_LSTRIDE
#define TRC_OBB_LSTRIDE 20      /* floats between the oriented boxes of two surfaces in their LDS copies.  At 20, the stride of the global
                                   table, eight lanes on different surfaces share a bank group and the counters show bank conflicts worth
                                   a quarter of k_s_fresh's time -- but 21 (every lane its own bank, 32-bit reads instead of 128-bit ones)
                                   measured the same on all three configurations: the conflicts hide behind the arithmetic */
#endif

// The LDS image of the tables a search kernel of the streaming engine reads (k_s_fresh, k_s_fresh2, k_s_bounce, k_s_bounce_coop):
// ONE description, read by the kernels, which carve their pointers from it (stage_search_tables, trc_device.h), and by the host,
// which sizes the launches from it and decides whether a scene's tables fit LDS (trc_stream_form_fresh, trc_stream_form_bounce).  The
// parts follow one another in the order of the fields below; a part that is absent takes no room.
#define SFQ_CAP 128             /* entries of a wave's queue between the two phases of k_s_fresh2 (a power of two, >= 2 x 64) */
#ifndef SBC_CELLS
#define SBC_CELLS 4             /* cells with faces a lane of k_s_bounce_coop collects per stage */
#endif
#define SBC_PAIRS 256           /* (ray, surface) pairs that can wait for their exact test, per wave of k_s_bounce_coop */
#define SBC_WAVE_BYTES (2 * SBC_CELLS * 64 * 4 + 64 * 4 + SBC_PAIRS * 4 + 64 * 8 + 64 * 4)
#define TRC_LDS_SLACK 16        /* bytes the fits-in-LDS decisions allow on top of what each of the oriented boxes, the footprint lists
                                   and the queues takes (half of it for the small grid, and 4 more when its cell count is odd): the
                                   margins of the hand-made sums this description replaced, kept so that no scene changes sides of a
                                   limit */
struct trc_lds_parts {
    int n_surf, stride;         // surfaces, doubles per surface record
    int buie_bytes;             // the Buie table (sizeof(trc_buie_fast)), 0: none
    int occ_words;              // occupancy words of the large grid, 0: none
    bool tables;                // surface records and oriented boxes (TRC_OBB_LSTRIDE floats apart)
    bool sbox, flags;           // per surface: axis-aligned box (6 floats), flags (one word)
    int fp_offs, fp_list;       // footprint map: cell offsets (0: none) and list entries, 16 bits each
    int grid_cells, grid_list;  // small grid: cells (0: none; one offset more) and list entries, 16 bits each
    int queue_waves;            // k_s_fresh2: waves with a queue of SFQ_CAP (ray, cell) pairs each
    int coop_waves;             // k_s_bounce_coop: waves with a block of SBC_WAVE_BYTES each
};
struct trc_lds_layout {
    size_t buie, occ, recs, obb, sbox, flags, fp_off, fp_list, grid_off, grid_list, queues, coop;      // byte offset of every part
    size_t end;                 // bytes in all
    size_t slack;               // what a fits-in-LDS decision adds to `end` (TRC_LDS_SLACK)
};
TRC_HD size_t trc_lds_round16(size_t b) { return (b + 15) & ~(size_t)15; }
TRC_HD trc_lds_layout trc_search_lds_layout(const trc_lds_parts &p) {
    trc_lds_layout L;
    const size_t S = (size_t)p.n_surf;
    size_t cur = 0, slack = 0;
    L.buie = cur; cur += trc_lds_round16((size_t)p.buie_bytes);
    L.occ = cur; cur += trc_lds_round16((size_t)p.occ_words * 4);
    L.recs = cur; if (p.tables) cur += S * (size_t)p.stride * 8;
    L.obb = cur; if (p.tables) { cur += trc_lds_round16(S * TRC_OBB_LSTRIDE * 4); slack += TRC_LDS_SLACK; }
    L.sbox = cur; if (p.sbox) cur += S * 6 * 4;
    L.flags = cur; if (p.flags) cur += trc_lds_round16(S * 4);
    L.fp_off = cur; if (p.fp_offs) cur += trc_lds_round16((size_t)p.fp_offs * 2);
    L.fp_list = cur; if (p.fp_offs) { cur += (size_t)p.fp_list * 2; slack += TRC_LDS_SLACK; }
    L.grid_off = cur; if (p.grid_cells) cur += (((size_t)p.grid_cells + 2) & ~(size_t)1) * 2;
    L.grid_list = cur; if (p.grid_cells) { cur += (size_t)p.grid_list * 2; slack += TRC_LDS_SLACK / 2 + ((p.grid_cells & 1) ? 4 : 0); }      // (odd: the old sum's rounding)
    if (p.queue_waves) { cur = trc_lds_round16(cur); slack += TRC_LDS_SLACK; }
    L.queues = cur; cur += (size_t)p.queue_waves * (2 * SFQ_CAP * 4);
    L.coop = cur; cur += (size_t)p.coop_waves * SBC_WAVE_BYTES;
    L.end = cur; L.slack = slack;
    return L;
}

// The LDS image of a kernel of the streaming engine that finishes hits, as the HOST sees it: it sizes the launches and decides "fits in
// LDS" from this description alone (trc_stream_form_shade, trc_stream_form_absorb, through trc_shade_lds_choose), and
// tests/test_shade_cases_host.py holds it to the hand-made sums it replaced.  The kernels do NOT read it: each carves its image in its
// own text (each says why at its carving), and that text is kept in agreement with the order, sizes and rounding written here BY HAND
// -- whoever changes a carving changes trc_shade_lds_layout with it; the device tests of the maps and of the shading instances are
// what notices a kernel that carves more than this sums.  The parts follow one another in the order of the layout's fields; a part
// that is absent takes no room.
enum trc_shade_img {
    TRC_IMG_SHADE,              // k_s_shade: every part
    TRC_IMG_SHADE_X,            // k_s_shade_x: every part
    TRC_IMG_LEAN,               // k_s_shade_c<DIFFUSE>: every part
    TRC_IMG_LEAN_MIRROR,        // k_s_shade_c<MIRROR>: no optics tables (no mirror reads one)
    TRC_IMG_ABSORB,             // k_s_absorb: no records, optics parameters or optics tables
    TRC_IMG_INLINE              // k_s_bounce where it finishes the terminal hits itself: k_s_absorb's, behind its search image
};
#define TRC_LDS_SHADE_SLACK 16      /* bytes a decision allows beside the flux-map tables, and again beside the bins ... */
#define TRC_LDS_INLINE_SLACK 64     /* ... and for an image that starts behind another one: the margins of the hand-made sums this
                                       description replaced, kept so that no scene changes sides of a limit (as TRC_LDS_SLACK) */
struct trc_shade_parts {
    int n_surf, stride;         // surfaces, doubles per surface record
    int n_fm_edges, fms_bytes;  // flux maps: edges of all maps (doubles), bytes of the descriptors (n_fm * sizeof(FluxMapDev))
    int n_extra, fm_bins;       // doubles of the optics tables; bins of all flux maps
    int counts;                 // words behind the per-surface sums: the workgroup's hits and rays that go on
    bool tally;                 // the three sums per surface
    bool recs;                  // surface records and optics parameters (8 doubles per surface)
    bool maps;                  // flux-map edges, descriptors, surface -> map
    bool flags;                 // the surface flags behind surface -> map, the two rounded to 8 bytes together.  Without them
                                // surface -> map is rounded on its own
    bool extra;                 // the optics tables
    bool bins;                  // a private copy of the flux-map bins (fm_bins may be 0: the part is there, and its margin)
};
struct trc_shade_layout {
    size_t tally, recs, opt, fm_edges, fms, fm_of, flags, extra, bins;     // byte offset of every part
    size_t end;                 // bytes in all
    size_t slack;               // what a fits-in-LDS decision and a launch add to `end`
};
// The parts of a kernel's image.  lds: the scene's tables are staged (all of them or none: every access then has a known address
// space, see k_s_shade); fm_bins: the flux-map bins privatised in LDS, 0: none.  Without tables the two count words remain -- the lean
// kernels and k_s_shade_x add their counts through them; k_s_shade adds them per wave then and keeps one word that nobody reads.
// k_s_absorb and k_s_bounce run with their tables in LDS only, and always have a bins part (empty when the scene has no map).
TRC_HD trc_shade_parts trc_shade_lds_parts(int img, bool lds, int n_surf, int stride, int n_fm_edges, int fms_bytes, int n_extra, int fm_bins) {
    trc_shade_parts p = {};
    const bool terminal = img == TRC_IMG_ABSORB || img == TRC_IMG_INLINE;
    p.n_surf = n_surf; p.stride = stride; p.n_fm_edges = n_fm_edges; p.fms_bytes = fms_bytes; p.n_extra = n_extra; p.fm_bins = fm_bins;
    p.counts = (img == TRC_IMG_SHADE && !lds) ? 1 : 2;
    p.tally = p.maps = lds;
    p.recs = lds && !terminal;
    p.flags = lds && img != TRC_IMG_INLINE;     // (k_s_bounce reads the flags of its search image)
    p.extra = lds && !terminal && img != TRC_IMG_LEAN_MIRROR;
    p.bins = terminal || fm_bins > 0;
    return p;
}
TRC_HD trc_shade_layout trc_shade_lds_layout(const trc_shade_parts &p) {
    trc_shade_layout L;
    const size_t S = (size_t)p.n_surf;
    size_t cur = 0, slack = 0;
    L.tally = cur; cur += ((p.tally ? 3 * S : 0) + (size_t)p.counts) * 8;
    L.recs = cur; if (p.recs) cur += S * (size_t)p.stride * 8;
    L.opt = cur; if (p.recs) cur += S * 8 * 8;
    L.fm_edges = cur; if (p.maps) cur += (size_t)p.n_fm_edges * 8;
    L.fms = cur; if (p.maps) cur += (((size_t)p.fms_bytes + 7) / 8) * 8;
    L.fm_of = cur; if (p.maps) cur += S * 4;
    L.flags = cur; if (p.maps && p.flags) cur += S * 4;
    if (p.maps) {
        const size_t r = (cur + 7) & ~(size_t)7;
        // flags read from elsewhere take no room here, but the old sum counted them all the same: what of their S * 4 bytes the
        // rounding of surface -> map does not use up stays in the sum as a margin, beside the one for the start behind another image
        const size_t borrowed = p.flags ? 0 : cur + S * 4 - r;
        slack += TRC_LDS_SHADE_SLACK + (p.flags ? 0 : TRC_LDS_INLINE_SLACK) + borrowed;
        cur = r;
    }
    L.extra = cur; if (p.extra) cur += (size_t)p.n_extra * 8;
    L.bins = cur; if (p.bins) { cur += (size_t)p.fm_bins * 8; slack += TRC_LDS_SHADE_SLACK; }
    L.end = cur; L.slack = slack;
    return L;
}
// the bytes up to which an image's tables go to LDS, and (bins) up to which the flux-map bins go with them
TRC_HD size_t trc_shade_lds_limit(int img, bool bins) {
    switch (img) {
    case TRC_IMG_SHADE: case TRC_IMG_SHADE_X: return (size_t)(bins ? 78 : 72) * 1024;       // two workgroups per CU
    case TRC_IMG_LEAN: case TRC_IMG_LEAN_MIRROR: return (size_t)(bins ? 150 : 120) * 1024;  // one workgroup of sixteen waves per CU
    case TRC_IMG_ABSORB: return (size_t)78 * 1024;
    default: return (size_t)158 * 1024;          // TRC_IMG_INLINE: with the search image in front
    }
}
// Tables and bins of a shading kernel (not TRC_IMG_ABSORB / TRC_IMG_INLINE, which follow k_s_shade's choice): the tables go to LDS when
// the image fits the kernel's limit, all `bins` flux-map bins with them when the image still fits the limit set for that (bins are
// never in LDS without the tables).  Returns the dynamic LDS of the launch: end + slack of the image chosen.
TRC_HD size_t trc_shade_lds_choose(int img, int n_surf, int stride, int n_fm_edges, int fms_bytes, int n_extra, long long bins, bool *in_lds,
                                   int *lds_fm_bins) {
    trc_shade_layout L = trc_shade_lds_layout(trc_shade_lds_parts(img, true, n_surf, stride, n_fm_edges, fms_bytes, n_extra, 0));
    *in_lds = L.end + L.slack <= trc_shade_lds_limit(img, false);
    L = trc_shade_lds_layout(trc_shade_lds_parts(img, true, n_surf, stride, n_fm_edges, fms_bytes, n_extra, (int)bins));
    *lds_fm_bins = (bins > 0 && *in_lds && L.end + L.slack <= trc_shade_lds_limit(img, true)) ? (int)bins : 0;
    L = trc_shade_lds_layout(trc_shade_lds_parts(img, *in_lds, n_surf, stride, n_fm_edges, fms_bytes, n_extra, *lds_fm_bins));
    return L.end + L.slack;
}

struct trc_accel_host {
    std::vector<float> sbox;          // 6 per surface
    std::vector<float> obb;           // TRC_OBB_STRIDE per surface (unbounded: a box nothing misses)
    std::vector<int32_t> unbounded;
    std::vector<uint32_t> nodes;      // 2 per Kd node
    std::vector<uint16_t> leaf_surfs;
    std::vector<uint16_t> brute_leaf;  // all bounded surfaces: the single leaf used when no Kd-tree is given
    uint32_t brute_nodes[2];
    float brute_root[6];
    float root[6];
    float delta;
    double cen[3], slo[3], shi[3];
    bool any_bounded;
    int kd_depth;
    // uniform grid over the scene box (trc_accel_build_grid)
    bool grid_ok;
    int32_t grid_dim[3];
    float grid_lo[3], grid_cs[3], grid_inv[3];
    std::vector<uint16_t> grid_off;    // cells + 1
    std::vector<uint16_t> grid_list;
    std::vector<int32_t> grid_apart;   // bounded surfaces kept out of the grid: their boxes are tested for every ray
    float grid_root[6];                // box of the surfaces in the grid, relative, rounded outwards
    // clear cones of the surfaces listed in that grid (trc_clear_build): per surface clear_T x clear_T tiles of four floats, the
    // unit axis and tan^2 of the half-angle (0: no cone); clear_cones: tiles that have one (0: the table is not uploaded)
    std::vector<float> clear;
    int32_t clear_T = 0, clear_cones = 0;
    // the same kind of grid without the limits of LDS, for scenes the one above cannot hold (trc_accel_build_grid32):
    // 32-bit offsets and lists in global memory; big_apart: the few surfaces kept out of it (as grid_apart)
    bool big_ok;
    std::vector<int32_t> big_apart;
    int32_t big_dim[3];
    float big_lo[3], big_cs[3], big_inv[3], big_root[6];
    std::vector<uint32_t> big_off, big_list;
    // what the walk reads per listed surface, in the order of big_list (TRC_BG_ENT floats each, see trc_tri_hit32 in trc_core.h):
    // a triangle with its corner and two edges, any other kind with its box -- the list entry, the box and the oriented box of a
    // candidate are three loads one behind the other otherwise; and one bit per cell that lists anything
    std::vector<float> big_ent;
    std::vector<uint32_t> big_occ;
};

// surfaces -> boxes, scene box, centre, delta
static inline void trc_accel_build_surfaces(const trc_surface_desc *surfs, int n, trc_accel_host &A) {
    const double INF = std::numeric_limits<double>::infinity();
    std::vector<double> lo(3 * (size_t)n), hi(3 * (size_t)n);
    std::vector<char> bounded(n);
    double slo[3] = {INF, INF, INF}, shi[3] = {-INF, -INF, -INF};
    A.unbounded.clear();
    A.any_bounded = false;
    for (int i = 0; i < n; ++i) {
        bounded[i] = trc_surface_bounds(surfs[i], &lo[3 * (size_t)i], &hi[3 * (size_t)i]);
        if (bounded[i]) {
            A.any_bounded = true;
            for (int k = 0; k < 3; ++k) { slo[k] = std::fmin(slo[k], lo[3 * (size_t)i + k]); shi[k] = std::fmax(shi[k], hi[3 * (size_t)i + k]); }
        } else A.unbounded.push_back(i);
    }
    if (!A.any_bounded) for (int k = 0; k < 3; ++k) { slo[k] = 0.0; shi[k] = 0.0; }
    double ext = 0.0;
    for (int k = 0; k < 3; ++k) { A.cen[k] = 0.5 * (slo[k] + shi[k]); ext = std::fmax(ext, shi[k] - slo[k]); }
    // float32 spacing at the largest relative coordinate is ~ext * 6e-8: delta is >= 400 such steps
    double delta = std::fmax(1e-3, 2.5e-5 * ext);
    A.delta = (float)delta;
    for (int k = 0; k < 3; ++k) { A.slo[k] = slo[k] - 2.0 * delta; A.shi[k] = shi[k] + 2.0 * delta; }
    A.brute_leaf.clear();
    for (int i = 0; i < n && i < 65536; ++i) if (bounded[i]) A.brute_leaf.push_back((uint16_t)i);
    A.brute_nodes[0] = 0u;
    A.brute_nodes[1] = ((uint32_t)A.brute_leaf.size() << 2) | 3u;
    for (int k = 0; k < 3; ++k) {
        A.brute_root[k] = trc_f32_down(A.slo[k] - A.cen[k]);
        A.brute_root[3 + k] = trc_f32_up(A.shi[k] - A.cen[k]);
    }
    A.grid_ok = false;
    A.big_ok = false;
    A.big_off.clear(); A.big_list.clear();
    A.sbox.assign(6 * (size_t)n, 0.0f);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            if (bounded[i]) {
                A.sbox[6 * (size_t)i + k] = trc_f32_down(lo[3 * (size_t)i + k] - A.cen[k] - delta);
                A.sbox[6 * (size_t)i + 3 + k] = trc_f32_up(hi[3 * (size_t)i + k] - A.cen[k] + delta);
            } else {
                A.sbox[6 * (size_t)i + k] = -INFINITY;
                A.sbox[6 * (size_t)i + 3 + k] = INFINITY;
            }
        }
    A.obb.assign((size_t)TRC_OBB_STRIDE * (size_t)n, 0.0f);
    for (int i = 0; i < n; ++i) {
        float *B = &A.obb[(size_t)TRC_OBB_STRIDE * (size_t)i];
        double l[3], h[3];
        bool global_axes = false;
        const bool ok = bounded[i] && trc_surface_local_box(surfs[i], l, h, &global_axes);
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k)         // row r of A = column r of the frame's rotation (local axis r in global coordinates)
                B[4 * r + k] = (ok && !global_axes) ? (float)surfs[i].frame[4 * k + r] : (r == k ? 1.0f : 0.0f);
            B[4 * r + 3] = ok ? (float)(surfs[i].frame[4 * r + 3] - A.cen[r]) : 0.0f;
        }
        for (int k = 0; k < 3; ++k) {
            // the rotation is rounded to float32 (6e-8 relative): over a box of half-size |l|, |h| that moves a point by at most
            // ~2e-7 * size, far inside delta
            const float blo = ok ? trc_f32_down(l[k] - delta) : -INFINITY, bhi = ok ? trc_f32_up(h[k] + delta) : INFINITY;
            B[12 + k] = blo;
            B[15 + k] = bhi;
        }
    }
}

// Uniform grid over the scene box for the DDA of trc_core.h (call after trc_accel_build_surfaces).  About two cells per
// bounded surface, cubic cells, at most 8192 cells and 65535 list entries (uint16 offsets, everything stays in LDS);
// the resolution is halved until that holds.  A surface is listed in every cell its box, inflated by 2*delta on top of
// the delta already in sbox, overlaps.
static inline void trc_accel_build_grid(trc_accel_host &A, int n_surf) {
    A.grid_ok = false;
    A.grid_off.clear();
    A.grid_list.clear();
    A.grid_apart.clear();
    if (A.brute_leaf.empty() || n_surf > 65535) return;
    // Surfaces that stand far from the rest (the receiver on its tower above a heliostat field) would stretch the grid over
    // mostly empty space that every ray then has to step through.  Up to 8 of them (and at most a quarter of the scene) are
    // set apart while leaving one out shrinks the box of the others by more than 30 %: their boxes are tested for every ray.
    std::vector<uint16_t> members(A.brute_leaf);
    auto box_of = [&](const std::vector<uint16_t> &m, int skip, double *blo, double *bhi) {
        for (int k = 0; k < 3; ++k) { blo[k] = INFINITY; bhi[k] = -INFINITY; }
        for (size_t j = 0; j < m.size(); ++j) {
            if ((int)j == skip) continue;
            const float *b = &A.sbox[6 * (size_t)m[j]];
            for (int k = 0; k < 3; ++k) { blo[k] = std::fmin(blo[k], (double)b[k]); bhi[k] = std::fmax(bhi[k], (double)b[3 + k]); }
        }
    };
    auto volume = [](const double *blo, const double *bhi) {
        double e[3], emax = 0.0;
        for (int k = 0; k < 3; ++k) { e[k] = bhi[k] - blo[k]; emax = std::fmax(emax, e[k]); }
        double v = 1.0;
        for (int k = 0; k < 3; ++k) v *= std::fmax(e[k], 1e-3 * emax);     // flat axes do not make the volume vanish
        return v;
    };
    // (the search is quadratic in the number of surfaces: scenes beyond a few thousand keep everything in the grid)
    while (A.grid_apart.size() < 8 && members.size() > 4 && members.size() <= 4096 && A.grid_apart.size() * 4 < A.brute_leaf.size()) {
        double blo[3], bhi[3];
        box_of(members, -1, blo, bhi);
        const double v_all = volume(blo, bhi);
        int best = -1;
        double v_best = v_all;
        for (size_t j = 0; j < members.size(); ++j) {
            const float *b = &A.sbox[6 * (size_t)members[j]];
            bool on_face = false;              // only a surface that touches a face of the box can shrink it
            for (int k = 0; k < 3; ++k) on_face = on_face || (double)b[k] <= blo[k] || (double)b[3 + k] >= bhi[k];
            if (!on_face) continue;
            double l2[3], h2[3];
            box_of(members, (int)j, l2, h2);
            const double v = volume(l2, h2);
            if (v < v_best) { v_best = v; best = (int)j; }
        }
        if (best < 0 || !(v_best < 0.7 * v_all)) break;
        A.grid_apart.push_back((int32_t)members[(size_t)best]);
        members.erase(members.begin() + best);
    }
    const size_t nb = members.size();
    double lo[3], hi[3], ext[3];
    box_of(members, -1, lo, hi);
    for (int k = 0; k < 3; ++k) {
        A.grid_root[k] = trc_f32_down(lo[k] - 2.0 * (double)A.delta);
        A.grid_root[3 + k] = trc_f32_up(hi[k] + 2.0 * (double)A.delta);
        lo[k] = (double)A.grid_root[k];
        ext[k] = (double)A.grid_root[3 + k] - lo[k];
    }
#ifndef TRC_GRID_DENSITY
#define TRC_GRID_DENSITY 2.0
#endif
    double target = std::fmin(8192.0, std::fmax(8.0, TRC_GRID_DENSITY * (double)nb));
    for (int attempt = 0; attempt < 12; ++attempt, target *= 0.5) {
        // cubic cells of volume V/target over the axes that have an extent; flat axes get one cell
        double emax = std::fmax(ext[0], std::fmax(ext[1], ext[2]));
        if (!(emax > 0.0)) return;
        double vol = 1.0;
        int nax = 0;
        for (int k = 0; k < 3; ++k) if (ext[k] > 1e-3 * emax) { vol *= ext[k]; ++nax; }
        double cell = std::pow(vol / target, 1.0 / (double)(nax > 0 ? nax : 1));
        int dim[3];
        size_t cells = 1;
        for (int k = 0; k < 3; ++k) {
            int n = (ext[k] > 1e-3 * emax) ? (int)std::ceil(ext[k] / cell) : 1;
            dim[k] = n < 1 ? 1 : (n > 128 ? 128 : n);
            cells *= (size_t)dim[k];
        }
        if (cells > 8192) continue;
        float cs[3], inv[3];
        for (int k = 0; k < 3; ++k) {
            double c = ext[k] / dim[k];
            if (!(c > 0.0)) c = 1.0;
            cs[k] = (float)c;
            inv[k] = (float)(1.0 / c);
        }
        const double pad = 2.0 * (double)A.delta;
        std::vector<uint32_t> count(cells + 1, 0u);
        std::vector<int> range(6 * nb);
        size_t total = 0;
        for (size_t j = 0; j < nb; ++j) {
            const float *b = &A.sbox[6 * (size_t)members[j]];
            size_t c = 1;
            for (int k = 0; k < 3; ++k) {
                int a = (int)std::floor(((double)b[k] - pad - lo[k]) / (double)cs[k]);
                int z = (int)std::floor(((double)b[3 + k] + pad - lo[k]) / (double)cs[k]);
                a = a < 0 ? 0 : (a >= dim[k] ? dim[k] - 1 : a);
                z = z < 0 ? 0 : (z >= dim[k] ? dim[k] - 1 : z);
                range[6 * j + k] = a; range[6 * j + 3 + k] = z;
                c *= (size_t)(z - a + 1);
            }
            total += c;
        }
        if (total > 65535) continue;
        for (size_t j = 0; j < nb; ++j)
            for (int z = range[6 * j + 2]; z <= range[6 * j + 5]; ++z)
                for (int y = range[6 * j + 1]; y <= range[6 * j + 4]; ++y)
                    for (int x = range[6 * j]; x <= range[6 * j + 3]; ++x) count[((size_t)z * dim[1] + y) * dim[0] + x + 1]++;
        for (size_t c = 0; c < cells; ++c) count[c + 1] += count[c];
        A.grid_off.assign(cells + 1, 0);
        for (size_t c = 0; c <= cells; ++c) A.grid_off[c] = (uint16_t)count[c];
        A.grid_list.assign(total > 0 ? total : 1, 0);
        std::vector<uint32_t> cur(count.begin(), count.end() - 1);
        for (size_t j = 0; j < nb; ++j)      // ascending surface index inside every cell
            for (int z = range[6 * j + 2]; z <= range[6 * j + 5]; ++z)
                for (int y = range[6 * j + 1]; y <= range[6 * j + 4]; ++y)
                    for (int x = range[6 * j]; x <= range[6 * j + 3]; ++x)
                        A.grid_list[cur[((size_t)z * dim[1] + y) * dim[0] + x]++] = members[j];
        for (int k = 0; k < 3; ++k) { A.grid_dim[k] = dim[k]; A.grid_lo[k] = (float)lo[k]; A.grid_cs[k] = cs[k]; A.grid_inv[k] = inv[k]; }
        A.grid_ok = true;
        return;
    }
}

// ---------------------------------------------------------------------------------------------
// Clear cones (trc_clear_tile / trc_clear_inside in trc_core.h; call after trc_accel_build_grid).  The rays a heliostat sends on
// were aimed: they leave plate h within a few mrad of the line from h to the receiver, and for most plates nothing stands near
// that line.  Every tile of every plate gets a cone -- the axis a from the plate's centre to the mean centre of the surfaces set
// apart from the grid, and a half-angle -- inside which a ray that starts on the tile can meet the oriented box of no surface
// listed in the grid.  k_s_bounce then leaves the walk out for such a ray; the surfaces set apart and the unbounded ones are
// tested before the walk whatever happens.
//
// The bound, per tile box B (the tile in h's oriented-box frame, as thick as that box, neighbours overlapping by 2 delta on
// every side) and per other listed surface g (its oriented box G as stored in A.obb, whatever its kind):
//   s_max = max_{q in G} a.q - min_{p in B} a.p    (<= 0: g lies behind, ignored)
//   D     = distance of the two boxes' projections onto the plane normal to a (0 when they overlap or touch)
//   tan(alpha_hg) = D / s_max.
// A ray from p in B at angle theta < pi/2 to a has, at axial distance s from p, the perpendicular offset s tan(theta) exactly.
// To reach q it needs |q_perp - p_perp| = s_q tan(theta) with 0 < s_q <= s_max, and |q_perp - p_perp| >= D: theta >= alpha_hg.
// alpha = min over g, capped at TRC_CLEAR_CAP (a wider cone serves nobody, and the cap lets bounding spheres sort out the pairs);
// stored is k = tan^2(alpha (1 - 1e-3) - 1e-4) rounded down -- the margin stands for the single-precision direction and test of
// the kernel and for the tolerance of the box tests a walking ray is given (trc_box_hit32, trc_obb_hit32).
// h qualifies when it is flat with its plate in the plane z = 0 of its frame (a ray that leaves it carries SQ_SKIP_SELF and
// starts on that plane), bounded and listed in the grid, and the scene has a surface set apart.  Everything else gets k = 0.
// ---------------------------------------------------------------------------------------------
#define TRC_CLEAR_CAP 0.2      /* rad */

struct trc_clear_box { double c[8][3]; double cen[3], rad; };

static inline void trc_clear_box_finish(trc_clear_box &b) {
    for (int i = 0; i < 3; ++i) { b.cen[i] = 0.0; for (int c = 0; c < 8; ++c) b.cen[i] += 0.125 * b.c[c][i]; }
    b.rad = 0.0;
    for (int c = 0; c < 8; ++c) {
        double r2 = 0.0;
        for (int i = 0; i < 3; ++i) r2 += (b.c[c][i] - b.cen[i]) * (b.c[c][i] - b.cen[i]);
        b.rad = std::fmax(b.rad, std::sqrt(r2));
    }
}
// the box [l, h] of the oriented-box record B in coordinates relative to the scene centre
static inline void trc_clear_box_of(const float *B, const double l[3], const double h[3], trc_clear_box &b) {
    for (int c = 0; c < 8; ++c) {
        const double p[3] = {(c & 1) ? h[0] : l[0], (c & 2) ? h[1] : l[1], (c & 4) ? h[2] : l[2]};
        for (int i = 0; i < 3; ++i) b.c[c][i] = (double)B[4 * i + 3] + (double)B[i] * p[0] + (double)B[4 + i] * p[1] + (double)B[8 + i] * p[2];
    }
    trc_clear_box_finish(b);
}
// tan(alpha_hg) of the tile box P and the box Q about the unit axis a with the basis (e1, e2) of its normal plane; INFINITY: Q lies
// behind.  The widest gap along a separating edge normal is a lower bound of the distance: where it already gives `bound` or more, it is
// returned in place of the exact value (*exact = false) -- the caller asks for a minimum, and for who stays below the cap.
static inline double trc_clear_tan(const trc_clear_box &P, const trc_clear_box &Q, const double a[3], const double e1[3], const double e2[3],
                                   double bound, bool *exact) {
    double p2[8][2], q2[8][2], pmin = INFINITY, qmax = -INFINITY;
    *exact = true;
    for (int c = 0; c < 8; ++c) {
        pmin = std::fmin(pmin, a[0] * P.c[c][0] + a[1] * P.c[c][1] + a[2] * P.c[c][2]);
        qmax = std::fmax(qmax, a[0] * Q.c[c][0] + a[1] * Q.c[c][1] + a[2] * Q.c[c][2]);
        for (int k = 0; k < 2; ++k) {
            const double *e = k ? e2 : e1;
            p2[c][k] = e[0] * P.c[c][0] + e[1] * P.c[c][1] + e[2] * P.c[c][2];
            q2[c][k] = e[0] * Q.c[c][0] + e[1] * Q.c[c][1] + e[2] * Q.c[c][2];
        }
    }
    const double smax = qmax - pmin;
    if (!(smax > 0.0)) return INFINITY;
    // The projection of a box is the zonotope of its three projected edges: two of them overlap unless one of the six edge normals
    // separates them.
    double gap = 0.0;
    for (int w = 0; w < 2; ++w)
        for (int bit = 1; bit < 8; bit <<= 1) {
            const double (*z)[2] = w ? q2 : p2;
            const double nx = -(z[bit][1] - z[0][1]), ny = z[bit][0] - z[0][0], nn = nx * nx + ny * ny;
            if (!(nn > 0.0)) continue;
            double p0 = INFINITY, p1 = -INFINITY, q0 = INFINITY, q1 = -INFINITY;
            for (int c = 0; c < 8; ++c) {
                const double pp = nx * p2[c][0] + ny * p2[c][1], qq = nx * q2[c][0] + ny * q2[c][1];
                p0 = std::fmin(p0, pp); p1 = std::fmax(p1, pp); q0 = std::fmin(q0, qq); q1 = std::fmax(q1, qq);
            }
            const double g = std::fmax(q0 - p1, p0 - q1);
            if (g > 0.0) gap = std::fmax(gap, g / std::sqrt(nn));
        }
    if (!(gap > 0.0)) return 0.0;
    if (gap * (1.0 - 1e-12) / smax >= bound) { *exact = false; return gap * (1.0 - 1e-12) / smax; }
    // apart: the distance is that of a corner of one to an edge of the other (every edge of a hull is a projected box edge, and the
    // projected edges inside a hull are no nearer than the hull)
    double d2 = INFINITY;
    for (int w = 0; w < 2; ++w) {
        const double (*z)[2] = w ? q2 : p2, (*o)[2] = w ? p2 : q2;       // edges of z, corners of o
        for (int c = 0; c < 8; ++c)
            for (int bit = 1; bit < 8; bit <<= 1) {
                if (c & bit) continue;
                const double ex = z[c | bit][0] - z[c][0], ey = z[c | bit][1] - z[c][1], ee = ex * ex + ey * ey, ie = ee > 0.0 ? 1.0 / ee : 0.0;
                for (int v = 0; v < 8; ++v) {
                    const double wx = o[v][0] - z[c][0], wy = o[v][1] - z[c][1];
                    double t = (wx * ex + wy * ey) * ie;
                    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
                    const double rx = wx - t * ex, ry = wy - t * ey;
                    d2 = std::fmin(d2, rx * rx + ry * ry);
                }
            }
    }
    return std::sqrt(d2) * (1.0 - 1e-12) / smax;
}

// T: tiles per side (the library: TRC_CLEAR_T).  surfs: the surfaces the tables of A were built from.
static inline void trc_clear_build(const trc_surface_desc *surfs, int n_surf, int T, trc_accel_host &A) {
    A.clear.clear();
    A.clear_T = T;
    A.clear_cones = 0;
    if (!A.grid_ok || A.grid_apart.empty() || T < 1) return;
    A.clear.assign((size_t)n_surf * T * T * 4, 0.0f);
    const double delta = (double)A.delta, tcap = std::tan(TRC_CLEAR_CAP);
    // the surfaces listed in the grid, with their oriented boxes
    std::vector<char> listed((size_t)n_surf, 0);
    for (size_t k = 0; k < (size_t)A.grid_off.back() && k < A.grid_list.size(); ++k) listed[A.grid_list[k]] = 1;
    std::vector<int> ids;
    std::vector<trc_clear_box> boxes;
    for (int g = 0; g < n_surf; ++g) {
        if (!listed[g]) continue;
        const float *B = &A.obb[(size_t)TRC_OBB_STRIDE * g];
        const double l[3] = {B[12], B[13], B[14]}, h[3] = {B[15], B[16], B[17]};
        trc_clear_box b;
        trc_clear_box_of(B, l, h, b);
        ids.push_back(g);
        boxes.push_back(b);
    }
    double target[3] = {0.0, 0.0, 0.0};
    for (int32_t s : A.grid_apart) {
        const float *B = &A.obb[(size_t)TRC_OBB_STRIDE * s];
        const double l[3] = {B[12], B[13], B[14]}, h[3] = {B[15], B[16], B[17]};
        trc_clear_box b;
        trc_clear_box_of(B, l, h, b);
        for (int i = 0; i < 3; ++i) target[i] += b.cen[i] / (double)A.grid_apart.size();
    }
    std::vector<int> near, keep;
    std::vector<std::vector<int>> lists, below;
    for (size_t hi = 0; hi < ids.size(); ++hi) {
        const int hs = ids[hi];
        const int kind = surfs[hs].gm_kind;
        const float *B = &A.obb[(size_t)TRC_OBB_STRIDE * hs];
        if (!trc_gm_is_flat(kind) || kind == TRC_GM_TRIANGLE || !(B[14] < 0.0f && B[17] > 0.0f && B[14] == -B[17])) continue;
        const trc_clear_box &H = boxes[hi];
        double a[3] = {target[0] - H.cen[0], target[1] - H.cen[1], target[2] - H.cen[2]};
        const double an = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        if (!(an > 0.0)) continue;
        for (int i = 0; i < 3; ++i) a[i] /= an;
        // what the kernel reads: the axis in single precision, made a unit vector again in double for the bound
        const float af[3] = {(float)a[0], (float)a[1], (float)a[2]};
        const double fn = std::sqrt((double)af[0] * af[0] + (double)af[1] * af[1] + (double)af[2] * af[2]);
        for (int i = 0; i < 3; ++i) a[i] = (double)af[i] / fn;
        const int m = std::fabs(a[0]) < std::fabs(a[1]) ? (std::fabs(a[0]) < std::fabs(a[2]) ? 0 : 2) : (std::fabs(a[1]) < std::fabs(a[2]) ? 1 : 2);
        double e1[3] = {0.0, 0.0, 0.0}, e2[3];
        e1[m] = 1.0;
        const double d1 = a[m];
        double n1 = 0.0;
        for (int i = 0; i < 3; ++i) { e1[i] -= d1 * a[i]; n1 += e1[i] * e1[i]; }
        n1 = std::sqrt(n1);
        for (int i = 0; i < 3; ++i) e1[i] /= n1;
        e2[0] = a[1] * e1[2] - a[2] * e1[1]; e2[1] = a[2] * e1[0] - a[0] * e1[2]; e2[2] = a[0] * e1[1] - a[1] * e1[0];
        // the surfaces whose bounding sphere comes within the widest cone of the whole plate's, the nearest along the axis first (what
        // blocks a tile is found early, and what is found early bounds the rest)
        // (by the spheres: does Q leave the cone of tangent t about P free?  D >= the gap of the spheres, s_max <= s + R)
        auto outside = [&](const trc_clear_box &P, const trc_clear_box &Q, double t) {
            const double v[3] = {Q.cen[0] - P.cen[0], Q.cen[1] - P.cen[1], Q.cen[2] - P.cen[2]};
            const double s = a[0] * v[0] + a[1] * v[1] + a[2] * v[2], R = P.rad + Q.rad;
            if (s + R <= 0.0) return true;
            const double w2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] - s * s, reach = t * (s + R) + R;
            return w2 >= reach * reach;
        };
        near.clear();
        for (size_t gi = 0; gi < ids.size(); ++gi) if (gi != hi && !outside(H, boxes[gi], tcap)) near.push_back((int)gi);
        std::sort(near.begin(), near.end(), [&](int x, int y) {
            const double sx = a[0] * boxes[(size_t)x].cen[0] + a[1] * boxes[(size_t)x].cen[1] + a[2] * boxes[(size_t)x].cen[2];
            const double sy = a[0] * boxes[(size_t)y].cen[0] + a[1] * boxes[(size_t)y].cen[1] + a[2] * boxes[(size_t)y].cen[2];
            return sx < sy || (sx == sy && x < y);
        });
        // From the whole plate down to its T x T tiles, halving: a tile lies inside the tile it came from, so a surface that leaves the
        // widest cone of a tile free leaves it free for the four below -- they inherit the list of those that do not.  (T that is no
        // power of two: the tiles at once.)
        const double lo[2] = {B[12], B[13]}, up[2] = {B[15], B[16]};
        lists.assign(1, near);
        for (int L = (T & (T - 1)) ? T : 1; L <= T; L *= 2) {
            const bool last = L == T;
            if (!last) below.assign((size_t)4 * L * L, std::vector<int>());
            for (int tv = 0; tv < L; ++tv)
                for (int tu = 0; tu < L; ++tu) {
                    const std::vector<int> &list = lists[lists.size() == 1 ? 0 : (size_t)tv * L + tu];
                    const int t2[2] = {tu, tv};
                    double l[3], h[3];
                    for (int k = 0; k < 2; ++k) {
                        const double w = (up[k] - lo[k]) / L;
                        l[k] = std::fmax(lo[k], lo[k] + t2[k] * w - 2.0 * delta);
                        h[k] = std::fmin(up[k], lo[k] + (t2[k] + 1) * w + 2.0 * delta);
                    }
                    l[2] = B[14]; h[2] = B[17];
                    trc_clear_box P;
                    trc_clear_box_of(B, l, h, P);
                    double tmin = tcap;
                    keep.clear();
                    for (size_t j = 0; j < list.size(); ++j) {
                        if (!(tmin > 0.0)) {        // blocked: nothing left to find for this tile; those below look again at the rest
                            if (last) break;
                            keep.push_back(list[j]);
                            continue;
                        }
                        const trc_clear_box &Q = boxes[(size_t)list[j]];
                        if (outside(P, Q, tcap)) continue;
                        if (tmin < tcap && outside(P, Q, tmin)) { keep.push_back(list[j]); continue; }      // (cannot lower the minimum)
                        bool exact;
                        const double t = trc_clear_tan(P, Q, a, e1, e2, tmin, &exact);
                        if (t >= tcap) continue;
                        keep.push_back(list[j]);
                        if (exact) tmin = std::fmin(tmin, t);
                    }
                    if (!last) {
                        for (int c = 0; c < 4; ++c) below[(size_t)(2 * tv + (c >> 1)) * (2 * L) + (2 * tu + (c & 1))] = keep;
                        continue;
                    }
                    const double alpha = std::fmax(std::atan(tmin) * (1.0 - 1e-3) - 1e-4, 0.0), tk = std::tan(alpha);
                    float k = trc_f32_down(tk * tk);
                    if (!(k > 0.0f)) k = 0.0f;
                    float *o = &A.clear[((size_t)hs * T * T + (size_t)tv * T + tu) * 4];
                    o[0] = af[0]; o[1] = af[1]; o[2] = af[2]; o[3] = k;
                    if (k > 0.0f) A.clear_cones += 1;
                }
            if (!last) lists.swap(below);
        }
    }
}

// Does the triangle (v0, v1, v2) touch the axis-aligned box of centre c and half sides h?  Separating axes (the box's three, the
// triangle's normal, the nine cross products of edges and axes); "touch" includes contact, and 1e-12 of the sizes involved is
// allowed on every comparison so that rounding never leaves a cell out.  Used to list a triangular face only in the cells of the
// large grid it really crosses: its box is twice its size in the plane and as thick as the face is steep.
static inline bool trc_tri_box_overlap(const double c[3], const double h[3], const double v0[3], const double v1[3], const double v2[3]) {
    double a[3][3], e[3][3];
    for (int i = 0; i < 3; ++i) { a[0][i] = v0[i] - c[i]; a[1][i] = v1[i] - c[i]; a[2][i] = v2[i] - c[i]; }
    for (int i = 0; i < 3; ++i) { e[0][i] = a[1][i] - a[0][i]; e[1][i] = a[2][i] - a[1][i]; e[2][i] = a[0][i] - a[2][i]; }
    double scale = 0.0;
    for (int k = 0; k < 3; ++k) for (int i = 0; i < 3; ++i) scale = std::fmax(scale, std::fabs(a[k][i]));
    for (int i = 0; i < 3; ++i) scale = std::fmax(scale, h[i]);
    const double tol = 1e-12 * scale;
    for (int i = 0; i < 3; ++i) {       // the box's axes
        const double mn = std::fmin(a[0][i], std::fmin(a[1][i], a[2][i])), mx = std::fmax(a[0][i], std::fmax(a[1][i], a[2][i]));
        if (mn > h[i] + tol || mx < -h[i] - tol) return false;
    }
    {                                   // the triangle's normal
        const double n[3] = {e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0]};
        const double d = n[0] * a[0][0] + n[1] * a[0][1] + n[2] * a[0][2];
        const double rr = h[0] * std::fabs(n[0]) + h[1] * std::fabs(n[1]) + h[2] * std::fabs(n[2]);
        if (std::fabs(d) > rr + tol * (std::fabs(n[0]) + std::fabs(n[1]) + std::fabs(n[2]))) return false;
    }
    for (int k = 0; k < 3; ++k)         // edge k x axis i
        for (int i = 0; i < 3; ++i) {
            const int j1 = (i + 1) % 3, j2 = (i + 2) % 3;
            // axis = unit(i) x e[k] = (.., -e[k][j2] at j1, e[k][j1] at j2)
            const double ax1 = -e[k][j2], ax2 = e[k][j1];
            double mn = INFINITY, mx = -INFINITY;
            for (int q = 0; q < 3; ++q) { const double pr = ax1 * a[q][j1] + ax2 * a[q][j2]; mn = std::fmin(mn, pr); mx = std::fmax(mx, pr); }
            const double rr = h[j1] * std::fabs(ax1) + h[j2] * std::fabs(ax2);
            if (mn > rr + tol * (std::fabs(ax1) + std::fabs(ax2)) || mx < -rr - tol * (std::fabs(ax1) + std::fabs(ax2))) return false;
        }
    return true;
}

// The grid for scenes that do not fit the one above: same construction (cells of about equal sides, three cells per
// surface, a surface listed in every cell its box inflated by 2*delta overlaps), at most 2^24 cells and 2^28 list entries, all
// bounded surfaces but the few set apart (big_apart), 32-bit offsets and lists.  Call after trc_accel_build_surfaces.
static inline void trc_accel_build_grid32(const trc_surface_desc *surfs, int n_surf, trc_accel_host &A) {
    A.big_ok = false;
    A.big_off.clear(); A.big_list.clear(); A.big_apart.clear(); A.big_ent.clear(); A.big_occ.clear();
    std::vector<uint32_t> members;
    for (int i = 0; i < n_surf; ++i) {
        const float *b = &A.sbox[6 * (size_t)i];
        if (!(b[3] == INFINITY && b[0] == -INFINITY)) members.push_back((uint32_t)i);
    }
    // Surfaces that stand far from the rest -- the lid 50 m above a mesh of 1e5 faces -- would stretch the grid over empty space
    // and leave hundreds of faces in every cell of the mesh (the 105 800-triangle relief: 280 -> ms per 2e7 rays).  As in
    // trc_accel_build_grid up to 8 of them are set apart while leaving one out shrinks the box of the others by more than 30 %;
    // here in linear time: only a surface that holds an extreme of the box on some axis can shrink it, and the box without it
    // follows from the two smallest lower and two largest upper bounds per axis.
    while (A.big_apart.size() < 8 && members.size() > 16) {
        double lo1[3], lo2[3], hi1[3], hi2[3];
        long ilo[3], ihi[3];
        for (int k = 0; k < 3; ++k) { lo1[k] = lo2[k] = INFINITY; hi1[k] = hi2[k] = -INFINITY; ilo[k] = ihi[k] = -1; }
        for (size_t j = 0; j < members.size(); ++j) {
            const float *b = &A.sbox[6 * (size_t)members[j]];
            for (int k = 0; k < 3; ++k) {
                const double l = (double)b[k], h = (double)b[3 + k];
                if (l < lo1[k]) { lo2[k] = lo1[k]; lo1[k] = l; ilo[k] = (long)j; } else if (l < lo2[k]) lo2[k] = l;
                if (h > hi1[k]) { hi2[k] = hi1[k]; hi1[k] = h; ihi[k] = (long)j; } else if (h > hi2[k]) hi2[k] = h;
            }
        }
        auto volume = [](const double *blo, const double *bhi) {
            double e[3], emax = 0.0;
            for (int k = 0; k < 3; ++k) { e[k] = bhi[k] - blo[k]; emax = std::fmax(emax, e[k]); }
            double v = 1.0;
            for (int k = 0; k < 3; ++k) v *= std::fmax(e[k], 1e-3 * emax);
            return v;
        };
        const double v_all = volume(lo1, hi1);
        long best = -1;
        double v_best = v_all;
        for (int c = 0; c < 6; ++c) {
            const long j = c < 3 ? ilo[c] : ihi[c - 3];
            if (j < 0) continue;
            double l2[3], h2[3];
            for (int k = 0; k < 3; ++k) { l2[k] = (ilo[k] == j) ? lo2[k] : lo1[k]; h2[k] = (ihi[k] == j) ? hi2[k] : hi1[k]; }
            const double v = volume(l2, h2);
            if (v < v_best) { v_best = v; best = j; }
        }
        if (best < 0 || !(v_best < 0.7 * v_all)) break;
        A.big_apart.push_back((int32_t)members[(size_t)best]);
        members.erase(members.begin() + best);
    }
    const size_t nb = members.size();
    if (nb == 0) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, ext[3];
    for (size_t j = 0; j < nb; ++j) {
        const float *b = &A.sbox[6 * (size_t)members[j]];
        for (int k = 0; k < 3; ++k) { lo[k] = std::fmin(lo[k], (double)b[k]); hi[k] = std::fmax(hi[k], (double)b[3 + k]); }
    }
    for (int k = 0; k < 3; ++k) {
        A.big_root[k] = trc_f32_down(lo[k] - 2.0 * (double)A.delta);
        A.big_root[3 + k] = trc_f32_up(hi[k] + 2.0 * (double)A.delta);
        lo[k] = (double)A.big_root[k];
        ext[k] = (double)A.big_root[3 + k] - lo[k];
    }
    // cells per listed surface: 3 measured best on the relief of 105 800 triangles with k_s_bounce_coop (1: 9.4 ms per 1e7 rays,
    // 2: 9.0, 3: 8.7, 4: 8.9, 6: 9.8, 12: 10.5; with a lane per ray, k_s_bounce<2>, 6: 14.1)
    const double density = 3.0;
    double target = std::fmin(16777216.0, std::fmax(8.0, density * (double)nb));
    for (int attempt = 0; attempt < 16; ++attempt, target *= 0.5) {
        double emax = std::fmax(ext[0], std::fmax(ext[1], ext[2]));
        if (!(emax > 0.0)) return;
        double vol = 1.0;
        int nax = 0;
        for (int k = 0; k < 3; ++k) if (ext[k] > 1e-3 * emax) { vol *= ext[k]; ++nax; }
        double cell = std::pow(vol / target, 1.0 / (double)(nax > 0 ? nax : 1));
        int dim[3];
        size_t cells = 1;
        for (int k = 0; k < 3; ++k) {
            int n = (ext[k] > 1e-3 * emax) ? (int)std::ceil(ext[k] / cell) : 1;
            dim[k] = n < 1 ? 1 : (n > 1024 ? 1024 : n);
            cells *= (size_t)dim[k];
        }
        if (cells > 16777216) continue;
        float cs[3], inv[3];
        for (int k = 0; k < 3; ++k) {
            double c = ext[k] / dim[k];
            if (!(c > 0.0)) c = 1.0;
            cs[k] = (float)c;
            inv[k] = (float)(1.0 / c);
        }
        const double pad = 2.0 * (double)A.delta;
        std::vector<uint32_t> count(cells + 1, 0u);
        std::vector<int> range(6 * nb);
        size_t total = 0;
        for (size_t j = 0; j < nb; ++j) {
            const float *b = &A.sbox[6 * (size_t)members[j]];
            size_t c = 1;
            for (int k = 0; k < 3; ++k) {
                int a = (int)std::floor(((double)b[k] - pad - lo[k]) / (double)cs[k]);
                int z = (int)std::floor(((double)b[3 + k] + pad - lo[k]) / (double)cs[k]);
                a = a < 0 ? 0 : (a >= dim[k] ? dim[k] - 1 : a);
                z = z < 0 ? 0 : (z >= dim[k] ? dim[k] - 1 : z);
                range[6 * j + k] = a; range[6 * j + 3 + k] = z;
                c *= (size_t)(z - a + 1);
            }
            total += c;
        }
        if (total > 268435456) continue;
        // a triangular face is listed in the cells (grown by the pad) it touches, not in all those of its box
        auto listed = [&](size_t j, int x, int y, int z, const double (*tv)[3]) {
            if (!tv) return true;
            const int c3[3] = {x, y, z};
            double cc[3], hh[3];
            for (int k = 0; k < 3; ++k) { cc[k] = lo[k] + ((double)c3[k] + 0.5) * (double)cs[k]; hh[k] = 0.5 * (double)cs[k] + pad + 1e-6 * (double)cs[k]; }
            (void)j;
            return trc_tri_box_overlap(cc, hh, tv[0], tv[1], tv[2]);
        };
        std::vector<double> tri_v;           // 9 per member that is a triangle (corners relative to the scene centre), else unused
        std::vector<char> is_tri(nb, 0);
        tri_v.assign(9 * nb, 0.0);
        for (size_t j = 0; j < nb; ++j) {
            const trc_surface_desc &sd = surfs[members[j]];
            if (sd.gm_kind != TRC_GM_TRIANGLE) continue;
            is_tri[j] = 1;
            double *t = &tri_v[9 * j];
            for (int i = 0; i < 3; ++i) {
                t[i] = sd.frame[4 * i + 3] - A.cen[i];
                for (int q = 0; q < 2; ++q)
                    t[3 + 3 * q + i] = t[i] + sd.frame[4 * i] * sd.gm[3 * q] + sd.frame[4 * i + 1] * sd.gm[3 * q + 1] + sd.frame[4 * i + 2] * sd.gm[3 * q + 2];
            }
        }
        total = 0;
        for (size_t j = 0; j < nb; ++j) {
            const double (*tv)[3] = is_tri[j] ? (const double (*)[3])&tri_v[9 * j] : nullptr;
            for (int z = range[6 * j + 2]; z <= range[6 * j + 5]; ++z)
                for (int y = range[6 * j + 1]; y <= range[6 * j + 4]; ++y)
                    for (int x = range[6 * j]; x <= range[6 * j + 3]; ++x)
                        if (listed(j, x, y, z, tv)) { count[((size_t)z * dim[1] + y) * dim[0] + x + 1]++; ++total; }
        }
        for (size_t c = 0; c < cells; ++c) count[c + 1] += count[c];
        A.big_off.assign(count.begin(), count.end());
        A.big_list.assign(total > 0 ? total : 1, 0u);
        std::vector<uint32_t> cur(count.begin(), count.end() - 1);
        for (size_t j = 0; j < nb; ++j) {    // ascending surface index inside every cell
            const double (*tv)[3] = is_tri[j] ? (const double (*)[3])&tri_v[9 * j] : nullptr;
            for (int z = range[6 * j + 2]; z <= range[6 * j + 5]; ++z)
                for (int y = range[6 * j + 1]; y <= range[6 * j + 4]; ++y)
                    for (int x = range[6 * j]; x <= range[6 * j + 3]; ++x)
                        if (listed(j, x, y, z, tv)) A.big_list[cur[((size_t)z * dim[1] + y) * dim[0] + x]++] = members[j];
        }
        for (int k = 0; k < 3; ++k) { A.big_dim[k] = dim[k]; A.big_lo[k] = (float)lo[k]; A.big_cs[k] = cs[k]; A.big_inv[k] = inv[k]; }
        // the entries of the walk: per member once, then copied in list order
        std::vector<float> ent_of((size_t)TRC_BG_ENT * nb, 0.0f);
        std::vector<uint32_t> member_no((size_t)n_surf, 0u);
        for (size_t j = 0; j < nb; ++j) {
            const uint32_t si = members[j];
            member_no[si] = (uint32_t)j;
            float *e = &ent_of[(size_t)TRC_BG_ENT * j];
            const trc_surface_desc &sd = surfs[si];
            uint32_t w = si;
            if (sd.gm_kind == TRC_GM_TRIANGLE) {
                // corner (the frame's origin) relative to the scene centre, the two edges in global axes; [7] = 1.5 delta max|edge|,
                // [11] = max|edge|^2, both rounded up
                double ed[2][3], emax = 0.0;
                for (int q = 0; q < 2; ++q) {
                    double n2 = 0.0;
                    for (int i = 0; i < 3; ++i) {
                        ed[q][i] = sd.frame[4 * i] * sd.gm[3 * q] + sd.frame[4 * i + 1] * sd.gm[3 * q + 1] + sd.frame[4 * i + 2] * sd.gm[3 * q + 2];
                        n2 += ed[q][i] * ed[q][i];
                    }
                    emax = std::fmax(emax, std::sqrt(n2));
                }
                for (int i = 0; i < 3; ++i) {
                    e[1 + i] = (float)(sd.frame[4 * i + 3] - A.cen[i]);
                    e[4 + i] = (float)ed[0][i];
                    e[8 + i] = (float)ed[1][i];
                }
                e[7] = trc_f32_up(1.5 * (double)A.delta * emax * 1.000001);
                e[11] = trc_f32_up(emax * emax * 1.000001);
            } else {
                w |= 0x80000000u;        // its box here, its oriented box from the table
                const float *b = &A.sbox[6 * (size_t)si];
                for (int i = 0; i < 3; ++i) { e[1 + i] = b[i]; e[4 + i] = b[3 + i]; }
            }
            std::memcpy(&e[0], &w, 4);
        }
        A.big_ent.assign((size_t)TRC_BG_ENT * (total > 0 ? total : 1), 0.0f);
        for (size_t i = 0; i < total; ++i)
            std::memcpy(&A.big_ent[(size_t)TRC_BG_ENT * i], &ent_of[(size_t)TRC_BG_ENT * member_no[A.big_list[i]]], TRC_BG_ENT * sizeof(float));
        A.big_occ.assign((cells + 31) / 32 + 1, 0u);
        for (size_t c = 0; c < cells; ++c) if (A.big_off[c + 1] > A.big_off[c]) A.big_occ[c >> 5] |= 1u << (c & 31);
        A.big_ok = true;
        return;
    }
}

// Kd-tree -> packed nodes relative to the centre (call after trc_accel_build_surfaces). Returns false when the
// tree cannot use the packed form (surface index or node count too large).
static inline bool trc_accel_build_kd(const trc_kdtree_desc *kd, trc_accel_host &A) {
    if (kd->n_nodes >= (1 << 28)) return false;
    A.nodes.assign(2 * (size_t)kd->n_nodes, 0u);
    A.leaf_surfs.assign((size_t)kd->n_leaf_surfs, 0);
    for (int i = 0; i < kd->n_leaf_surfs; ++i) {
        if (kd->leaf_surfs[i] > 65535) return false;
        A.leaf_surfs[i] = (uint16_t)kd->leaf_surfs[i];
    }
    std::vector<int> depth(kd->n_nodes, 0);
    A.kd_depth = 0;
    for (int i = 0; i < kd->n_nodes; ++i) {
        int f = kd->flag[i];
        if (f == 3) {
            A.nodes[2 * (size_t)i] = (uint32_t)kd->leaf_off[i];
            A.nodes[2 * (size_t)i + 1] = ((uint32_t)kd->leaf_cnt[i] << 2) | 3u;
        } else {
            float sp = (float)(kd->split[i] - A.cen[f]);
            uint32_t w;
            std::memcpy(&w, &sp, 4);
            A.nodes[2 * (size_t)i] = w;
            A.nodes[2 * (size_t)i + 1] = ((uint32_t)kd->child[i] << 2) | (uint32_t)f;
            int c = kd->child[i];
            depth[c] = depth[c + 1] = depth[i] + 1;
            if (depth[c] > A.kd_depth) A.kd_depth = depth[c];
        }
    }
    for (int k = 0; k < 3; ++k) {
        A.root[k] = trc_f32_down(kd->bounds[k] - A.cen[k] - A.delta);
        A.root[3 + k] = trc_f32_up(kd->bounds[3 + k] - A.cen[k] + A.delta);
    }
    return true;
}

// ---- the room of a streaming call whose optics split rays (k_s_shade_x<.., SPLIT>) --------------------------------------------
// Such a call never recycles a slot of the ray table: a hit that sends two rays on keeps its slot for the first and takes a new
// one for the second.  What one bounce can ask of a workspace, from what the host knows before it launches the bounce:
//   slots          slots of the ray table handed out so far (bounce 0: what the search stage can hand out, its unused chunk
//                  tails included)
//   live           rays that enter the bounce: at most as many hits, as many new slots and twice as many rays that go on
//   search_tails   entries the appending waves of the search stage can leave unused in a list (waves x chunk, summed over
//                  the kernels that append to one list)
//   shade_waves    waves of the shading kernel; every wave can leave one chunk of slots (slot_chunk entries) and one chunk of the
//                  active list (act_chunk entries) unused
// room: entries of the ray table, of the tables beside it and of every list of the search stage; act_room: of the active lists.
// The sums saturate at 2^64 - 1 instead of wrapping (a need beyond the 32-bit slot numbers is refused by the caller).
typedef unsigned long long trc_u64;
static inline trc_u64 trc_sat_add(trc_u64 a, trc_u64 b) { return a > ~0ull - b ? ~0ull : a + b; }
static inline trc_u64 trc_sat_mul(trc_u64 a, trc_u64 b) { return (a != 0 && b > ~0ull / a) ? ~0ull : a * b; }
struct trc_split_room { trc_u64 room, act_room; };
static inline trc_split_room trc_split_room_need(trc_u64 slots, trc_u64 live, trc_u64 search_tails, trc_u64 shade_waves, trc_u64 slot_chunk,
                                                 trc_u64 act_chunk) {
    trc_split_room r;
    const trc_u64 table = trc_sat_add(trc_sat_add(slots, live), trc_sat_mul(shade_waves, slot_chunk));
    const trc_u64 lists = trc_sat_add(live, search_tails);
    r.room = table > lists ? table : lists;
    r.act_room = trc_sat_add(trc_sat_mul(2ull, live), trc_sat_mul(shade_waves, act_chunk));
    return r;
}
// `slots` for bounce 0, where nothing has been handed out yet: the search stage gives every ray of the batch that hits a slot
// (at most nb) and can leave `search_slot_tails` entries of its waves' chunks unused; the shading kernel of the same bounce then
// takes its slots behind those.
static inline trc_u64 trc_split_slots_bounce0(trc_u64 nb, trc_u64 search_slot_tails) { return trc_sat_add(nb, search_slot_tails); }
// The doubling rule: the size a table of `have` entries grows to for a need of `need` -- `have` itself while it is enough, else
// the first of 2 have, 4 have, ... (from 64 entries) that reaches the need; 2^64 - 1 where doubling would wrap.
static inline trc_u64 trc_split_grow(trc_u64 have, trc_u64 need) {
    if (need <= have) return have;
    trc_u64 r = have < 64ull ? 64ull : have;
    while (r < need) r = r > ~0ull / 2ull ? ~0ull : 2ull * r;
    return r;
}

#endif  // TRC_BOUNDS_H
