// trc_footprint.h -- footprint map of a source: where on the source's plane a fresh ray has to start to be able to
// touch a surface at all.
//
// The sources of sources.py:175-515 start their rays on a disc or a rectangle and aim them into a narrow cone about
// one direction w (pillbox: ang_range; Buie: the solar disc, 4.65 mrad -- the rare rays of the aureole, up to 43.6
// mrad, take the general path).  A ray that starts at o and reaches the point x of a surface at depth s along w has
//     o = x - s (w + tan(theta) u),   |u| = 1, u perpendicular to w, theta <= theta_c,
// i.e. o lies within margin(x) = |h| (a / (|wn| (|wn| - a)) + tan(theta_c) / (|wn| - a)) of the projection of x along w onto
// the source plane, with h = (x - c).n the height of x over the plane, wn = w.n and a = tan(theta_c) sqrt(1 - wn^2)
// (a = 0 for a source that faces its direction: margin = depth * tan(theta_c)).  The footprint of a surface is therefore
// the convex hull of the projections of the eight corners of its box, grown by the largest margin of a corner; a ray
// that starts outside every footprint cannot hit anything and is finished after its Philox block and a float32 position
// -- before its direction is sampled.  Two tables are made from the footprints, in the source's local coordinates
// (lx, ly) over [-half, half]^2:
//   mask   M x M bits: some footprint (+ cell half-diagonal + eps) overlaps the cell          (k_s_fresh stage A, in LDS)
//   lists  (M/4) x (M/4) cells: the surfaces whose footprint overlaps the cell, ascending    (stage B, candidate tests)
//   umask  Mu x Mv bits over the source's two position uniforms: some footprint (+ a radius covering the cell's region) overlaps the
//          region of the start shape that the rays with these top bits of their uniforms start in -- an annular sector of a
//          disc (r = R sqrt(u): cells of equal area), a small rectangle of a rectangle                        (k_s_ucull, in LDS)
// The Cartesian mask wants the ray's float32 start point; the mask over the uniforms wants nothing but the Philox block: the top
// log2 Mu and log2 Mv bits of the two words are its index (trc_fp_ucell), and the step from the bits to the cell is exact, so
// it carries no eps.  Mu Mv is the largest power of two within M M, split Mu : Mv as 1 : 4, 1 : 1 or 4 : 1, whichever sets the
// fewest bits for the scene and source; ucoverage, the share of its bits set, is the share of the source's rays it lists (for
// discs as for rectangles: every cell holds the same share of the rays).  k_s_ucull lists the ray alone; its consumer
// k_s_fresh2 finds the list cell from the float32 start point it makes anyway.  k_s_cull, on the Cartesian mask, hands the cell
// to the consumers that do not (k_s_fresh).
// eps covers the float32 evaluation of the start point in stage A (trc_fp_position32; checked on the device against
// the float64 position by tests/test_gpu_parity.py).  Conservative by construction: a set bit or a listed surface
// only costs time.  tests/test_hostcheck.py checks on the CPU that every ray of the source that hits a surface
// (brute force, float64) has its bit set and that surface listed and passing the oriented-box test; tests/test_umask_host.py the
// same of the mask over the uniforms, with the list cell taken from the float32 start point.
//
// Plain C++ for the host part; the lookups are TRC_HD and shared with the kernels.
#ifndef TRC_FOOTPRINT_H
#define TRC_FOOTPRINT_H

#include "trc_core.h"
#include <cmath>

#define TRC_FP_SHIFT 2            /* a list cell is 4 x 4 mask cells */
#define TRC_FP_EPS_REL 1e-4       /* eps = TRC_FP_EPS_REL * half: float32 start points are good to ~1e-6 * half */

struct trc_fp_params {
    int32_t kind;                 // source kind (trc_source_kind; the Buie kind of the same start shape for a tabulated sunshape)
    int32_t M, Mc;                // mask cells / list cells per side; M = Mc << TRC_FP_SHIFT, a multiple of 32
    int32_t has_generic;          // Buie: rays with u2 >= cdf_end (aureole) take the general path; tabulated sunshape: u2 >= u_c
    float half, inv_cell;         // the map covers [-half, half]^2; inv_cell = M / (2 half)
    float p[6];                   // start-point mapping in float32, per kind (trc_fp_position32)
    double cdf_end;
    double t_adv;                 // every ray may be advanced by this much before its float32 copy is taken: no surface is nearer
};

// float32 start point of a source ray in the source's local coordinates from its Philox block (the float64 one is
// trc_source_ray_t's).  Device: v_sqrt_f32 / v_sin_f32 / v_cos_f32 (1 ulp / ~1e-6 absolute: see TRC_FP_EPS_REL).
// KIND >= 0 promises F.kind == KIND (the kernels compile one instance per source kind).
TRC_HD float trc_fp_sqrt32(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return sqrtf(x);
#endif
}
TRC_HD void trc_fp_sincos_rev32(float rev, float *sn, float *cs) {        // sine and cosine of 2 pi rev
#if defined(__HIP_DEVICE_COMPILE__)
    *sn = __builtin_amdgcn_sinf(rev); *cs = __builtin_amdgcn_cosf(rev);
#else
    *sn = sinf(6.2831853071795865f * rev); *cs = cosf(6.2831853071795865f * rev);
#endif
}
template <int KIND>
TRC_HD void trc_fp_position32_t(const trc_fp_params &F, const uint32_t o[4], float *lx, float *ly) {
    const float s = 1.0f / 4294967296.0f;
    // (the tabulated sunshapes start their rays as the Buie sources: their maps carry the Buie kind, trc_fp_source)
    const int kind = KIND == TRC_SRC_SUNSHAPE_DISK ? TRC_SRC_BUIE_DISK : KIND == TRC_SRC_SUNSHAPE_RECT ? TRC_SRC_BUIE_RECT
                   : KIND >= 0 ? KIND : F.kind;
    float sn, cs;
    if (kind == TRC_SRC_BUIE_DISK) {            // r = R sqrt(u0), phi = 2 pi u1
        const float u0 = ((float)o[0] + 0.5f) * s, u1 = ((float)o[1] + 0.5f) * s;
        const float r = F.p[0] * trc_fp_sqrt32(u0);
        trc_fp_sincos_rev32(u1, &sn, &cs);
        *lx = r * cs; *ly = r * sn;
    } else if (kind == TRC_SRC_BUIE_RECT) {
        const float u0 = ((float)o[0] + 0.5f) * s, u1 = ((float)o[1] + 0.5f) * s;
        *lx = F.p[0] * (u0 - 0.5f); *ly = F.p[1] * (u1 - 0.5f);
    } else if (kind == TRC_SRC_PILLBOX_DISK) {  // r = sqrt(Ri^2 + u2 (Re^2 - Ri^2)), th = span0 + (span1 - span0) u3
        const float u2 = ((float)o[2] + 0.5f) * s, u3 = ((float)o[3] + 0.5f) * s;
        const float r = trc_fp_sqrt32(F.p[0] + u2 * F.p[1]);
        trc_fp_sincos_rev32(F.p[2] + F.p[3] * u3, &sn, &cs);
        *lx = r * cs; *ly = r * sn;
    } else {                                    // TRC_SRC_PILLBOX_RECT: (lx, ly) = (ys, xs), swapped when the source says so
        const float u2 = ((float)o[2] + 0.5f) * s, u3 = ((float)o[3] + 0.5f) * s;
        const float a = F.p[0] * (u2 - 0.5f), b = F.p[1] * (u3 - 0.5f);    // xs, ys
        const bool swap = F.p[2] != 0.0f;
        *lx = swap ? a : b; *ly = swap ? b : a;
    }
}
TRC_HD void trc_fp_position32(const trc_fp_params &F, const uint32_t o[4], float *lx, float *ly) { trc_fp_position32_t<-1>(F, o, lx, ly); }

// mask cell of a start point (clamped: a point that float32 puts just outside the map belongs to its border cell)
TRC_HD void trc_fp_cell(const trc_fp_params &F, float lx, float ly, int32_t *ix, int32_t *iy) {
    int32_t x = (int32_t)floorf((lx + F.half) * F.inv_cell), y = (int32_t)floorf((ly + F.half) * F.inv_cell);
    *ix = x < 0 ? 0 : (x >= F.M ? F.M - 1 : x);
    *iy = y < 0 ? 0 : (y >= F.M ? F.M - 1 : y);
}

// does this ray take the general path (Buie aureole)?  The same comparison as trc_buie_theta_fast makes on the same value.
TRC_HD bool trc_fp_generic(const trc_fp_params &F, const uint32_t o[4]) {
    return F.has_generic && !(((double)o[2] + 0.5) * (1.0 / 4294967296.0) < F.cdf_end);
}

// ---- the mask over the uniforms (umask) ----
// Bit (a, b) of the Mu x Mv mask stands for the rays whose first position uniform has a in its top log2 Mu bits and whose
// second has b in its top log2 Mv bits (o[0], o[1] for the Buie and sunshape kinds, o[2], o[3] for the pillbox kinds).  Bit
// a + Mu b of the mask, words of 32: the word index is b followed by the top log2 Mu - 5 bits of the first uniform, the bit
// its next five -- one alignbit behind a shift, and one bit-field extract.  64 <= Mu, 2 <= Mv (trc_fp_build sees to it).
TRC_HD int trc_fp_first_uniform(int kind) { return (kind == TRC_SRC_PILLBOX_DISK || kind == TRC_SRC_PILLBOX_RECT) ? 2 : 0; }
TRC_HD void trc_fp_ucell(uint32_t ua, uint32_t ub, int lu, int lv, uint32_t *word, uint32_t *bit) {
    const uint32_t b = ub >> (32 - lv);
#if defined(__HIP_DEVICE_COMPILE__)
    *word = __builtin_amdgcn_alignbit(b, ua, (uint32_t)(37 - lu));
#else
    *word = (uint32_t)((((uint64_t)b << 32) | (uint64_t)ua) >> (37 - lu));
#endif
    *bit = (ua >> (32 - lu)) & 31u;
}

// trc_fp_generic as one unsigned compare: ((double)o2 + 0.5) 2^-32 < cdf_end holds exactly when o2 < ceil(cdf_end 2^32 - 0.5)
// (the scaling is exact, and so is the subtraction wherever its result is not below 0).  *on = false: no ray takes the general
// path (no aureole, or a threshold of 2^32 and more); otherwise a ray does when !(o[2] < threshold).
static inline uint32_t trc_fp_generic_threshold(const trc_fp_params &F, bool *on) {
    *on = false;
    if (!F.has_generic) return 0u;
    const double t = std::ceil(F.cdf_end * 4294967296.0 - 0.5);
    if (t >= 4294967296.0) return 0u;
    *on = true;
    return t > 0.0 ? (uint32_t)t : 0u;          // (a cdf_end that is no number compares false with everything: every ray)
}
TRC_HD bool trc_fp_generic_u(bool on, uint32_t threshold, uint32_t o2) { return on && !(o2 < threshold); }

// ---- host side: construction (plain C++, parsed by both passes of hipcc like trc_bounds.h) ----
#include <algorithm>
#include <cmath>
#include <vector>
#include "trc_bounds.h"

struct trc_fp_host {
    bool ok;
    trc_fp_params P;
    std::vector<uint32_t> mask;       // M * M / 32 words, bit (iy * M + ix)
    std::vector<uint32_t> coff;       // Mc * Mc + 1
    std::vector<uint32_t> clist;
    double coverage;                  // fraction of mask cells set
    std::vector<uint32_t> umask;      // Mu * Mv / 32 words, bit (b * Mu + a): the mask over the uniforms (trc_fp_ucell)
    int Mu, Mv;                       // powers of two, Mu >= 64, Mu * Mv <= M * M
    double ucoverage;                 // fraction of umask bits set = the share of the source's rays it lists
    const char *why;                  // when !ok
};

// distance of a point to a convex polygon given counter-clockwise (0 inside); 1 or 2 vertices: point / segment
static inline double trc_fp_dist_poly(const std::vector<double> &px, const std::vector<double> &py, double x, double y) {
    const size_t n = px.size();
    if (n == 0) return INFINITY;
    if (n == 1) return std::hypot(x - px[0], y - py[0]);
    bool inside = n >= 3;
    double best = INFINITY;
    for (size_t i = 0; i < n; ++i) {
        const size_t j = (i + 1) % n;
        if (n == 2 && i == 1) break;
        const double ex = px[j] - px[i], ey = py[j] - py[i], vx = x - px[i], vy = y - py[i];
        if (ex * vy - ey * vx < 0.0) inside = false;
        const double l2 = ex * ex + ey * ey;
        double t = l2 > 0.0 ? (vx * ex + vy * ey) / l2 : 0.0;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        best = std::fmin(best, std::hypot(vx - t * ex, vy - t * ey));
    }
    return inside ? 0.0 : best;
}

// convex hull (Andrew's monotone chain), counter-clockwise, collinear points dropped
static inline void trc_fp_hull(std::vector<std::pair<double, double>> pts, std::vector<double> &hx, std::vector<double> &hy) {
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    const size_t n = pts.size();
    hx.clear(); hy.clear();
    if (n <= 2) { for (auto &p : pts) { hx.push_back(p.first); hy.push_back(p.second); } return; }
    std::vector<std::pair<double, double>> h(2 * n);
    size_t k = 0;
    auto cross = [](const std::pair<double, double> &o, const std::pair<double, double> &a, const std::pair<double, double> &b) {
        return (a.first - o.first) * (b.second - o.second) - (a.second - o.second) * (b.first - o.first);
    };
    for (size_t i = 0; i < n; ++i) { while (k >= 2 && cross(h[k - 2], h[k - 1], pts[i]) <= 0.0) --k; h[k++] = pts[i]; }
    for (size_t i = n - 1, t = k + 1; i > 0; --i) { while (k >= t && cross(h[k - 2], h[k - 1], pts[i - 1]) <= 0.0) --k; h[k++] = pts[i - 1]; }
    h.resize(k > 1 ? k - 1 : k);
    for (auto &p : h) { hx.push_back(p.first); hy.push_back(p.second); }
}

// The source's part of the map: kind, extent of the start shape (half), float32 mapping parameters, the cone's half angle.
// Returns false (reason in *why) for a source the map does not apply to.
static inline bool trc_fp_source(const trc_source_desc &src, trc_fp_params &P, double *half_out, double *theta_c_out, const char **why) {
    memset(&P, 0, sizeof(P));
    const double *p = src.p;
    double half = 0.0, theta_c = 0.0;
    P.kind = src.kind;
    switch (src.kind) {
    case TRC_SRC_BUIE_DISK: {
        const double *sc = src.buie + 3 * (TRC_BUIE_NELEM + 1);
        half = p[0]; theta_c = sc[3];                 // theta_dni: the largest polar angle of the tabulated part
        P.has_generic = 1; P.cdf_end = src.buie[2 * (TRC_BUIE_NELEM + 1) + TRC_BUIE_NELEM];
        P.p[0] = (float)p[0];
        break;
    }
    case TRC_SRC_BUIE_RECT: {
        const double *sc = src.buie + 3 * (TRC_BUIE_NELEM + 1);
        half = 0.5 * std::fmax(std::fabs(p[0]), std::fabs(p[1])); theta_c = sc[3];
        P.has_generic = 1; P.cdf_end = src.buie[2 * (TRC_BUIE_NELEM + 1) + TRC_BUIE_NELEM];
        P.p[0] = (float)p[0]; P.p[1] = (float)p[1];
        break;
    }
    case TRC_SRC_SUNSHAPE_DISK:
    case TRC_SRC_SUNSHAPE_RECT:
        // the core cone theta_c (p[] of a resolved descriptor): a ray with u2 < u_c falls in an interval of the table that ends
        // at or below theta_c, and the sampler clamps to the interval -- its angle is x0 + h, at most one ulp above theta_c.
        // That ulp moves a ray by depth * 2.2e-16 * theta_c, far inside the margin's 1e-9 (half + depth) term (trc_fp_build).
        // The rays of the tail (u2 >= u_c) take the general path.
        if (src.kind == TRC_SRC_SUNSHAPE_DISK) { half = p[0]; P.p[0] = (float)p[0]; P.kind = TRC_SRC_BUIE_DISK; }
        else { half = 0.5 * std::fmax(std::fabs(p[0]), std::fabs(p[1])); P.p[0] = (float)p[0]; P.p[1] = (float)p[1]; P.kind = TRC_SRC_BUIE_RECT; }
        theta_c = p[TRC_SUNSHAPE_P_THETA_C];
        P.has_generic = 1; P.cdf_end = p[TRC_SUNSHAPE_P_U_C];
        break;
    case TRC_SRC_PILLBOX_DISK:
        if (p[5] != 0.0) { *why = "disc source with x_cut (positions are redrawn)"; return false; }
        half = std::fmax(std::fabs(p[0]), std::fabs(p[1])); theta_c = p[4];
        P.p[0] = (float)(p[1] * p[1]); P.p[1] = (float)(p[0] * p[0] - p[1] * p[1]);
        P.p[2] = (float)(p[2] / TRC_TWO_PI); P.p[3] = (float)((p[3] - p[2]) / TRC_TWO_PI);
        break;
    case TRC_SRC_PILLBOX_RECT:
        half = 0.5 * std::fmax(std::fabs(p[0]), std::fabs(p[1])); theta_c = p[2];
        P.p[0] = (float)p[0]; P.p[1] = (float)p[1]; P.p[2] = p[3] != 0.0 ? 1.0f : 0.0f;
        break;
    default:
        *why = "source kind without a plane start shape"; return false;
    }
    if (!(half > 0.0) || !std::isfinite(half) || !(theta_c >= 0.0) || !(theta_c < 0.5)) { *why = "cone too wide (or degenerate source)"; return false; }
    P.half = (float)half;
    *half_out = half; *theta_c_out = theta_c;
    return true;
}

// The region of the start shape that the rays of umask cell (a, b) cover, as a point and a radius that covers the region from
// it.  Discs: the annular sector r0 <= r <= r1, |phi - phi_m| <= dphi / 2 (r = R sqrt(u): cells of equal area; a = 0 reaches
// the centre); from the point (r_m, phi_m) its farthest point is a corner (the distance grows with the angle and is convex
// in r).  Rectangles: a small rectangle, its centre and half diagonal.  src_p: the float64 parameters of the descriptor.
static inline void trc_fp_uregion(int kind, const double *p, int Mu, int Mv, int a, int b, double *cx, double *cy, double *rad) {
    const double ua0 = (double)a / Mu, ua1 = (double)(a + 1) / Mu, ub0 = (double)b / Mv, ub1 = (double)(b + 1) / Mv;
    if (kind == TRC_SRC_BUIE_DISK || kind == TRC_SRC_PILLBOX_DISK) {
        double r0, r1, f0, f1;
        if (kind == TRC_SRC_BUIE_DISK) {
            r0 = p[0] * std::sqrt(ua0); r1 = p[0] * std::sqrt(ua1);
            f0 = TRC_TWO_PI * ub0; f1 = TRC_TWO_PI * ub1;
        } else {
            const double i2 = p[1] * p[1], d2 = p[0] * p[0] - p[1] * p[1];
            r0 = std::sqrt(std::fmax(0.0, i2 + ua0 * d2)); r1 = std::sqrt(std::fmax(0.0, i2 + ua1 * d2));
            f0 = p[2] + (p[3] - p[2]) * ub0; f1 = p[2] + (p[3] - p[2]) * ub1;
        }
        if (r1 < r0) std::swap(r0, r1);
        const double rm = 0.5 * (r0 + r1), fm = 0.5 * (f0 + f1), hw = 0.5 * std::fabs(f1 - f0);
        *cx = rm * std::cos(fm); *cy = rm * std::sin(fm);
        if (hw >= 0.5 * TRC_PI) { *rad = rm + r1; return; }          // (a sector wider than half a turn: the whole disc about the point)
        const double ch = std::cos(hw);
        const double d0 = std::sqrt(std::fmax(0.0, rm * rm + r0 * r0 - 2.0 * rm * r0 * ch)), d1 = std::sqrt(std::fmax(0.0, rm * rm + r1 * r1 - 2.0 * rm * r1 * ch));
        *rad = std::fmax(d0, d1) * (1.0 + 1e-12) + 1e-12 * r1;
    } else {
        double x0, x1, y0, y1;
        if (kind == TRC_SRC_BUIE_RECT) { x0 = p[0] * (ua0 - 0.5); x1 = p[0] * (ua1 - 0.5); y0 = p[1] * (ub0 - 0.5); y1 = p[1] * (ub1 - 0.5); }
        else {      // TRC_SRC_PILLBOX_RECT: xs from the first uniform, ys from the second, swapped when the source says so; (lx, ly) = (ys, xs)
            const double xa = -p[0] / 2.0 + p[0] * ua0, xb = -p[0] / 2.0 + p[0] * ua1, ya = -p[1] / 2.0 + p[1] * ub0, yb = -p[1] / 2.0 + p[1] * ub1;
            if (p[3] != 0.0) { x0 = xa; x1 = xb; y0 = ya; y1 = yb; }
            else { x0 = ya; x1 = yb; y0 = xa; y1 = xb; }
        }
        *cx = 0.5 * (x0 + x1); *cy = 0.5 * (y0 + y1);
        *rad = 0.5 * std::hypot(x1 - x0, y1 - y0) * (1.0 + 1e-12);
    }
}

// one footprint: the hull of a surface's projected box and the margin its rays can start from it (without the float32 eps)
struct trc_fp_print { std::vector<double> hx, hy; double margin; };

// umask of Mu x Mv bits from the footprints: the test of the Cartesian mask on every cell's region.  A bounding circle of the
// footprint bounds the rings (a) and, where it does not hold the centre, the sectors (b) that have to be looked at.
static inline size_t trc_fp_build_umask(int kind, const double *p, const std::vector<trc_fp_print> &prints, int Mu, int Mv, std::vector<uint32_t> &um) {
    um.assign((size_t)Mu * Mv / 32, 0u);
    const bool disc = kind == TRC_SRC_BUIE_DISK || kind == TRC_SRC_PILLBOX_DISK;
    // rings: the squared radius is linear in the first uniform, q(u) = q0 + u dq
    const double q0 = kind == TRC_SRC_PILLBOX_DISK ? p[1] * p[1] : 0.0, dq = kind == TRC_SRC_PILLBOX_DISK ? p[0] * p[0] - p[1] * p[1] : p[0] * p[0];
    for (const trc_fp_print &f : prints) {
        const size_t n = f.hx.size();
        if (n == 0) continue;
        double bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
        for (size_t k = 0; k < n; ++k) { bx0 = std::fmin(bx0, f.hx[k]); bx1 = std::fmax(bx1, f.hx[k]); by0 = std::fmin(by0, f.hy[k]); by1 = std::fmax(by1, f.hy[k]); }
        const double ccx = 0.5 * (bx0 + bx1), ccy = 0.5 * (by0 + by1);
        double cr = 0.0;
        for (size_t k = 0; k < n; ++k) cr = std::fmax(cr, std::hypot(f.hx[k] - ccx, f.hy[k] - ccy));
        cr += f.margin;
        int a0 = 0, a1 = Mu - 1, b0 = 0, nb = Mv;       // sectors b0, b0 + 1, ... (nb of them, wrapping)
        if (disc && dq != 0.0) {
            const double dc = std::hypot(ccx, ccy);
            const double lo = std::fmax(0.0, dc - cr), hi = dc + cr;
            double ul = (lo * lo - q0) / dq, uh = (hi * hi - q0) / dq;
            if (ul > uh) std::swap(ul, uh);
            const double fa0 = std::floor(ul * Mu) - 1.0, fa1 = std::floor(uh * Mu) + 1.0;
            if (fa1 < 0.0 || fa0 > Mu - 1) continue;
            a0 = fa0 < 0.0 ? 0 : (int)fa0; a1 = fa1 > Mu - 1 ? Mu - 1 : (int)fa1;
            const double span = kind == TRC_SRC_PILLBOX_DISK ? p[3] - p[2] : TRC_TWO_PI, f0 = kind == TRC_SRC_PILLBOX_DISK ? p[2] : 0.0;
            if (dc > cr * 1.0001 && std::fabs(span) > 0.0 && std::fabs(span) <= TRC_TWO_PI * (1.0 + 1e-9)) {
                // the circle is seen from the centre under the angles fc +- fw; in units of sectors, from the source's first angle
                const double fc = std::atan2(ccy, ccx), fw = std::asin(cr / dc);
                double t0 = (fc - fw - f0) / span, t1 = (fc + fw - f0) / span;
                if (t0 > t1) std::swap(t0, t1);
                const double turn = TRC_TWO_PI / std::fabs(span);           // the same direction again, in units of the span (>= 1)
                if (std::fabs(turn - 1.0) < 1e-9) {      // a whole disc: sectors wrap
                    const double s0 = std::floor(t0 * Mv) - 1.0, s1 = std::floor(t1 * Mv) + 1.0;
                    if (s1 - s0 + 1.0 < Mv) { nb = (int)(s1 - s0 + 1.0); b0 = (int)(((long long)s0 % Mv + Mv) % Mv); }
                }
                // (a part of a turn: the angles repeat with a period that is no whole number of sectors; every sector is looked at)
            }
        } else if (!disc) {
            // rectangles: which uniform runs along lx
            const bool first_is_x = kind == TRC_SRC_BUIE_RECT || p[3] != 0.0;
            const double wa = p[0], wb = p[1];          // extent along the first / second uniform
            const double alo = first_is_x ? bx0 : by0, ahi = first_is_x ? bx1 : by1, blo = first_is_x ? by0 : bx0, bhi = first_is_x ? by1 : bx1;
            auto range = [&](double lo, double hi, double w, int m, int *i0, int *i1) {
                if (!(std::fabs(w) > 0.0)) { *i0 = 0; *i1 = m - 1; return true; }
                double u0 = (lo - f.margin) / w + 0.5, u1 = (hi + f.margin) / w + 0.5;
                if (u0 > u1) std::swap(u0, u1);
                const double s0 = std::floor(u0 * m) - 1.0, s1 = std::floor(u1 * m) + 1.0;
                if (s1 < 0.0 || s0 > m - 1) return false;
                *i0 = s0 < 0.0 ? 0 : (int)s0; *i1 = s1 > m - 1 ? m - 1 : (int)s1;
                return true;
            };
            int b1;
            if (!range(alo, ahi, wa, Mu, &a0, &a1) || !range(blo, bhi, wb, Mv, &b0, &b1)) continue;
            nb = b1 - b0 + 1;
        }
        for (int kb = 0; kb < nb; ++kb) {
            const int b = (b0 + kb) % Mv;
            for (int a = a0; a <= a1; ++a) {
                const size_t bit = (size_t)b * Mu + a;
                if ((um[bit >> 5] >> (bit & 31)) & 1u) continue;
                double cx, cy, rad;
                trc_fp_uregion(kind, p, Mu, Mv, a, b, &cx, &cy, &rad);
                const double dx = cx - ccx, dy = cy - ccy, reach = cr + rad;
                if (dx * dx + dy * dy > reach * reach) continue;
                if (trc_fp_dist_poly(f.hx, f.hy, cx, cy) <= f.margin + rad) um[bit >> 5] |= 1u << (bit & 31);
            }
        }
    }
    size_t bits = 0;
    for (uint32_t wd : um) bits += (size_t)__builtin_popcount(wd);
    return bits;
}

// A: trc_accel_build_surfaces of the same surfaces.  M: mask cells per side (a multiple of 32 << TRC_FP_SHIFT is not needed,
// a multiple of 32 is).  with_umask: also the mask over the uniforms (umask, Mu, Mv, ucoverage) -- the largest power-of-two
// budget of bits within M * M, in the split (Mu = m / 2, m, 2 m by Mv = 2 m, m, m / 2) that sets the fewest bits for this scene
// and source.  Without it umask stays empty and ucoverage 1.
static inline void trc_fp_build(const trc_surface_desc *surfs, int n_surf, const trc_accel_host &A, const trc_source_desc &src,
                                trc_fp_host &F, int M = 512, bool with_umask = true) {
    F.ok = false;
    F.why = "";
    F.mask.clear(); F.coff.clear(); F.clist.clear();
    F.coverage = 1.0;
    F.umask.clear(); F.Mu = F.Mv = 0; F.ucoverage = 1.0;
    memset(&F.P, 0, sizeof(F.P));
    if (!A.unbounded.empty()) { F.why = "the scene has unbounded surfaces"; return; }
    if (!A.any_bounded) { F.why = "no bounded surface"; return; }
    double half = 0.0, theta_c = 0.0;
    trc_fp_params &P = F.P;
    if (!trc_fp_source(src, P, &half, &theta_c, &F.why)) return;
    const double *rp = src.rot_pos, *rd = src.rot_dir;
    const double e1[3] = {rp[0], rp[3], rp[6]}, e2[3] = {rp[1], rp[4], rp[7]}, w[3] = {rd[2], rd[5], rd[8]};
    auto dot = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    if (std::fabs(dot(e1, e1) - 1.0) > 1e-9 || std::fabs(dot(e2, e2) - 1.0) > 1e-9 || std::fabs(dot(e1, e2)) > 1e-9 ||
        std::fabs(dot(w, w) - 1.0) > 1e-9) { F.why = "start-point axes are not orthonormal"; return; }
    const double nrm[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double wn = dot(w, nrm);
    const double tan_c = std::tan(theta_c);
    const double a = tan_c * std::sqrt(std::fmax(0.0, 1.0 - wn * wn));
    if (!(std::fabs(wn) > 0.1) || !(a < 0.5 * std::fabs(wn))) { F.why = "source direction too oblique to its plane"; return; }
    const double K = a / (std::fabs(wn) * (std::fabs(wn) - a)) + tan_c / (std::fabs(wn) - a);
    const double eps = TRC_FP_EPS_REL * half;
    if (M < 32) M = 32;
    M = (M + 31) & ~31;
    const int Mc = M >> TRC_FP_SHIFT;
    const double cell = 2.0 * half / M, ccell = cell * (1 << TRC_FP_SHIFT);
    const double hd = 0.5 * cell * std::sqrt(2.0), chd = 0.5 * ccell * std::sqrt(2.0);
    P.M = M; P.Mc = Mc; P.half = (float)half; P.inv_cell = (float)(M / (2.0 * half));
    F.mask.assign((size_t)M * M / 32, 0u);
    std::vector<std::vector<uint32_t>> lists((size_t)Mc * Mc);
    double depth_min = INFINITY;
    std::vector<double> hx, hy;
    std::vector<trc_fp_print> prints;
    for (int s = 0; s < n_surf; ++s) {
        double l[3], h[3];
        bool global_axes;
        if (!trc_surface_local_box(surfs[s], l, h, &global_axes)) { F.ok = false; F.why = "unbounded surface"; return; }
        std::vector<std::pair<double, double>> pts;
        double depth_max = -INFINITY, d_lo = INFINITY;
        for (int c = 0; c < 8; ++c) {
            double q[3];
            trc_surface_box_corner(surfs[s], l, h, global_axes, c, q);
            const double v[3] = {q[0] - src.center[0], q[1] - src.center[1], q[2] - src.center[2]};
            const double depth = dot(v, nrm) / wn;                  // distance along w from the source plane to the corner
            const double f[3] = {v[0] - depth * w[0], v[1] - depth * w[1], v[2] - depth * w[2]};
            pts.emplace_back(dot(f, e1), dot(f, e2));
            depth_max = std::fmax(depth_max, depth); d_lo = std::fmin(d_lo, depth);
        }
        if (!(depth_max > 0.0)) continue;                           // wholly behind the source plane: no fresh ray reaches it
        depth_min = std::fmin(depth_min, d_lo);
        // |h| = |depth * wn| <= depth_max |wn| for the corners in front; corners behind (depth < 0) are not reached
        const double margin = depth_max * std::fabs(wn) * K + eps + 1e-9 * (half + depth_max);
        trc_fp_hull(pts, hx, hy);
        // (the mask over the uniforms needs no eps: the kernel's step from the bits to the cell is exact, and the 1e-9 term covers
        // the float64 rounding of the start point)
        if (with_umask) prints.push_back({hx, hy, depth_max * std::fabs(wn) * K + 1e-9 * (half + depth_max)});
        double bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
        for (size_t k = 0; k < hx.size(); ++k) { bx0 = std::fmin(bx0, hx[k]); bx1 = std::fmax(bx1, hx[k]); by0 = std::fmin(by0, hy[k]); by1 = std::fmax(by1, hy[k]); }
        auto range = [&](double lo, double hi, double c, int n, int *i0, int *i1) {
            double a0 = std::floor((lo + half) / c), a1 = std::floor((hi + half) / c);
            *i0 = a0 < 0.0 ? 0 : (a0 > n - 1 ? n - 1 : (int)a0);
            *i1 = a1 < 0.0 ? 0 : (a1 > n - 1 ? n - 1 : (int)a1);
            return !(hi + half < 0.0) && !(lo + half > c * n);
        };
        int x0, x1, y0, y1;
        if (range(bx0 - margin - cell, bx1 + margin + cell, cell, M, &x0, &x1) && range(by0 - margin - cell, by1 + margin + cell, cell, M, &y0, &y1))
            for (int iy = y0; iy <= y1; ++iy)
                for (int ix = x0; ix <= x1; ++ix) {
                    const double cx = -half + (ix + 0.5) * cell, cy = -half + (iy + 0.5) * cell;
                    if (trc_fp_dist_poly(hx, hy, cx, cy) <= margin + hd) F.mask[((size_t)iy * M + ix) >> 5] |= 1u << (ix & 31);
                }
        if (range(bx0 - margin - ccell, bx1 + margin + ccell, ccell, Mc, &x0, &x1) && range(by0 - margin - ccell, by1 + margin + ccell, ccell, Mc, &y0, &y1))
            for (int iy = y0; iy <= y1; ++iy)
                for (int ix = x0; ix <= x1; ++ix) {
                    const double cx = -half + (ix + 0.5) * ccell, cy = -half + (iy + 0.5) * ccell;
                    if (trc_fp_dist_poly(hx, hy, cx, cy) <= margin + chd) lists[(size_t)iy * Mc + ix].push_back((uint32_t)s);   // ascending s
                }
    }
    size_t total = 0, bits = 0;
    for (auto &v : lists) total += v.size();
    for (uint32_t wd : F.mask) bits += (size_t)__builtin_popcount(wd);
    F.coverage = (double)bits / ((double)M * M);
    F.coff.assign((size_t)Mc * Mc + 1, 0u);
    F.clist.assign(total > 0 ? total : 1, 0);
    size_t k = 0;
    for (size_t c = 0; c < lists.size(); ++c) {
        F.coff[c] = (uint32_t)k;
        for (uint32_t s : lists[c]) F.clist[k++] = s;
    }
    F.coff[lists.size()] = (uint32_t)k;
    // a ray can be advanced to just before the nearest depth of any box: a point at parameter t has depth
    // t (cos(theta) + sin(theta) (u.n) / wn) <= t (1 + a / |wn|)
    const double t_min = depth_min / (1.0 + a / std::fabs(wn));
    const double slack = 4.0 * (double)A.delta + 1e-6 * std::fabs(t_min);
    P.t_adv = (std::isfinite(t_min) && t_min - slack > 0.0) ? t_min - slack : 0.0;
    if (with_umask) {
        int m = 32;
        while (2 * m <= M) m *= 2;
        std::vector<uint32_t> um;
        size_t best = 0;
        for (int k = 0; k < 3; ++k) {
            const int Mu = k == 0 ? m / 2 : (k == 1 ? m : 2 * m), Mv = k == 0 ? 2 * m : (k == 1 ? m : m / 2);
            if (Mu < 64) continue;
            const size_t set = trc_fp_build_umask(P.kind, src.p, prints, Mu, Mv, um);
            if (F.umask.empty() || set < best) { best = set; F.umask.swap(um); F.Mu = Mu; F.Mv = Mv; }
        }
        F.ucoverage = (double)best / ((double)F.Mu * F.Mv);
    }
    F.ok = true;
}
#endif  // TRC_FOOTPRINT_H
