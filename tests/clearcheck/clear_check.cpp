// clear_check.cpp -- TEST-ONLY host build of the clear cones (trc_clear_build in tracer_amd/csrc/trc_bounds.h, trc_clear_tile and
// trc_clear_inside in trc_core.h: what k_s_bounce leaves the grid walk out by).
//
// cc_sound draws rays that start on the plates and run inside the stored cones -- edges, corners and tile seams included, on the
// plane and delta off it on either side, angles uniform up to the boundary and a share of them at 0.999 of it -- decides the skip
// exactly as the kernel does (single-precision ray of trc_ray32_prepare, tile and test of trc_core.h) and searches every ray that
// skips by brute force over the boxes a walking ray is tested with (trc_box_hit32 and trc_obb_hit32 of every surface the grid
// lists).  A ray that skips while a listed surface passes both boxes is a violation.  cc_walk_share traces source rays to their
// first hit in float64, shades them and reports how many of the rays that go on still walk.  Built by `make clearcheck` as a
// shared library for tests/test_clear_cones_host.py and as a program of its own under the sanitizers, which builds the tables of
// the scenes the test wrote with write_cases() and runs a short soundness pass.  Not a product path.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include <algorithm>
#include "../../tracer_amd/csrc/trc_core.h"
#include "../../tracer_amd/csrc/trc_bounds.h"
#include "../../tracer_amd/csrc/trc_scene_host.h"

namespace {

struct Rng {        // splitmix64: the check's own uniforms
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double u() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

double build_tables(const trc_surface_desc *surfs, int n, int T, trc_accel_host &A) {
    trc_accel_build_surfaces(surfs, n, A);
    trc_accel_build_grid(A, n);
    const auto t0 = std::chrono::steady_clock::now();
    trc_clear_build(surfs, n, T, A);
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// the kernel's decision for a continued ray that left surface h (k_s_bounce<1, .., false>): 0 it walks the grid, 1 it skips the walk
// inside its tile's cone, 2 it misses the grid's box and walks in neither build
int kernel_skips(const trc_accel_host &A, int T, double kscale, int h, double px, double py, double pz, double dx, double dy, double dz, trc_ray32 *r) {
    double t0;
    if (!trc_ray32_prepare(A.slo, A.shi, A.cen, px, py, pz, dx, dy, dz, r, &t0)) return 2;
    float tmin, tmax;
    if (!trc_kd32_root(A.grid_root, *r, &tmin, &tmax)) return 2;
    if (A.clear.empty() || t0 != 0.0) return 0;
    const int tile = trc_clear_tile(&A.obb[(size_t)TRC_OBB_STRIDE * h], T, r->ox, r->oy, r->oz);
    const float *c = &A.clear[((size_t)h * T * T + tile) * 4];
    return trc_clear_inside(c[0], c[1], c[2], (float)((double)c[3] * kscale), r->dx, r->dy, r->dz) ? 1 : 0;
}

}  // namespace

extern "C" {

int cc_T() { return TRC_CLEAR_T; }      // tiles per side the library is built with

// out[0] rays drawn, [1] rays that skip, [2] VIOLATIONS, [3] tiles with a cone, [4] tiles of surfaces listed in the grid, [5] seconds
// of trc_clear_build, [6] surfaces set apart, [7] smallest, [8] median, [9] largest half-angle among the cones (rad), [10] entries of
// the table whose k is negative or no number (0), [11] box pairs a skipping ray was searched against.
// kscale: every stored k times this (1: as stored; 2.25: cones 1.5 x wider, which must be caught).
int cc_sound(int n_surf, const trc_surface_desc *surfs, int T, long n_rays, uint64_t seed, double kscale, double *out) {
    for (int k = 0; k < 12; ++k) out[k] = 0.0;
    trc_accel_host A;
    out[5] = build_tables(surfs, n_surf, T, A);
    out[6] = (double)A.grid_apart.size();
    if (!A.grid_ok) return -3;
    std::vector<char> listed((size_t)n_surf, 0);
    for (size_t k = 0; k < (size_t)A.grid_off.back(); ++k) listed[A.grid_list[k]] = 1;
    std::vector<int> lst;
    for (int s = 0; s < n_surf; ++s) if (listed[s]) lst.push_back(s);
    out[4] = (double)lst.size() * T * T;
    std::vector<int> cones;         // (surface * T * T + tile) of every tile with a cone
    std::vector<double> ang;
    for (size_t i = 0; i + 3 < A.clear.size(); i += 4) {
        const float k = A.clear[i + 3];
        if (k > 0.0f) { cones.push_back((int)(i / 4)); ang.push_back(std::atan(std::sqrt((double)k))); }
        else if (!(k == 0.0f)) out[10] += 1.0;
    }
    out[3] = (double)cones.size();
    if ((int)cones.size() != A.clear_cones) return -4;
    if (cones.empty()) return 0;
    std::sort(ang.begin(), ang.end());
    out[7] = ang.front(); out[8] = ang[ang.size() / 2]; out[9] = ang.back();
    Rng R{seed * 2654435761ull + 12345u};
    const double delta = (double)A.delta;
    for (long i = 0; i < n_rays; ++i) {
        const int ct = cones[(size_t)(R.next() % cones.size())];
        const int h = ct / (T * T), tile = ct % (T * T);
        const float *B = &A.obb[(size_t)TRC_OBB_STRIDE * h];
        const float *cn = &A.clear[(size_t)ct * 4];
        // a point of the plate: inside the tile, on one of its seams, on the plate's edge or corner.  (B's bounds carry delta; the
        // plate itself ends delta inside them.)
        const int t2[2] = {tile % T, tile / T};
        double loc[3];
        for (int k = 0; k < 2; ++k) {
            const double lo = (double)B[12 + k], hi = (double)B[15 + k], w = (hi - lo) / T;
            const double a = std::fmax(lo + delta, lo + t2[k] * w), b = std::fmin(hi - delta, lo + (t2[k] + 1) * w);
            const uint64_t mode = R.next() % 8;
            loc[k] = mode == 0 ? a : (mode == 1 ? b : (mode == 2 ? std::nextafter(a, b) : (mode == 3 ? std::nextafter(b, a) : a + (b - a) * R.u())));
        }
        const uint64_t zm = R.next() % 4;
        loc[2] = zm == 0 ? delta : (zm == 1 ? -delta : 0.0);
        double p[3];
        for (int k = 0; k < 3; ++k)
            p[k] = A.cen[k] + (double)B[4 * k + 3] + (double)B[k] * loc[0] + (double)B[4 + k] * loc[1] + (double)B[8 + k] * loc[2];
        // a direction inside the (scaled) cone
        double a[3] = {cn[0], cn[1], cn[2]};
        const double an = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int k = 0; k < 3; ++k) a[k] /= an;
        const int m = std::fabs(a[0]) < std::fabs(a[1]) ? (std::fabs(a[0]) < std::fabs(a[2]) ? 0 : 2) : (std::fabs(a[1]) < std::fabs(a[2]) ? 1 : 2);
        double e1[3] = {0.0, 0.0, 0.0}, e2[3], n1 = 0.0;
        e1[m] = 1.0;
        const double d1 = a[m];
        for (int k = 0; k < 3; ++k) { e1[k] -= d1 * a[k]; n1 += e1[k] * e1[k]; }
        for (int k = 0; k < 3; ++k) e1[k] /= std::sqrt(n1);
        e2[0] = a[1] * e1[2] - a[2] * e1[1]; e2[1] = a[2] * e1[0] - a[0] * e1[2]; e2[2] = a[0] * e1[1] - a[1] * e1[0];
        const double amax = std::atan(std::sqrt((double)cn[3] * kscale));
        const double th = (R.next() % 5 == 0) ? 0.999 * amax : amax * R.u(), ph = 6.283185307179586 * R.u();
        double d[3];
        for (int k = 0; k < 3; ++k) d[k] = std::cos(th) * a[k] + std::sin(th) * (std::cos(ph) * e1[k] + std::sin(ph) * e2[k]);
        out[0] += 1.0;
        trc_ray32 r;
        if (kernel_skips(A, T, kscale, h, p[0], p[1], p[2], d[0], d[1], d[2], &r) != 1) continue;
        out[1] += 1.0;
        bool bad = false;
        for (int g : lst) {
            if (g == h) continue;
            out[11] += 1.0;
            if (trc_box_hit32(&A.sbox[6 * (size_t)g], r) && trc_obb_hit32(&A.obb[(size_t)TRC_OBB_STRIDE * g], r.ox, r.oy, r.oz, r.dx, r.dy, r.dz)) { bad = true; break; }
        }
        if (bad) out[2] += 1.0;
    }
    return 0;
}

// The rays that go on from the first hits of n source rays (float64 brute force, the scene's own optics), per T in Ts[0 .. nT):
// out[4 * j + 0] continued rays that leave a surface with a box in the grid's lists, [1] those of them that still walk (no cone or
// outside it), [2] those that skip although a listed surface passes both boxes (VIOLATIONS), [3] seconds of trc_clear_build.
// tail[0] source rays, [1] first hits, [2] rays that go on, [3] of those: a listed surface passes both boxes (blocked or nearly).
int cc_walk_share(int n_surf, const trc_surface_desc *surfs, const double *extra, const trc_source_desc *src, long n, uint64_t seed,
                  int nT, const int *Ts, double *out, double *tail) {
    const int stride = trc_scene_stride(surfs, n_surf);
    std::vector<double> recs((size_t)n_surf * stride);
    for (int i = 0; i < n_surf; ++i) trc_pack_record(surfs[i], recs.data() + (size_t)i * stride, stride);
    std::vector<trc_accel_host> A((size_t)nT);
    for (int j = 0; j < nT; ++j) { for (int k = 0; k < 4; ++k) out[4 * j + k] = 0.0; out[4 * j + 3] = build_tables(surfs, n_surf, Ts[j], A[(size_t)j]); }
    for (int k = 0; k < 4; ++k) tail[k] = 0.0;
    if (nT < 1 || !A[0].grid_ok) return -3;
    const trc_accel_host &A0 = A[0];
    std::vector<char> listed((size_t)n_surf, 0);
    for (size_t k = 0; k < (size_t)A0.grid_off.back(); ++k) listed[A0.grid_list[k]] = 1;
    for (long i = 0; i < n; ++i) {
        double px, py, pz, dx, dy, dz;
        trc_source_ray(src, src->buie, nullptr, seed, (uint64_t)i, &px, &py, &pz, &dx, &dy, &dz);
        tail[0] += 1.0;
        // first hit: the single-precision boxes sort out the candidates, the exact test decides (as every engine does)
        trc_ray32 r;
        double t0;
        if (!trc_ray32_prepare(A0.slo, A0.shi, A0.cen, px, py, pz, dx, dy, dz, &r, &t0)) continue;
        double tb = TRC_INF;
        int sb = -1;
        for (int s = 0; s < n_surf; ++s) {
            const float *b = &A0.sbox[6 * (size_t)s];
            if (!(b[3] == INFINITY && b[0] == -INFINITY) && !trc_box_hit32(b, r)) continue;
            const double t = trc_intersect(recs.data() + (size_t)s * stride, extra, px, py, pz, dx, dy, dz);
            if (t != 0.0 && t < tb) { tb = t; sb = s; }
        }
        if (sb < 0) continue;
        tail[1] += 1.0;
        const trc_surface_desc &S = surfs[sb];
        const double hx = px + tb * dx, hy = py + tb * dy, hz = pz + tb * dz;
        double nx, ny, nz;
        trc_normal(recs.data() + (size_t)sb * stride, hx, hy, hz, dx, dy, dz, &nx, &ny, &nz);
        trc_ray_out o[2];
        const int no = trc_shade(S.optics_kind, S.opt, extra, S.extra_off, S.extra_len, S.frame[2], S.frame[6], S.frame[10], dx, dy, dz, 1.0, 1.0, 0.0,
                                 tb, nx, ny, nz, seed, (uint64_t)i, 0u, o);
        if (no < 1 || !(o[0].e > 0.0) || o[0].back != 0.0 || o[0].shift != 0.0) continue;
        tail[2] += 1.0;
        if (!listed[sb]) continue;
        bool blocked = false, have = false;
        for (int j = 0; j < nT; ++j) {
            trc_ray32 q;
            const int skips = kernel_skips(A[(size_t)j], Ts[j], 1.0, sb, hx, hy, hz, o[0].dx, o[0].dy, o[0].dz, &q);
            if (!have) {
                have = true;
                for (int g = 0; g < n_surf && !blocked; ++g)
                    if (g != sb && listed[g] && trc_box_hit32(&A0.sbox[6 * (size_t)g], q) &&
                        trc_obb_hit32(&A0.obb[(size_t)TRC_OBB_STRIDE * g], q.ox, q.oy, q.oz, q.dx, q.dy, q.dz)) blocked = true;
                if (blocked) tail[3] += 1.0;
            }
            out[4 * j] += 1.0;
            if (skips == 0) out[4 * j + 1] += 1.0;
            else if (skips == 1 && blocked) out[4 * j + 2] += 1.0;
        }
    }
    return 0;
}

// seconds of trc_clear_build for a regular field of n_plates plates aimed at a tower and its receiver (4095: the 4096-surface figure
// of profiles/clear_cones.txt)
double cc_build_time(int n_plates, int T, int *cones) {
    std::vector<trc_surface_desc> surfs((size_t)n_plates + 1);
    int n_side = 1;
    while (n_side * n_side < n_plates) ++n_side;
    memset(surfs.data(), 0, surfs.size() * sizeof(trc_surface_desc));
    const double tower[3] = {0.0, 0.0, 120.0};
    for (size_t i = 0; i < surfs.size(); ++i) {
        trc_surface_desc &s = surfs[i];
        s.gm_kind = TRC_GM_RECT;
        const bool rec = i + 1 == surfs.size();
        s.gm[0] = s.gm[1] = rec ? 10.0 : 3.0;
        double c[3] = {((double)(i % n_side) - 0.5 * n_side) * 9.0, 40.0 + (double)(i / n_side) * 9.0, 3.0};
        if (rec) { c[0] = tower[0]; c[1] = tower[1]; c[2] = tower[2]; }
        // z axis: half way between the zenith and the tower (a sun overhead), the receiver faces +y
        double z[3] = {tower[0] - c[0], tower[1] - c[1], tower[2] - c[2]};
        double zn = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
        for (int k = 0; k < 3; ++k) z[k] /= zn;
        z[2] += 1.0;
        if (rec) { z[0] = 0.0; z[1] = 1.0; z[2] = 0.0; }
        zn = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
        for (int k = 0; k < 3; ++k) z[k] /= zn;
        double x[3] = {1.0, 0.0, 0.0};
        const double xz = x[0] * z[0] + x[1] * z[1] + x[2] * z[2];
        for (int k = 0; k < 3; ++k) x[k] -= xz * z[k];
        const double xn = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        for (int k = 0; k < 3; ++k) x[k] /= xn;
        const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
        for (int k = 0; k < 3; ++k) { s.frame[4 * k] = x[k]; s.frame[4 * k + 1] = y[k]; s.frame[4 * k + 2] = z[k]; s.frame[4 * k + 3] = c[k]; }
    }
    trc_accel_host A;
    const double t = build_tables(surfs.data(), (int)surfs.size(), T, A);
    *cones = A.clear_cones;
    return t;
}

}  // extern "C"

#ifdef CLEAR_CHECK_MAIN
// The scenes of tests/clear_cases.py as write_cases() stores them, one after the other: int32 n_surf, T; int64 n_rays; the surface
// descriptors.  Builds the tables, runs the soundness pass and frees everything: the run the sanitizers watch.
template <class V> static bool rd(FILE *f, V *p, size_t n = 1) { return fread(p, sizeof(V), n, f) == n; }
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int bad = 0, n_cases = 0;
    for (;;) {
        int32_t hdr[2];
        int64_t n_rays;
        if (!rd(f, hdr, 2)) break;
        if (!rd(f, &n_rays) || hdr[0] < 1) { bad = 1; break; }
        std::vector<trc_surface_desc> surfs((size_t)hdr[0]);
        if (!rd(f, surfs.data(), surfs.size())) { bad = 1; break; }
        double out[12];
        const int rc = cc_sound(hdr[0], surfs.data(), hdr[1], (long)n_rays, 7u, 1.0, out);
        printf("case %d: %d surfaces T %d rc %d cones %.0f of %.0f tiles, apart %.0f, rays %.0f skip %.0f violations %.0f, build %.4f s\n", n_cases, hdr[0], hdr[1],
               rc, out[3], out[4], out[6], out[0], out[1], out[2], out[5]);
        if ((rc != 0 && rc != -3) || out[2] != 0.0 || out[10] != 0.0) bad = 1;
        ++n_cases;
    }
    fclose(f);
    int cones = 0;
    cc_build_time(60, 2, &cones);
    printf("%d cases, %s\n", n_cases, bad || !n_cases ? "FAILED" : "ok");
    return bad || !n_cases ? 1 : 0;
}
#endif
