// umask_check.cpp -- TEST-ONLY host build of the footprint map's mask over the uniforms (tracer_amd/csrc/trc_footprint.h).
//
// What k_s_ucull decides from the top bits of a ray's two position uniforms, and what k_s_fresh2 then derives from the float32
// start point, against a float64 brute-force trace of the same rays: a ray that hits a surface and does not take the general
// path has its umask bit set, and the Cartesian list cell of its float32 start point lists that surface.  The integer form of
// the general-path test against trc_fp_generic.  Built by `make umaskcheck` as a shared library for tests/test_umask_host.py and
// as a program of its own (`make umaskcheck-exe`, the form that is run under sanitizers): it reads the scenes the test wrote
// with write_cases() and checks the same.  Not a product path.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../tracer_amd/csrc/trc_core.h"
#include "../../tracer_amd/csrc/trc_bounds.h"
#include "../../tracer_amd/csrc/trc_footprint.h"

static void pack_record(const trc_surface_desc &s, double *rec, int stride) {
    for (int i = 0; i < stride; ++i) rec[i] = 0.0;
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) rec[3 * r + k] = s.frame[4 * r + k];
        rec[9 + r] = s.frame[4 * r + 3];
    }
    int32_t h[4] = {s.gm_kind, s.optics_kind, s.extra_off, s.extra_len};
    memcpy(rec + 12, h, sizeof(h));
    int np = trc_gm_nparams(s.gm_kind);
    for (int i = 0; i < np; ++i) rec[TRC_REC_HDR + i] = s.gm[i];
}

extern "C" {

// out[0] rays, [1] general path, [2] umask bit set, [3] hits, [4] VIOLATIONS of the umask (a hit ray, not general, bit clear),
// [5] VIOLATIONS of the list (... its Cartesian list cell does not list the surface), [6] ucoverage, [7] coverage, [8] Mu, [9] Mv,
// [10] rays with the Cartesian bit set, [11] rays on which trc_fp_generic_u differs from trc_fp_generic, [12] set bits of the
// umask that the builder's own count disagrees with (0), [13] hit rays whose cell's wrap neighbour b = Mv - 1 or 0 was theirs
// (rays at the u1 = 0 / 1 seam that hit).  Returns 0, or -3 when the map does not apply (reason in `why`).
int uc_umask(int n_surf, const trc_surface_desc *surfs, const double *extra, const trc_source_desc *src, long n, uint64_t seed,
             uint64_t offset, int M, double *out, char *why, int why_len) {
    int max_np = 0;
    for (int i = 0; i < n_surf; ++i) { int np = trc_gm_nparams(surfs[i].gm_kind); if (np > max_np) max_np = np; }
    int stride = TRC_REC_HDR + max_np;
    if ((stride & 1) == 0) stride += 1;
    std::vector<double> recs((size_t)n_surf * stride);
    for (int i = 0; i < n_surf; ++i) pack_record(surfs[i], recs.data() + (size_t)i * stride, stride);
    trc_accel_host H;
    trc_accel_build_surfaces(surfs, n_surf, H);
    trc_fp_host F;
    trc_fp_build(surfs, n_surf, H, *src, F, M);
    for (int k = 0; k < 14; ++k) out[k] = 0.0;
    if (!F.ok) { if (why && why_len > 0) { strncpy(why, F.why, (size_t)why_len - 1); why[why_len - 1] = 0; } return -3; }
    const trc_fp_params &P = F.P;
    out[6] = F.ucoverage; out[7] = F.coverage; out[8] = F.Mu; out[9] = F.Mv;
    if (F.Mu < 64 || F.Mv < 2 || (F.Mu & (F.Mu - 1)) || (F.Mv & (F.Mv - 1)) || (long long)F.Mu * F.Mv > (long long)P.M * P.M ||
        F.umask.size() != (size_t)F.Mu * F.Mv / 32) return -4;
    size_t bits = 0;
    for (uint32_t w : F.umask) bits += (size_t)__builtin_popcount(w);
    out[12] = std::fabs((double)bits - F.ucoverage * (double)F.Mu * F.Mv) > 0.5 ? 1.0 : 0.0;
    int lu = 0, lv = 0;
    while ((1 << lu) < F.Mu) ++lu;
    while ((1 << lv) < F.Mv) ++lv;
    bool gen_on;
    const uint32_t gen_thr = trc_fp_generic_threshold(P, &gen_on);
    const int U = trc_fp_first_uniform(P.kind);
    for (long i = 0; i < n; ++i) {
        const uint64_t rid = offset + (uint64_t)i;
        double px, py, pz, dx, dy, dz;
        trc_source_ray(src, src->buie, nullptr, seed, rid, &px, &py, &pz, &dx, &dy, &dz);
        double tb; int sb;
        trc_nearest_brute(recs.data(), stride, n_surf, extra, px, py, pz, dx, dy, dz, &tb, &sb);
        uint32_t o[4];
        trc_philox4x32_10((uint32_t)rid, (uint32_t)(rid >> 32), 0, 0, (uint32_t)seed, (uint32_t)(seed >> 32), o);
        // k_s_ucull
        uint32_t word, b;
        trc_fp_ucell(o[U], o[U + 1], lu, lv, &word, &b);
        if (word >= F.umask.size() || b > 31u) return -5;
        const bool ubit = (F.umask[word] >> b) & 1u;
        const bool generic = trc_fp_generic(P, o);
        if (trc_fp_generic_u(gen_on, gen_thr, o[2]) != generic) out[11] += 1.0;
        // k_s_fresh2, phase 1: the list cell from the float32 start point
        float lx, ly;
        trc_fp_position32(P, o, &lx, &ly);
        int32_t ix, iy;
        trc_fp_cell(P, lx, ly, &ix, &iy);
        const bool cbit = (F.mask[((size_t)iy * P.M + ix) >> 5] >> (ix & 31)) & 1u;
        const size_t c = (size_t)(iy >> TRC_FP_SHIFT) * P.Mc + (ix >> TRC_FP_SHIFT);
        bool listed = false;
        for (uint32_t k = F.coff[c]; k < F.coff[c + 1]; ++k) if ((int)F.clist[k] == sb) listed = true;
        out[0] += 1.0;
        if (generic) out[1] += 1.0;
        if (ubit) out[2] += 1.0;
        if (cbit) out[10] += 1.0;
        if (sb >= 0) out[3] += 1.0;
        if (sb >= 0 && !generic) {
            if (!ubit) out[4] += 1.0;
            if (!listed) out[5] += 1.0;
            const uint32_t bcell = o[U + 1] >> (32 - lv);
            if (bcell == 0u || bcell == (uint32_t)F.Mv - 1u) out[13] += 1.0;
        }
    }
    return 0;
}

// trc_fp_generic against its integer form on given values of o[2]; returns the number of values on which they differ.
// *threshold, *on: what trc_fp_generic_threshold makes of (has_generic, cdf_end).
long uc_generic(int has_generic, double cdf_end, long n, const uint32_t *o2, double *threshold, int *on) {
    trc_fp_params P;
    memset(&P, 0, sizeof(P));
    P.has_generic = has_generic; P.cdf_end = cdf_end;
    bool gen_on;
    const uint32_t thr = trc_fp_generic_threshold(P, &gen_on);
    *threshold = (double)thr; *on = gen_on ? 1 : 0;
    long bad = 0;
    for (long i = 0; i < n; ++i) {
        const uint32_t o[4] = {0u, 0u, o2[i], 0u};
        if (trc_fp_generic(P, o) != trc_fp_generic_u(gen_on, thr, o2[i])) ++bad;
    }
    return bad;
}

}  // extern "C"

#ifdef UMASK_CHECK_MAIN
// The cases of tests/umask_cases.py as write_cases() stores them, one after the other:
//   int32 n_surf, M, n_table; int64 n_extra, n_rays; uint64 seed, offset; the surface descriptors; extra (n_extra doubles); the
//   source descriptor; n_table doubles of a sunshape table (its address goes into the descriptor's buie[0]).
template <class T> static bool rd(FILE *f, T *p, size_t n = 1) { return fread(p, sizeof(T), n, f) == n; }
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int bad = 0, n_cases = 0;
    for (;;) {
        int32_t hdr[3];
        if (!rd(f, hdr, 3)) break;
        int64_t cnt[2]; uint64_t so[2];
        if (!rd(f, cnt, 2) || !rd(f, so, 2)) { bad = 1; break; }
        std::vector<trc_surface_desc> surfs((size_t)hdr[0]);
        std::vector<double> extra((size_t)(cnt[0] > 0 ? cnt[0] : 1)), table((size_t)hdr[2]);
        trc_source_desc src;
        if (!rd(f, surfs.data(), surfs.size()) || (cnt[0] > 0 && !rd(f, extra.data(), (size_t)cnt[0])) || !rd(f, &src) ||
            (hdr[2] > 0 && !rd(f, table.data(), table.size()))) { bad = 1; break; }
        if (hdr[2] > 0) { const uint64_t a = (uint64_t)(uintptr_t)table.data(); memcpy(&src.buie[0], &a, sizeof(a)); }
        double out[14];
        char why[128] = "";
        const int rc = uc_umask(hdr[0], surfs.data(), extra.data(), &src, (long)cnt[1], so[0], so[1], hdr[1], out, why, 128);
        printf("case %d: kind %d rc %d %s rays %.0f hits %.0f general %.0f umask %d x %d ucoverage %.4f coverage %.4f violations %.0f %.0f generic mismatches %.0f\n",
               n_cases, src.kind, rc, why, out[0], out[3], out[1], (int)out[8], (int)out[9], out[6], out[7], out[4], out[5], out[11]);
        if (rc != 0 || out[4] != 0.0 || out[5] != 0.0 || out[11] != 0.0 || out[12] != 0.0 || !(out[3] > 0.0)) bad = 1;
        // the integer form of the general-path test around its threshold
        const bool buie = src.kind == TRC_SRC_BUIE_DISK || src.kind == TRC_SRC_BUIE_RECT;
        const double ends[3] = {buie ? src.buie[2 * (TRC_BUIE_NELEM + 1) + TRC_BUIE_NELEM] : 0.98, 1.0, 0.0};
        for (double ce : ends) {
            double t; int on;
            uc_generic(1, ce, 0, nullptr, &t, &on);
            const uint32_t thr = (uint32_t)t;
            const uint32_t o2[9] = {0u, 1u, 0xFFFFFFFFu, 0xFFFFFFFEu, thr, thr + 1u, thr - 1u, thr + 2u, thr - 2u};
            if (uc_generic(1, ce, 9, o2, &t, &on) != 0) bad = 1;
        }
        ++n_cases;
    }
    fclose(f);
    printf("%d cases, %s\n", n_cases, bad || !n_cases ? "FAILED" : "ok");
    return bad || !n_cases ? 1 : 0;
}
#endif
