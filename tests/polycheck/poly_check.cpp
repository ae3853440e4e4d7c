// poly_check -- what k_s_shade_p rests on, checked on the host as a program of its own (built with the sanitizers, `make polycheck`):
//
//   interp   trc_interp2_at(tab, cell_theta, w_theta, cell_lambda, w_lambda), with the cells trc_grid_cell gives, equals
//            trc_interp2(tab, theta, lambda) bit for bit: over tables of 2 x 2, 3 x 5 and 64 x 64 nodes, 1e5 fuzzed (theta, lambda)
//            each, among them values on nodes, below the first node, at and beyond the last, and NaN.  One line per table:
//            "interp NT NL checked mismatches".
//   ids      every id of family k_s_shade_p the header holds valid, as a kernel trace spells it: "id NAME".
//   choose   the shading stage trc_stream_form_shade decides for the fact blocks given on the command line, eleven integers each:
//            n_surf stride n_fm_edges fms_bytes n_extra fm_bins chart splits poly_src poly_walls mat_dev
//            "choose NAME lds_bytes tables_in_lds bins_in_lds cells" (or "choose none").
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../include/tracer_amd.h"
#include "../../tracer_amd/csrc/trc_core.h"
#include "../../tracer_amd/csrc/trc_forms.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

static long check_table(int nt, int nl, long n, long *checked) {
    std::vector<double> tab((size_t)2 + nt + nl + (size_t)nt * nl);
    tab[0] = nt; tab[1] = nl;
    double *ts = tab.data() + 2, *ls = ts + nt, *v = ls + nl;
    double x = 0.0;
    for (int i = 0; i < nt; ++i) { ts[i] = x; x += 0.01 + uni() * 1.5 / nt; }     // uneven nodes, strictly increasing
    x = 0.3e-6;
    for (int i = 0; i < nl; ++i) { ls[i] = x; x += 1e-9 + uni() * 2.2e-6 / nl; }
    for (int i = 0; i < nt * nl; ++i) v[i] = uni();
    long bad = 0;
    for (long k = 0; k < n; ++k) {
        double th, lam;
        // a third of the draws on special values of either axis: a node, below the first, the last, beyond it, NaN
        auto pick = [&](const double *xs, int m) {
            const double lo = xs[0], hi = xs[m - 1];
            switch (rnd() % 15) {
            case 0: return xs[rnd() % m];
            case 1: return lo - uni() * (hi - lo);
            case 2: return hi;
            case 3: return hi + uni() * (hi - lo);
            case 4: return (double)NAN;
            default: return lo + uni() * (hi - lo);
            }
        };
        th = pick(ts, nt); lam = pick(ls, nl);
        double wt, wl;
        const int it = trc_grid_cell(ts, nt, th, &wt), il = trc_grid_cell(ls, nl, lam, &wl);
        if (it < 0 || it > nt - 2 || il < 0 || il > nl - 2) { ++bad; continue; }       // (the cells index the table: never outside it)
        const double a = trc_interp2_at(tab.data(), it, wt, il, wl), b = trc_interp2(tab.data(), th, lam);
        uint64_t ua, ub;
        memcpy(&ua, &a, 8); memcpy(&ub, &b, 8);
        if (ua != ub) ++bad;
        ++*checked;
    }
    return bad;
}

int main(int argc, char **argv) {
    const int shapes[3][2] = {{2, 2}, {3, 5}, {64, 64}};
    for (auto &s : shapes) {
        long checked = 0;
        const long bad = check_table(s[0], s[1], 100000, &checked);
        printf("interp %d %d %ld %ld\n", s[0], s[1], checked, bad);
    }
    for (int a = 0; a < 8; ++a) {
        const trc_kernel_id id = trc_kid(TRC_K_SHADE_P, a & 1, (a >> 1) & 1, (a >> 2) & 1);
        char name[96];
        if (!trc_kernel_id_valid(id)) continue;
        trc_kernel_name(id, name, sizeof(name));
        printf("id %s\n", name);
    }
    for (int k = 1; k + 10 < argc; k += 11) {
        trc_facts f = {};
        int v[11];
        for (int j = 0; j < 11; ++j) v[j] = atoi(argv[k + j]);
        f.scene.n_surf = v[0]; f.scene.stride = v[1]; f.scene.n_fm_edges = v[2]; f.scene.fms_bytes = v[3]; f.scene.n_extra = v[4];
        f.scene.fm_bins = v[5]; f.scene.chart = v[6] != 0; f.scene.splits = v[7] != 0;
        f.scene.walked = true; f.scene.cls_all = f.scene.cls_moving = 1u << TRC_CLS_GENERAL;
        f.call.n = 4096; f.call.src_kind = TRC_SRC_PILLBOX_RECT; f.call.term_ok = true;
        f.call.poly_src = v[8]; f.call.poly_walls = v[9]; f.call.mat_dev = v[10] != 0;
        f.call.carry = f.call.poly_src > 0 || f.scene.splits || f.call.mat_dev;      // (as the streaming engine sets it)
        f.call.spec = f.call.poly_src > 0;
        trc_stream_forms F;
        memset(&F, 0, sizeof(F));
        if (!trc_stream_form_shade(F, f) || F.n_shk != 1) { printf("choose none\n"); continue; }
        char name[96];
        trc_kernel_name(F.shk[0].id, name, sizeof(name));
        printf("choose %s | %zu %d %d %d\n", name, F.shk[0].lds, F.shk[0].lds_tables, F.shk[0].lds_fm_bins, F.poly_cells);
    }
    return 0;
}
