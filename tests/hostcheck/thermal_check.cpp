// thermal_check.cpp -- TEST-ONLY host build of the thermal-emitter parts of the per-ray core (tracer_amd/csrc/trc_core.h:
// trc_emittance_pack, trc_emittance_theta, trc_thermal_point_u, trc_thermal_ray through trc_source_ray).  Built by `make hostcheck`
// into tests/hostcheck/libtrc_thermal_check.so, loaded only by the thermal tests; with -DTHERMAL_CHECK_MAIN the same source is a
// program (`make thermalcheck`, built with the address and undefined-behaviour sanitizers) that runs the inversion grid of
// tests/test_thermal_sources_host.py on tables of its own making and checks it against a restatement of the CDF in long double.
// Not a product path.
#include <string.h>
#include "../../tracer_amd/csrc/trc_forms.h"

extern "C" {

int ht_kind(void) { return TRC_SRC_EMIT_THERMAL; }
long ht_sizeof_source_desc(void) { return (long)sizeof(trc_source_desc); }
double ht_theta_max(void) { return TRC_EMITTANCE_THETA_MAX; }
int ht_is_emitter(int kind) { return trc_src_kind_is_emitter(kind) ? 1 : 0; }
int ht_is_lamp(int kind) { return trc_src_kind_is_lamp(kind) ? 1 : 0; }

// tab[3n] = theta | eps / M | cdf as trc_emittance_table_create packs them, *mass = M; 0 for a table without mass
int ht_pack(int n, const double *theta, const double *eps, double *tab, double *mass) {
    return trc_emittance_pack(n, theta, eps, tab, mass) ? 1 : 0;
}
// what trc_emittance_table_create refuses a table for before it packs it ("" for a table it takes)
const char *ht_table_fault(int n, const double *theta, const double *eps) {
    const char *f = trc_emittance_table_fault(n, theta, eps);
    return f ? f : "";
}

// the polar angles of m uniforms, and the iterations each took
void ht_theta(const double *tab, int n, long m, const double *u, double *theta, int *iters) {
    for (long k = 0; k < m; ++k) theta[k] = trc_emittance_theta(tab, n, u[k], &iters[k]);
}

// points and normals of a shape (p as the descriptor's) in the source's own frame from GIVEN uniforms u[2][m]
void ht_points_u(const double *p, long m, const double *u, double *x, double *y, double *z, double *nx, double *ny, double *nz) {
    for (long k = 0; k < m; ++k) trc_thermal_point_u(p, u[k], u[m + k], &x[k], &y[k], &z[k], &nx[k], &ny[k], &nz[k]);
}

// the direction of polar angle theta and azimuth uniform u3 about the unit vector n
void ht_dirs(long m, const double *theta, const double *u3, const double *nx, const double *ny, const double *nz, double *ax, double *ay,
             double *az) {
    for (long k = 0; k < m; ++k) trc_thermal_dir(theta[k], u3[k], nx[k], ny[k], nz[k], &ax[k], &ay[k], &az[k]);
}

static trc_source_desc ht_resolved(const trc_source_desc *src_in, const double *tab, int n_tab) {
    trc_source_desc src = *src_in;              // as source_resolve leaves a thermal descriptor
    src.p[TRC_SUNSHAPE_P_N] = (double)n_tab;
    memset(src.buie, 0, sizeof(src.buie));
    src.buie[0] = __builtin_bit_cast(double, (uint64_t)(uintptr_t)tab);
    return src;
}

// rays rid0 .. rid0+m-1 with their Philox draws, through the entry every engine's generation goes through; also the normal each
// ray's direction is drawn about, in the source's own frame (sign * the shape's: rot_dir poses it), and its four uniforms u[4][m]
void ht_rays(const trc_source_desc *src_in, const double *tab, int n_tab, unsigned long long seed, unsigned long long rid0, long m,
             double *x, double *y, double *z, double *dx, double *dy, double *dz, double *nx, double *ny, double *nz, double *u) {
    const trc_source_desc src = ht_resolved(src_in, tab, n_tab);
    for (long k = 0; k < m; ++k) {
        const unsigned long long rid = rid0 + (unsigned long long)k;
        trc_source_ray(&src, src.buie, nullptr, seed, rid, &x[k], &y[k], &z[k], &dx[k], &dy[k], &dz[k]);
        double u0, u1, u2, u3, lx, ly, lz;
        trc_uniform_quad(seed, rid, 0, 0, &u0, &u1, &u2, &u3);
        u[k] = u0; u[m + k] = u1; u[2 * m + k] = u2; u[3 * m + k] = u3;
        trc_thermal_point_u(src.p, u0, u1, &lx, &ly, &lz, &nx[k], &ny[k], &nz[k]);
        nx[k] *= src.p[6]; ny[k] *= src.p[6]; nz[k] *= src.p[6];
    }
}

}

#ifdef THERMAL_CHECK_MAIN
#include <algorithm>
#include <stdio.h>
#include <vector>

// the CDF restated from the raw table in long double: every interval with its own slope at both its ends
static long double H_ld(long double a, long double b, long double t) {
    return (a * t + b) / 2.0L * sinl(t) * sinl(t) - a / 4.0L * (t - sinl(t) * cosl(t));
}
static long double F_ld(const std::vector<double> &th, const std::vector<double> &ep, double x) {
    const int n = (int)th.size();
    long double tot = 0.0L, at = 0.0L;
    for (int i = 0; i + 1 < n; ++i) {
        const long double a = ((long double)ep[i + 1] - ep[i]) / ((long double)th[i + 1] - th[i]), b = ep[i] - a * th[i];
        tot += H_ld(a, b, th[i + 1]) - H_ld(a, b, th[i]);
        if (x >= th[i + 1]) at += H_ld(a, b, th[i + 1]) - H_ld(a, b, th[i]);
        else if (x > th[i]) at += H_ld(a, b, x) - H_ld(a, b, th[i]);
    }
    return at / tot;
}
static double r8(double x) { return round(x * 1e8) / 1e8; }

int main() {
    struct Table { const char *name; std::vector<double> th, ep; };
    std::vector<Table> T;
    {
        Table d = {"dir", {}, {}};
        for (int i = 0; i < 10; ++i) {
            const double t = r8(TRC_PI / 2.0 * i / 9.0), g = (t - 1.2) / 0.2;
            d.th.push_back(t);
            d.ep.push_back(i == 9 ? 0.0 : r8(0.9 * pow(fmax(cos(t), 0.0), 0.3) * (1.0 - 0.5 * exp(-g * g))));
        }
        T.push_back(d);
        Table g5 = {"gray", {}, {}};
        for (int i = 0; i < 5; ++i) { g5.th.push_back(r8(TRC_PI / 2.0 * i / 4.0)); g5.ep.push_back(0.8); }
        T.push_back(g5);
        T.push_back({"gray2", {0.0, r8(TRC_PI / 2.0)}, {0.8, 0.8}});
        T.push_back({"cone", {0.0, 0.3, 0.6}, {1.0, 1.0, 0.5}});
        T.push_back({"gap", {0.0, 0.3, 0.5, 0.9, 1.2, 1.5}, {0.6, 0.9, 0.0, 0.0, 0.7, 0.2}});
        T.push_back({"steep", {0.0, 0.4, 1.0, 1.5}, {0.0, 1.0, 0.3, 0.0}});
    }
    int bad = 0;
    for (const Table &t : T) {
        const int n = (int)t.th.size();
        std::vector<double> tab(3 * (size_t)n);
        double mass = 0.0;
        if (trc_emittance_table_fault(n, t.th.data(), t.ep.data()) || !trc_emittance_pack(n, t.th.data(), t.ep.data(), tab.data(), &mass) || tab[3 * n - 1] != 1.0) {
            printf("%s: pack failed\n", t.name);
            return 1;
        }
        const std::vector<double> th(tab.begin(), tab.begin() + n);      // (the angles as packed: the last read as pi/2)
        const long m = 100000;
        std::vector<double> u((size_t)m);
        uint64_t s = 0x9E3779B97F4A7C15ull;                 // splitmix64
        for (long k = 0; k < m; ++k) {
            uint64_t z = (s += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            u[(size_t)k] = (double)(z >> 11) * (1.0 / 9007199254740992.0);
        }
        const double edge[6] = {0.0, ldexp(1.0, -33), ldexp(1.0, -32), 0.5, 1.0 - ldexp(1.0, -32), 1.0 - ldexp(1.0, -53)};
        for (int k = 0; k < 6; ++k) u[(size_t)k] = edge[k];
        for (int k = 0; k + 1 < n; ++k) u[(size_t)(6 + k)] = tab[2 * (size_t)n + k];
        std::sort(u.begin(), u.end());
        double prev = -1.0, worst = 0.0;
        int it_max = 0;
        for (long k = 0; k < m; ++k) {
            int it = 0;
            const double x = trc_emittance_theta(tab.data(), n, u[(size_t)k], &it);
            const double res = (double)fabsl(F_ld(th, t.ep, x) - (long double)u[(size_t)k]);
            if (res > worst) worst = res;
            if (it > it_max) it_max = it;
            bool ok = res <= 1e-12 && x >= th[0] && x <= th[n - 1] && x >= prev && it < TRC_EMITTANCE_MAX_ITER;
            if (!strcmp(t.name, "gap") && x > 0.5 && x < 0.9) ok = false;
            if (!strncmp(t.name, "gray", 4) && !(fabs(x - atan2(sqrt(u[(size_t)k]), sqrt(1.0 - u[(size_t)k]))) <= 1e-12)) ok = false;
            if (!ok && bad++ < 10) printf("%s: u = %.17g theta = %.17g residual %.3g iterations %d previous %.17g\n", t.name, u[(size_t)k], x, res, it, prev);
            prev = x;
        }
        printf("%-6s mass %.16g  worst residual %.3g  most iterations %d\n", t.name, mass, worst, it_max);
    }
    printf(bad ? "thermal_check: %d FAILED\n" : "thermal_check: OK\n", bad);
    return bad ? 1 : 0;
}
#endif
