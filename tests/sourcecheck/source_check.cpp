// The host side of the tabulated sources (csrc/trc_source_host.h) without a device: the one table check on bad tables of every kind
// by status and exact message (the messages are written out here as the create functions always gave them), the packing bit for bit
// against the pack functions of trc_core.h, the id registry in order, to exhaustion and under eight threads, and the arithmetic that
// resolves a descriptor naming a table.  Built with the address and undefined-behaviour sanitizers and with the thread sanitizer
// (make sourcecheck sourcecheck-tsan) and run by tests/test_source_tables_host.py; without SOURCE_CHECK_MAIN, a library that hands
// the check-and-pack functions to the same test.  The arrays of the tables are exactly as long as their counts say.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "../../tracer_amd/csrc/trc_source_host.h"

enum { K_SUNSHAPE = 0, K_ANGLE = 1, K_EMITTANCE = 2, K_SPECTRUM = 3, K_COUNT = 4 };

// the table (x, y) of n points through the check-and-pack function of `kind` (a spectrum: a TABLE for "who"): status, reason, table
static int make(int kind, int n, const double *x, const double *y, trc_table_packed &t, char *msg, size_t len) {
    msg[0] = 0;
    if (kind == K_SUNSHAPE) return trc_sunshape_make(n, x, y, t, msg, len);
    if (kind == K_ANGLE) return trc_angle_table_make(n, x, y, t, msg, len);
    if (kind == K_EMITTANCE) return trc_emittance_table_make(n, x, y, t, msg, len);
    trc_source_spectrum sp = {TRC_SPECTRUM_TABLE, n, 0.0, 1.0, x, y};
    t.n = n;
    return trc_spectrum_make(&sp, "who", t.tab, msg, len);
}

extern "C" int sc_table(int kind, int n, const double *x, const double *y, char *msg, int len) {
    trc_table_packed t;
    return make(kind, n, x, y, t, msg, (size_t)len);
}

#ifdef SOURCE_CHECK_MAIN
static int bad = 0, checks = 0;
#define EXPECT(cond, ...) do { ++checks; if (!(cond)) { ++bad; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const char *const WHO[K_COUNT] = {"trc_sunshape_create", "trc_angle_table_create", "trc_emittance_table_create", "who"};
static const int MAX_N[K_COUNT] = {TRC_SUNSHAPE_MAX_POINTS, TRC_SUNSHAPE_MAX_POINTS, TRC_SUNSHAPE_MAX_POINTS, TRC_SPECTRUM_MAX_POINTS};

// what each kind says of a bad table, after "<who>: " (%d: the point; null: the kind has no such refusal)
struct Words { const char *count, *missing, *x_nan, *order, *y_bad, *domain, *mass; };
static const Words SAYS[K_COUNT] = {
    {"the table has %d points, 2..4096 allowed", "angles or intensities missing", "angle %d is not finite", "angles are not strictly increasing (point %d)",
     "intensity %d is negative or not finite", "angles must lie in [0, pi/2)", "the table has no mass"},
    {"the table has %d points, 2..4096 allowed", "angles or densities missing", "angle %d is not finite", "angles are not strictly increasing (point %d)",
     "density %d is negative or not finite", "angles must lie in [0, pi]", "the table has no mass"},
    {"the table must have 2..4096 points", "angles or emittances missing", "an angle is not finite", "the angles are not strictly increasing",
     "an emittance is negative or not finite", "the angles must lie in [0, pi/2]", "the table has no mass"},
    {"spectrum table has %d points, 2..4096 allowed", "spectrum table without wavelengths or values", "spectrum wavelength %d is not finite",
     "spectrum wavelengths are not strictly increasing (point %d)", "spectrum value %d is negative or not finite", nullptr,
     "spectrum table has a zero (or non-finite) integral"}};

static void refused(int kind, const char *what, const std::vector<double> &x, const std::vector<double> &y, const char *says, int point,
                    const double *xp = nullptr, const double *yp = nullptr, int n = -1) {
    char msg[512], tail[256], want[512];
    trc_table_packed t;
    const int st = make(kind, n >= 0 ? n : (int)x.size(), n >= 0 ? xp : x.data(), n >= 0 ? yp : y.data(), t, msg, sizeof(msg));
    std::snprintf(tail, sizeof(tail), says, point);
    std::snprintf(want, sizeof(want), "%s: %s", WHO[kind], tail);
    EXPECT(st == TRC_ERR_INVALID && std::strcmp(msg, want) == 0, "kind %d, %s: status %d, message '%s', expected '%s'", kind, what, st, msg, want);
}

static void refusals(int kind) {
    const Words &w = SAYS[kind];
    const double inf = INFINITY, nan = NAN;
    const std::vector<double> big((size_t)MAX_N[kind] + 1, 1.0);
    std::vector<double> ramp((size_t)MAX_N[kind] + 1);
    for (size_t i = 0; i < ramp.size(); ++i) ramp[i] = 1e-4 * (double)(i + 1);
    refused(kind, "1 point", {0.1}, {1.}, w.count, 1);
    refused(kind, "MAX + 1 points", ramp, big, w.count, MAX_N[kind] + 1);
    const double two[2] = {0.1, 0.2};
    refused(kind, "no abscissae", {}, {}, w.missing, 0, nullptr, two, 2);
    refused(kind, "no ordinates", {}, {}, w.missing, 0, two, nullptr, 2);
    refused(kind, "a NaN abscissa", {0.1, nan, 0.3}, {1., 1., 1.}, w.x_nan, 1);
    refused(kind, "equal abscissae", {0.1, 0.2, 0.2}, {1., 1., 1.}, w.order, 2);
    refused(kind, "decreasing abscissae", {0.1, 0.3, 0.2}, {1., 1., 1.}, w.order, 2);
    refused(kind, "a negative ordinate", {0.1, 0.2}, {1., -1.}, w.y_bad, 1);
    refused(kind, "an infinite ordinate", {0.1, 0.2}, {1., inf}, w.y_bad, 1);
    refused(kind, "a NaN ordinate", {0.1, 0.2}, {nan, 1.}, w.y_bad, 0);
    if (w.domain) {
        refused(kind, "a first point below 0", {-0.001, 0.2}, {1., 1.}, w.domain, 0);
        if (kind == K_SUNSHAPE) refused(kind, "a last point at pi/2", {0.1, TRC_PI / 2.0}, {1., 1.}, w.domain, 0);
        if (kind == K_ANGLE) refused(kind, "a last point above pi", {0.1, std::nextafter(TRC_PI, 4.0)}, {1., 1.}, w.domain, 0);
        if (kind == K_EMITTANCE) refused(kind, "a last point above pi/2", {0.1, 2.0}, {1., 1.}, w.domain, 0);
    }
    refused(kind, "all-zero ordinates", {0.1, 0.2, 0.3}, {0., 0., 0.}, w.mass, 0);
}

// a good table of n points is accepted and packed as the pack function of its kind packs it, bit for bit
static void accepted(int kind, int n) {
    std::vector<double> x((size_t)n), y((size_t)n), ref((size_t)3 * n, 0.0);
    const double hi = kind == K_ANGLE ? TRC_PI : kind == K_SPECTRUM ? 2.5e-6 : 1.5;
    for (int i = 0; i < n; ++i) { x[i] = hi * (double)(i + 1) / (double)n; y[i] = 1.0 + 0.5 * std::sin(7.0 * x[i] / hi); }
    char msg[512];
    trc_table_packed t;
    const int st = make(kind, n, x.data(), y.data(), t, msg, sizeof(msg));
    EXPECT(st == TRC_OK && msg[0] == 0, "kind %d, %d points: status %d, message '%s'", kind, n, st, msg);
    if (st != TRC_OK) return;
    double theta_c = 0.0, u_c = 0.0;
    if (kind == K_SUNSHAPE) trc_sunshape_pack(n, x.data(), y.data(), ref.data(), &theta_c, &u_c);
    if (kind == K_ANGLE) { trc_angle_table_pack(n, x.data(), y.data(), ref.data()); theta_c = x[n - 1]; u_c = 1.0; }
    if (kind == K_EMITTANCE) { trc_emittance_pack(n, x.data(), y.data(), ref.data(), &u_c); theta_c = ref[n - 1]; }
    if (kind == K_SPECTRUM) {       // wl | value / integral | running trapezoid integral / integral
        double cum = 0.0;
        for (int i = 0; i < n; ++i) {
            ref[i] = x[i];
            if (i > 0) cum += (x[i] - x[i - 1]) * (y[i] + y[i - 1]) / 2.;
            ref[2 * n + i] = cum;
        }
        for (int i = 0; i < n; ++i) { ref[n + i] = y[i] / cum; ref[2 * n + i] = ref[2 * n + i] / cum; }
        EXPECT(ref[3 * n - 1] == 1.0, "the CDF of %d points ends at %.17g", n, ref[3 * n - 1]);
    }
    EXPECT(t.tab.size() == ref.size() && std::memcmp(t.tab.data(), ref.data(), ref.size() * sizeof(double)) == 0, "kind %d, %d points: the packing differs", kind, n);
    if (kind != K_SPECTRUM)
        EXPECT(t.n == n && t.packing == kind && std::memcmp(&t.theta_c, &theta_c, 8) == 0 && std::memcmp(&t.u_c, &u_c, 8) == 0,
               "kind %d, %d points: n %d, packing %d, theta_c %.17g (%.17g), u_c %.17g (%.17g)", kind, n, t.n, t.packing, t.theta_c, theta_c, t.u_c, u_c);
}

static void spectrum_kinds() {
    char msg[512];
    std::vector<double> tab(3, 1.0);
    trc_source_spectrum sp = {TRC_SPECTRUM_CONSTANT, 0, 5e-7, 1.0, nullptr, nullptr};
    EXPECT(trc_spectrum_make(&sp, "who", tab, msg, sizeof(msg)) == TRC_OK && tab.empty(), "a constant spectrum: '%s', %zu", msg, tab.size());
    sp.wavelength = NAN;
    EXPECT(trc_spectrum_make(&sp, "who", tab, msg, sizeof(msg)) == TRC_ERR_INVALID && !std::strcmp(msg, "who: spectrum wavelength is not finite"), "'%s'", msg);
    sp.wavelength = 5e-7; sp.ref_index = 0.0;
    EXPECT(trc_spectrum_make(&sp, "who", tab, msg, sizeof(msg)) == TRC_ERR_INVALID && !std::strcmp(msg, "who: spectrum ref_index must be finite and positive"), "'%s'", msg);
    sp.ref_index = 1.0; sp.kind = 7;
    EXPECT(trc_spectrum_make(&sp, "who", tab, msg, sizeof(msg)) == TRC_ERR_INVALID && !std::strcmp(msg, "who: spectrum kind 7 is neither CONSTANT nor TABLE nor CARRIED"), "'%s'", msg);
}

static void registry() {
    trc_id_registry<int> R;
    int32_t id[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) EXPECT(R.add(10 * (k + 1), &id[k]) == TRC_OK && id[k] == k + 1, "id %d is %d", k, id[k]);
    int got = 0;
    EXPECT(R.find(2, [&got](int v) { got = v; }) && got == 20, "id 2 holds %d", got);
    R.erase(2);
    EXPECT(!R.find(2, [](int) {}) && R.size() == 2, "an erased id is still found (%zu entries)", R.size());
    EXPECT(R.add(40, &id[3]) == TRC_OK && id[3] == 4, "the id after an erase is %d", id[3]);
    EXPECT(!R.find(99, [](int) {}), "an id never given is found");
    // the last id given out is INT32_MAX - 1: a registry that starts there gives one, one that starts a step lower two
    for (int room = 1; room <= 2; ++room) {
        trc_id_registry<int> E(INT32_MAX - room);
        int32_t e = 0;
        for (int k = 0; k < room; ++k) EXPECT(E.add(k, &e) == TRC_OK && e == INT32_MAX - room + k, "room %d: id %d", room, e);
        const int32_t before = e;
        EXPECT(E.add(7, &e) == TRC_ERR_CAPACITY && e == before && E.size() == (size_t)room, "room %d: exhausted registry holds %zu, id %d", room, E.size(), e);
        EXPECT(E.add(7, &e) == TRC_ERR_CAPACITY && E.size() == (size_t)room && !E.find(INT32_MAX, [](int) {}), "room %d: exhausted twice", room);
    }
}

// eight threads add, find and erase: afterwards the registry holds exactly the ids not erased
static void registry_threads() {
    const int T = 8, PER = 2000;
    trc_id_registry<int> R;
    std::vector<std::vector<int32_t>> kept(T);
    std::vector<int> wrong(T, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t]() {
            for (int k = 0; k < PER; ++k) {
                int32_t id = 0;
                if (R.add(t * PER + k, &id) != TRC_OK) { ++wrong[t]; continue; }
                int v = -1;
                if (!R.find(id, [&v](int x) { v = x; }) || v != t * PER + k) ++wrong[t];
                if (k % 3 == 0) { R.erase(id); if (R.find(id, [](int) {})) ++wrong[t]; }
                else kept[t].push_back(id);
            }
        });
    for (auto &x : th) x.join();
    size_t n_kept = 0;
    std::vector<char> seen((size_t)T * PER + 1, 0);
    for (int t = 0; t < T; ++t) {
        EXPECT(wrong[t] == 0, "thread %d saw %d wrong answers", t, wrong[t]);
        for (int32_t id : kept[t]) {
            int v = -1;
            EXPECT(id >= 1 && id <= T * PER && !seen[id] && R.find(id, [&v](int x) { v = x; }) && v / PER == t, "id %d of thread %d holds %d", id, t, v);
            if (id >= 1 && id <= T * PER) seen[id] = 1;
            ++n_kept;
        }
    }
    EXPECT(R.size() == n_kept, "the registry holds %zu entries, %zu were kept", R.size(), n_kept);
}

static trc_source_desc desc_of(int kind) {
    trc_source_desc s;
    std::memset(&s, 0, sizeof(s));
    s.kind = kind; s.table = 5; s.energy = 0.25;
    for (int i = 0; i < 8; ++i) s.p[i] = 0.5 + i;
    for (size_t i = 0; i < sizeof(s.buie) / 8; ++i) s.buie[i] = 1.0 + (double)i;
    return s;
}

static void descriptors() {
    char msg[512];
    const trc_table_facts sun = {37, 0.0123, 0.875, 0, 1, 0x7f12345678ull}, emit = {9, 1.5, 2.25, 2, 1, 0x7f00000100ull};
    const int kinds[4] = {TRC_SRC_SUNSHAPE_DISK, TRC_SRC_SUNSHAPE_RECT, TRC_SRC_ARC_VOLUME, TRC_SRC_EMIT_THERMAL};
    for (int kind : kinds) {
        const bool thermal = kind == TRC_SRC_EMIT_THERMAL;
        const trc_table_facts &t = thermal ? emit : sun;
        trc_source_desc s = desc_of(kind), out;
        if (thermal) { s.p[0] = TRC_THERMAL_FRUSTUM; s.p[1] = 1.0; s.p[2] = 2.0; }
        std::memset(&out, 0xAB, sizeof(out));
        EXPECT(trc_source_with_table(s, &t, 1, "who", out, msg, sizeof(msg)) == TRC_OK, "kind %d: '%s'", kind, msg);
        trc_source_desc want = s;
        if (!thermal) { want.p[TRC_SUNSHAPE_P_THETA_C] = t.theta_c; want.p[TRC_SUNSHAPE_P_U_C] = t.u_c; }
        want.p[TRC_SUNSHAPE_P_N] = (double)t.n;
        std::memset(want.buie, 0, sizeof(want.buie));
        std::memcpy(&want.buie[0], &t.address, 8);
        EXPECT(std::memcmp(&out, &want, sizeof(out)) == 0, "kind %d: the resolved descriptor differs", kind);
        uint64_t a = 0;
        std::memcpy(&a, &out.buie[0], 8);
        bool rest_zero = true;
        for (size_t i = 1; i < sizeof(out.buie) / 8; ++i) rest_zero = rest_zero && out.buie[i] == 0.0;
        EXPECT(a == t.address && rest_zero && out.p[TRC_SUNSHAPE_P_N] == (double)t.n, "kind %d: address %llx, n %g", kind, (unsigned long long)a, out.p[TRC_SUNSHAPE_P_N]);
        if (thermal) EXPECT(out.p[0] == s.p[0] && out.p[1] == s.p[1] && out.p[2] == s.p[2] && out.p[5] == s.p[5] && out.p[6] == s.p[6], "a thermal emitter's p[] changed");
        EXPECT(trc_source_with_table(s, &t, -1, "who", out, msg, sizeof(msg)) == TRC_OK, "kind %d without a device: '%s'", kind, msg);
        EXPECT(trc_source_with_table(s, nullptr, 1, "who", out, msg, sizeof(msg)) == TRC_ERR_INVALID &&
               !std::strcmp(msg, "who: the source names sunshape table 5, which does not exist (destroyed?)"), "kind %d: '%s'", kind, msg);
        EXPECT(trc_source_with_table(s, &t, 0, "who", out, msg, sizeof(msg)) == TRC_ERR_INVALID && !std::strcmp(msg, "who: sunshape table 5 lives on another device"),
               "kind %d: '%s'", kind, msg);
    }
    // a kind that names no table is handed back as it is, whatever the table
    trc_source_desc s = desc_of(TRC_SRC_PILLBOX_DISK), out;
    std::memset(&out, 0xAB, sizeof(out));
    EXPECT(trc_source_with_table(s, nullptr, 3, "who", out, msg, sizeof(msg)) == TRC_OK && std::memcmp(&out, &s, sizeof(s)) == 0, "a pillbox changed: '%s'", msg);
    // the thermal emitter's own refusals
    struct { double p0, p1, p2; const trc_table_facts *t; const char *says; } bad_thermal[] = {
        {TRC_THERMAL_DISK, 1., 2., &sun, "who: table 5 is not an emittance table (trc_emittance_table_create)"},
        {6., 1., 2., &emit, "who: a thermal emitter has no shape 6"},
        {-1., 1., 2., &emit, "who: a thermal emitter has no shape -1"},
        {2.5, 1., 2., &emit, "who: a thermal emitter has no shape 2.5"},
        {NAN, 1., 2., &emit, "who: a thermal emitter has no shape nan"},
        {TRC_THERMAL_FRUSTUM, 1.5, 1.5, &emit, "who: a thermal frustum needs r0 != r1 (use the cylinder)"}};
    for (auto &b : bad_thermal) {
        trc_source_desc th = desc_of(TRC_SRC_EMIT_THERMAL);
        th.p[0] = b.p0; th.p[1] = b.p1; th.p[2] = b.p2;
        EXPECT(trc_source_with_table(th, b.t, 1, "who", out, msg, sizeof(msg)) == TRC_ERR_INVALID && !std::strcmp(msg, b.says), "'%s', expected '%s'", msg, b.says);
    }
}

int main() {
    for (int kind = 0; kind < K_COUNT; ++kind) {
        refusals(kind);
        accepted(kind, 2);
        accepted(kind, MAX_N[kind]);
    }
    spectrum_kinds();
    registry();
    registry_threads();
    descriptors();
    std::printf("source_check: %d checks, %d violations\n", checks, bad);
    return bad ? 1 : 0;
}
#endif
