// trc_source_host.h -- the host side of the tabulated sources, free of HIP: the one check of a caller's table (sunshape, polar table
// of an arc lamp, source spectrum), the check-and-pack functions of every table kind, the registry that gives tables their ids, and
// the arithmetic that turns a descriptor naming a table into the one the kernels read.  The library (trc_protocol.hip) and the host
// checks (tests/sourcecheck) read the same functions.  A refusal is a status returned with its reason in msg (trc_refuse).
#ifndef TRC_SOURCE_HOST_H
#define TRC_SOURCE_HOST_H

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>
#include "trc_core.h"
#include "trc_scene_host.h"

// the nouns of a table kind's refusals: "<who>: <table> has 1 points", "<who>: <missing>", "<who>: <x> 3 is not finite",
// "<who>: <xs> are not strictly increasing", "<who>: <y> 3 is negative or not finite", "<who>: <xs> must lie in <domain>"
struct trc_table_words { const char *table, *missing, *x, *xs, *y, *domain; };

static const trc_table_words TRC_WORDS_SUNSHAPE = {"the table", "angles or intensities missing", "angle", "angles", "intensity", "[0, pi/2)"};
static const trc_table_words TRC_WORDS_ANGLE = {"the table", "angles or densities missing", "angle", "angles", "density", "[0, pi]"};
static const trc_table_words TRC_WORDS_SPECTRUM = {"spectrum table", "spectrum table without wavelengths or values", "spectrum wavelength",
                                                   "spectrum wavelengths", "spectrum value", nullptr};

// A caller's table of n points (x[i], y[i]) for `who`: 2..max_n points, both arrays there, x finite and strictly increasing, y finite
// and not negative; and, for a kind with a domain (w.domain), x[0] >= 0 and x[n-1] <= hi (closed) or < hi.
static inline int trc_table_check(const char *who, int n, int max_n, const double *x, const double *y, const trc_table_words &w,
                                  double hi, bool closed, char *msg, size_t len) {
    if (n < 2 || n > max_n) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: %s has %d points, 2..%d allowed", who, w.table, n, max_n);
    if (!x || !y) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: %s", who, w.missing);
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(x[i])) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: %s %d is not finite", who, w.x, i);
        if (i > 0 && !(x[i] > x[i - 1]))
            return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: %s are not strictly increasing (point %d)", who, w.xs, i);
        if (!std::isfinite(y[i]) || y[i] < 0.0) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: %s %d is negative or not finite", who, w.y, i);
    }
    if (w.domain && (!(x[0] >= 0.0) || !(closed ? x[n - 1] <= hi : x[n - 1] < hi)))
        return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: %s must lie in %s", who, w.xs, w.domain);
    return TRC_OK;
}

// A table checked and packed for the device: n points as x | y | cdf (the layout of its kind's sampler: trc_core.h), the two numbers
// a descriptor brings the kernels beside it, and which create function packed it: 0 trc_sunshape_create, 1 trc_angle_table_create,
// 2 trc_emittance_table_create
struct trc_table_packed {
    int32_t n = 0;
    std::vector<double> tab;
    double theta_c = 0.0, u_c = 0.0;
    int packing = 0;
};

// a tabulated sunshape (trc_sunshape_create's errors; trc_sunshape_pack)
static inline int trc_sunshape_make(int32_t n, const double *angle, const double *intensity, trc_table_packed &t, char *msg, size_t len) {
    const char *who = "trc_sunshape_create";
    if (const int st = trc_table_check(who, n, TRC_SUNSHAPE_MAX_POINTS, angle, intensity, TRC_WORDS_SUNSHAPE, TRC_PI / 2.0, false, msg, len)) return st;
    t.n = n; t.packing = 0;
    t.tab.assign((size_t)3 * n, 0.0);
    if (!trc_sunshape_pack(n, angle, intensity, t.tab.data(), &t.theta_c, &t.u_c)) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: the table has no mass", who);
    return TRC_OK;
}

// the polar table of an arc lamp, packed as a source spectrum's table (trc_angle_table_pack)
static inline int trc_angle_table_make(int32_t n, const double *angle, const double *density, trc_table_packed &t, char *msg, size_t len) {
    const char *who = "trc_angle_table_create";
    if (const int st = trc_table_check(who, n, TRC_SUNSHAPE_MAX_POINTS, angle, density, TRC_WORDS_ANGLE, TRC_PI, true, msg, len)) return st;
    t.n = n; t.packing = 1;
    t.tab.assign((size_t)3 * n, 0.0);
    if (!trc_angle_table_pack(n, angle, density, t.tab.data())) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: the table has no mass", who);
    t.theta_c = angle[n - 1]; t.u_c = 1.0;
    return TRC_OK;
}

// the emittance table of a thermal emitter (trc_emittance_table_fault; trc_emittance_pack)
static inline int trc_emittance_table_make(int32_t n, const double *theta, const double *eps, trc_table_packed &t, char *msg, size_t len) {
    const char *who = "trc_emittance_table_create";
    if (const char *fault = trc_emittance_table_fault(n, theta, eps)) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: %s", who, fault);
    t.n = n; t.packing = 2;
    t.tab.assign((size_t)3 * n, 0.0);
    double mass = 0.0;
    if (!trc_emittance_pack(n, theta, eps, t.tab.data(), &mass)) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: the table has no mass", who);
    t.theta_c = t.tab[n - 1]; t.u_c = mass;
    return TRC_OK;
}

// A spectrum checked and packed for the device: wl | density normalised to a unit trapezoid integral | its running integral
// (float64 on the host; the last entry of the CDF is 1 exactly, so every u in [0, 1) finds an interval of positive mass).
// A constant spectrum has no table: tab is left empty.
static inline int trc_spectrum_make(const trc_source_spectrum *sp, const char *who, std::vector<double> &tab, char *msg, size_t len) {
    tab.clear();
    if (sp->kind != TRC_SPECTRUM_CONSTANT && sp->kind != TRC_SPECTRUM_TABLE && sp->kind != TRC_SPECTRUM_CARRIED)
        return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: spectrum kind %d is neither CONSTANT nor TABLE nor CARRIED", who, sp->kind);
    if (!std::isfinite(sp->ref_index) || !(sp->ref_index > 0.0))
        return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: spectrum ref_index must be finite and positive", who);
    if (sp->kind == TRC_SPECTRUM_CONSTANT) {
        if (!std::isfinite(sp->wavelength)) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: spectrum wavelength is not finite", who);
        return TRC_OK;
    }
    const int n = sp->n;
    if (const int st = trc_table_check(who, n, TRC_SPECTRUM_MAX_POINTS, sp->wl, sp->value, TRC_WORDS_SPECTRUM, 0.0, false, msg, len)) return st;
    tab.assign((size_t)3 * n, 0.0);
    double *w = tab.data(), *v = w + n, *c = v + n;
    double cum = 0.0;
    for (int i = 0; i < n; ++i) {
        w[i] = sp->wl[i];
        if (i > 0) cum += (sp->wl[i] - sp->wl[i - 1]) * (sp->value[i] + sp->value[i - 1]) / 2.;
        c[i] = cum;
    }
    if (!(cum > 0.0) || !std::isfinite(cum)) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: spectrum table has a zero (or non-finite) integral", who);
    for (int i = 0; i < n; ++i) { v[i] = sp->value[i] / cum; c[i] = c[i] / cum; }
    return TRC_OK;
}

// Every live table by id, under one mutex.  Ids count up from `first` and are never reused, so that a descriptor (and the footprint
// map cached from it) always means the same table; INT32_MAX is never given out.
template <class T>
class trc_id_registry {
    std::mutex mu_;
    std::unordered_map<int32_t, T> live_;
    int32_t next_;
public:
    explicit trc_id_registry(int32_t first = 1) : next_(first) {}
    // v is kept under a new id; TRC_ERR_CAPACITY, and nothing kept, when the ids are exhausted
    int add(const T &v, int32_t *id) {
        std::lock_guard<std::mutex> lk(mu_);
        if (next_ == INT32_MAX) return TRC_ERR_CAPACITY;
        *id = next_++;
        live_[*id] = v;
        return TRC_OK;
    }
    // use(the entry of id), called under the mutex; false: there is none
    template <class F>
    bool find(int32_t id, F use) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = live_.find(id);
        if (it == live_.end()) return false;
        use(it->second);
        return true;
    }
    void erase(int32_t id) {
        std::lock_guard<std::mutex> lk(mu_);
        live_.erase(id);
    }
    size_t size() {
        std::lock_guard<std::mutex> lk(mu_);
        return live_.size();
    }
};

// the kinds whose descriptor names a table: the tabulated sunshapes, the arc volume with its polar table and the thermal emitter with
// its emittance table
static inline bool trc_source_is_sunshape(int kind) {
    return kind == TRC_SRC_SUNSHAPE_DISK || kind == TRC_SRC_SUNSHAPE_RECT || kind == TRC_SRC_ARC_VOLUME || kind == TRC_SRC_EMIT_THERMAL;
}

// what a descriptor takes from the table it names
struct trc_table_facts {
    int32_t n;
    double theta_c, u_c;
    int packing;
    int device;             // the GPU the table lives on
    uint64_t address;       // ... and where
};

// A descriptor that names a table as the kernels read it: out = src with theta_c, u_c, n in p[] and the table's device address in
// buie[0], the rest of buie zero.  t NULL: the registry holds no table src.table; device < 0: any device will do.  A descriptor of
// another kind is copied as it is.
static inline int trc_source_with_table(const trc_source_desc &src, const trc_table_facts *t, int device, const char *who, trc_source_desc &out,
                                        char *msg, size_t len) {
    if (!trc_source_is_sunshape(src.kind)) { out = src; return TRC_OK; }
    if (!t) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: the source names sunshape table %d, which does not exist (destroyed?)", who, src.table);
    if (device >= 0 && t->device != device) return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: sunshape table %d lives on another device", who, src.table);
    if (src.kind == TRC_SRC_EMIT_THERMAL) {       // (the one kind that checks the packing: its sampler solves another equation)
        if (t->packing != 2)
            return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: table %d is not an emittance table (trc_emittance_table_create)", who, src.table);
        if (!(src.p[0] >= TRC_THERMAL_DISK && src.p[0] <= TRC_THERMAL_SPHERE) || (double)(int)src.p[0] != src.p[0])      // (in range before it is cast)
            return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: a thermal emitter has no shape %g", who, src.p[0]);
        if ((int)src.p[0] == TRC_THERMAL_FRUSTUM && src.p[1] == src.p[2])
            return trc_refuse(msg, len, TRC_ERR_INVALID, "%s: a thermal frustum needs r0 != r1 (use the cylinder)", who);
    }
    out = src;
    if (src.kind != TRC_SRC_EMIT_THERMAL) {        // (a thermal emitter keeps its shape parameters and its sign there)
        out.p[TRC_SUNSHAPE_P_THETA_C] = t->theta_c;
        out.p[TRC_SUNSHAPE_P_U_C] = t->u_c;
    }
    out.p[TRC_SUNSHAPE_P_N] = (double)t->n;
    memset(out.buie, 0, sizeof(out.buie));
    memcpy(&out.buie[0], &t->address, sizeof(double));
    return TRC_OK;
}

#endif
