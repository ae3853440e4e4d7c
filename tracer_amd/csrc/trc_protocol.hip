// trc_protocol.hip -- every entry point of include/tracer_amd.h that takes a context and no scene, and their kernels:
//   * the tabulated source tables (trc_sunshape_*, trc_angle_table_create, trc_emittance_table_create): checked and packed by
//     trc_source_host.h, uploaded once, named by descriptors through their id;
//   * source generation into a bundle (trc_source_start32, trc_source_generate, trc_source_generate_x);
//   * the reference's per-object protocol (trc_kdtree_traversal, trc_gm_*, trc_optics_*).
// The engines (trc_kernels.hip) call the few functions of this unit that trc_host.h declares.

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include <hip/hip_runtime.h>

#include "trc_core.h"
#include "trc_bounds.h"
#include "trc_footprint.h"
#include "trc_device.h"
#include "trc_scene_host.h"
#include "trc_host.h"
#include "trc_source_host.h"

// a status of trc_source_host.h as the library reports it: the reason of a refusal becomes the thread's error string
static int refused(int st, const char *msg) { return st == TRC_OK ? TRC_OK : trc_fail(st, "%s", msg); }

// ================================================================================================
// source generation as a bundle (sources.*_bundle)
// ================================================================================================
template <bool THERMAL>
__device__ __forceinline__ void source_generate_body(const trc_source_desc *src, long long n, unsigned long long seed, unsigned long long offset,
                                                     double *x, double *y, double *z, double *dx, double *dy, double *dz, double *e,
                                                     uint64_t *rid, double *l_buie) {
    for (int i = threadIdx.x; i < TRC_BUIE_TABLE; i += blockDim.x) l_buie[i] = src->buie[i];
    if (threadIdx.x == 0 && (src->kind == TRC_SRC_BUIE_DISK || src->kind == TRC_SRC_BUIE_RECT)) trc_buie_aureole_consts(src->buie, l_buie + TRC_BUIE_TABLE);
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        unsigned long long r = offset + (unsigned long long)i;
        double px, py, pz, qx, qy, qz;
        trc_source_ray<THERMAL>(src, l_buie, l_buie + TRC_BUIE_TABLE, seed, r, &px, &py, &pz, &qx, &qy, &qz);
        x[i] = px; y[i] = py; z[i] = pz;
        dx[i] = qx; dy[i] = qy; dz[i] = qz;
        e[i] = src->energy;
        if (rid) rid[i] = r;
    }
}

// every kind but the thermal emitter ...
__global__ __launch_bounds__(256) void k_source_generate(const trc_source_desc *src, long long n,
                                                         unsigned long long seed, unsigned long long offset,
                                                         double *x, double *y, double *z, double *dx, double *dy,
                                                         double *dz, double *e, uint64_t *rid) {
    __shared__ double l_buie[TRC_BUIE_STAGED];
    source_generate_body<false>(src, n, seed, offset, x, y, z, dx, dy, dz, e, rid, l_buie);
}

// ... and the thermal emitter (TRC_SRC_EMIT_THERMAL), whose sampler would cost the kernel above two waves of occupancy
__global__ __launch_bounds__(256) void k_source_generate_emit(const trc_source_desc *src, long long n,
                                                              unsigned long long seed, unsigned long long offset,
                                                              double *x, double *y, double *z, double *dx, double *dy,
                                                              double *dz, double *e, uint64_t *rid) {
    __shared__ double l_buie[TRC_BUIE_STAGED];
    source_generate_body<true>(src, n, seed, offset, x, y, z, dx, dy, dz, e, rid, l_buie);
}

// the generation kernel of a descriptor's kind (host: src is the caller's copy)
static auto source_generate_kernel(const trc_source_desc *src) -> decltype(&k_source_generate) {
    return src->kind == TRC_SRC_EMIT_THERMAL ? k_source_generate_emit : k_source_generate;
}

// float32 start points as k_s_cull evaluates them (trc_source_start32)
__global__ __launch_bounds__(256) void k_source_start32(trc_fp_params F, long long n, unsigned long long seed, unsigned long long offset,
                                                        float *lx, float *ly) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long rid = offset + (unsigned long long)i;
        uint32_t o[4];
        trc_philox4x32_10((uint32_t)rid, (uint32_t)(rid >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
        float x, y;
        trc_fp_position32(F, o, &x, &y);
        lx[i] = x; ly[i] = y;
    }
}

// ================================================================================================
// per-surface protocol kernels
// ================================================================================================
__global__ __launch_bounds__(256) void k_gm_intersect(const double *rec, const double *extra, long long n,
                                                      const double *x, const double *y, const double *z,
                                                      const double *dx, const double *dy, const double *dz,
                                                      double *t_out, double *hx, double *hy, double *hz) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double t = trc_intersect(rec, extra, x[i], y[i], z[i], dx[i], dy[i], dz[i]);
    t_out[i] = t;
    if (hx) {
        // FiniteFlatGM / QuadricGM keep v + t*d for every ray (flat_surface.py:156, quadric.py:101)
        hx[i] = x[i] + t * dx[i]; hy[i] = y[i] + t * dy[i]; hz[i] = z[i] + t * dz[i];
    }
}

__global__ __launch_bounds__(256) void k_gm_normals(const double *rec, long long n, const double *hx,
                                                    const double *hy, const double *hz, const double *dx,
                                                    const double *dy, const double *dz, double *nx, double *ny,
                                                    double *nz) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a, b, c;
    trc_normal(rec, hx[i], hy[i], hz[i], dx[i], dy[i], dz[i], &a, &b, &c);
    nx[i] = a; ny[i] = b; nz[i] = c;
}

struct OpticsParams {
    const double *rec, *opt, *extra;
    long long n;
    const double *dx, *dy, *dz, *e, *ref, *wl;
    const uint64_t *rid;
    unsigned long long ray_offset;
    const double *path;             // distance from the ray origin to the hit (null: 0)
    const double *nx, *ny, *nz;
    unsigned long long seed;
    int event;
    double *odx, *ody, *odz, *oe, *oref;
    int32_t *oblk;  // 2n: -1 empty, else block id
    // complex indices, material rows, spectra (trc_shade_x): inputs with rows n apart, outputs 2n apart
    const double *ref_im, *mat, *spec_wl, *spec;
    int n_mat, W;
    double *o_im, *o_spec;
    double *oshift;     // 2n: how far along the oriented normal the outgoing ray starts from the hit point (PeriodicBoundary)
};

__global__ __launch_bounds__(256) void k_optics_apply(OpticsParams P) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    trc_ray_out out[2];
    unsigned long long rid = P.rid ? P.rid[i] : (P.ray_offset + (unsigned long long)i);
    const double path = P.path ? P.path[i] : 0.0;
    trc_ray_ext X;
    X.ref_im = P.ref_im ? P.ref_im[i] : 0.0;
    X.W = P.W; X.n_mat = P.n_mat; X.stride = P.n;
    X.mat = P.mat ? P.mat + i : nullptr;
    X.wl = P.spec_wl ? P.spec_wl + i : nullptr;
    X.spec = P.spec ? P.spec + i : nullptr;
    double out_im[2], poly_th;
    int n_out = trc_shade_x(trc_rec_opt_kind(P.rec), P.opt, P.extra, trc_rec_extra_off(P.rec),
                            trc_rec_extra_len(P.rec), P.rec[2], P.rec[5], P.rec[8], P.dx[i], P.dy[i], P.dz[i],
                            P.e[i], P.ref ? P.ref[i] : 1.0, P.wl ? P.wl[i] : 0.0, path, P.nx[i], P.ny[i], P.nz[i], P.seed,
                            rid, (uint32_t)P.event, X, out, out_im, &poly_th);
    for (int c = 0; c < 2; ++c) {
        long long slot = c == 0 ? i : P.n + i;
        if (c < n_out) {
            P.odx[slot] = out[c].dx; P.ody[slot] = out[c].dy; P.odz[slot] = out[c].dz;
            P.oe[slot] = out[c].e; P.oref[slot] = out[c].ref; P.oblk[slot] = out[c].blk;
            P.oshift[slot] = out[c].shift;
            if (P.o_im) P.o_im[slot] = out_im[c];
            if (P.o_spec) {
                const double *tab = P.extra + trc_rec_extra_off(P.rec);
                for (int w = 0; w < P.W; ++w) {
                    const double f = poly_th >= 0.0 ? 1.0 - trc_poly_absorptance(tab, poly_th, X.wl[(size_t)w * P.n]) : out[c].sf;
                    P.o_spec[(size_t)w * 2 * P.n + slot] = X.spec[(size_t)w * P.n] * f;
                }
            }
        } else {
            P.oblk[slot] = -1;
        }
    }
}

// ================================================================================================
// tabulated sunshapes (trc_sunshape): tables packed and uploaded once, named by descriptors through their id
// ================================================================================================
struct trc_sunshape {
    int device;                     // the GPU of the context it was made on
    int32_t id;
    trc_table_packed t;             // theta | g | cdf (trc_sunshape_theta layout), theta_c, u_c, and which create function packed it
    DevBuf<double> d_tab;
};

// every live table by id (trc_id_registry: ids count up and are never reused)
static trc_id_registry<trc_sunshape *> g_sun;

// the table `packed` (checked and packed for `who`) on the context's device and in the registry; `what` names it when the upload fails
static int table_create(trc_ctx *ctx, const char *who, const char *what, trc_table_packed &&packed, trc_sunshape **out) {
    std::unique_ptr<trc_sunshape> t(new (std::nothrow) trc_sunshape());
    if (!t) return trc_fail(TRC_ERR_NOMEM, "out of host memory");
    t->device = ctx->device;
    t->t = std::move(packed);
    HIP_TRY(hipSetDevice(ctx->device));
    char fail[64];
    snprintf(fail, sizeof(fail), "%s upload failed", what);
    TRC_TRY(dev_upload(t->d_tab, t->t.tab.data(), t->t.tab.size(), fail));
    if (g_sun.add(t.get(), &t->id) != TRC_OK) return trc_fail(TRC_ERR_CAPACITY, "%s: table ids exhausted", who);
    *out = t.release();
    return TRC_OK;
}

extern "C" int trc_sunshape_create(trc_ctx *ctx, int32_t n, const double *angle, const double *intensity, trc_sunshape **out) {
    if (!ctx || !out) return trc_fail(TRC_ERR_INVALID, "trc_sunshape_create: bad arguments");
    *out = nullptr;
    trc_table_packed t;
    char msg[512];
    TRC_TRY(refused(trc_sunshape_make(n, angle, intensity, t, msg, sizeof(msg)), msg));
    return table_create(ctx, "trc_sunshape_create", "sunshape", std::move(t), out);
}

// the polar table of an arc lamp (TRC_SRC_ARC_VOLUME): a trc_sunshape packed as a source spectrum's table (trc_angle_table_pack)
extern "C" int trc_angle_table_create(trc_ctx *ctx, int32_t n, const double *angle, const double *density, trc_sunshape **out) {
    if (!ctx || !out) return trc_fail(TRC_ERR_INVALID, "trc_angle_table_create: bad arguments");
    *out = nullptr;
    trc_table_packed t;
    char msg[512];
    TRC_TRY(refused(trc_angle_table_make(n, angle, density, t, msg, sizeof(msg)), msg));
    return table_create(ctx, "trc_angle_table_create", "angle table", std::move(t), out);
}

// the emittance table of a thermal emitter (TRC_SRC_EMIT_THERMAL): a trc_sunshape packed by trc_emittance_pack
extern "C" int trc_emittance_table_create(trc_ctx *ctx, int32_t n, const double *theta, const double *eps, trc_sunshape **out) {
    if (!ctx || !out) return trc_fail(TRC_ERR_INVALID, "trc_emittance_table_create: bad arguments");
    *out = nullptr;
    trc_table_packed t;
    char msg[512];
    TRC_TRY(refused(trc_emittance_table_make(n, theta, eps, t, msg, sizeof(msg)), msg));
    return table_create(ctx, "trc_emittance_table_create", "emittance table", std::move(t), out);
}

extern "C" int trc_sunshape_id(trc_sunshape *t, int32_t *id) {
    if (!t || !id) return trc_fail(TRC_ERR_INVALID, "trc_sunshape_id: bad arguments");
    *id = t->id;
    return TRC_OK;
}

extern "C" int trc_sunshape_get(trc_sunshape *t, int32_t *n, double *packed, double *theta_c, double *u_c) {
    if (!t) return trc_fail(TRC_ERR_INVALID, "trc_sunshape_get: table is NULL");
    if (n) *n = t->t.n;
    if (packed) memcpy(packed, t->t.tab.data(), t->t.tab.size() * sizeof(double));
    if (theta_c) *theta_c = t->t.theta_c;
    if (u_c) *u_c = t->t.u_c;
    return TRC_OK;
}

extern "C" int trc_sunshape_destroy(trc_sunshape *t) {
    if (!t) return TRC_OK;
    g_sun.erase(t->id);
    HIP_TRY(hipSetDevice(t->device));
    delete t;
    return TRC_OK;
}

int source_resolve(trc_ctx *ctx, const trc_source_desc *&src, trc_source_desc &tmp, const char *who) {
    if (!src || !trc_source_is_sunshape(src->kind)) return TRC_OK;
    trc_table_facts f;
    const bool found = g_sun.find(src->table, [&f](const trc_sunshape *t) {
        f = {t->t.n, t->t.theta_c, t->t.u_c, t->t.packing, t->device, (uint64_t)(uintptr_t)t->d_tab.get()};
    });
    char msg[512];
    TRC_TRY(refused(trc_source_with_table(*src, found ? &f : nullptr, ctx ? ctx->device : -1, who, tmp, msg, sizeof(msg)), msg));
    src = &tmp;
    return TRC_OK;
}

int source_kind_check(const trc_source_desc *src) {
    if (src->kind < TRC_SRC_PILLBOX_DISK || src->kind > TRC_SRC_EMIT_THERMAL)
        return trc_fail(TRC_ERR_UNSUPPORTED, "source kind %d is not in the native table", src->kind);
    return TRC_OK;
}

static int upload_source(const trc_source_desc *src, DevBuf<trc_source_desc> &d_src) {
    TRC_TRY(source_kind_check(src));
    return dev_upload(d_src, src, 1);
}

// ================================================================================================
// C-ABI: source generation
// ================================================================================================
extern "C" int trc_source_start32(trc_ctx *ctx, const trc_source_desc *src, int64_t n, uint64_t seed, uint64_t ray_offset,
                                  float *lx, float *ly, double *eps) {
    if (!ctx || !src || n < 0 || !lx || !ly) return trc_fail(TRC_ERR_INVALID, "trc_source_start32: bad arguments");
    trc_source_desc src_res;
    TRC_TRY(source_resolve(ctx, src, src_res, "trc_source_start32"));
    HIP_TRY(hipSetDevice(ctx->device));
    trc_fp_params F;
    double half = 0.0, theta_c = 0.0;
    const char *why = "";
    if (!trc_fp_source(*src, F, &half, &theta_c, &why)) return trc_fail(TRC_ERR_UNSUPPORTED, "no footprint map for this source: %s", why);
    if (eps) *eps = TRC_FP_EPS_REL * half;
    if (n == 0) return TRC_OK;
    DevBuf<float> d[2];
    TRC_TRY(d[0].alloc((size_t)n));
    TRC_TRY(d[1].alloc((size_t)n));
    TRC_TRY(launch_wait(ctx, "k_source_start32", k_source_start32, n, 8192, F, n, seed, ray_offset, d[0].get(), d[1].get()));
    TRC_TRY(dev_download(lx, d[0].get(), (size_t)n));
    return dev_download(ly, d[1].get(), (size_t)n);
}

int source_generate_start(trc_ctx *ctx, const trc_source_desc *src, DevBuf<trc_source_desc> &d_src, int64_t n, uint64_t seed,
                          uint64_t ray_offset, double *const col[7], uint64_t *rid) {
    TRC_TRY(upload_source(src, d_src));
    long long grid = (n + 255) / 256;
    if (grid > 8192) grid = 8192;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(source_generate_kernel(src), dim3((unsigned)grid), dim3(256), 0, ctx->stream, d_src.get(), (long long)n,
                       (unsigned long long)seed, (unsigned long long)ray_offset, col[0], col[1], col[2], col[3], col[4], col[5],
                       col[6], rid);
    return TRC_OK;
}

extern "C" int trc_source_generate(trc_ctx *ctx, const trc_source_desc *src, int64_t n, uint64_t seed,
                                   uint64_t ray_offset, trc_rays *out) {
    if (!ctx || !src || n < 0) return trc_fail(TRC_ERR_INVALID, "trc_source_generate: bad arguments");
    trc_source_desc src_res;
    TRC_TRY(source_resolve(ctx, src, src_res, "trc_source_generate"));
    TRC_TRY(check_rays(out, n, "trc_source_generate"));
    if (!out->e) return trc_fail(TRC_ERR_INVALID, "trc_source_generate: energy column required");
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return TRC_OK;
    // the kernel writes the caller's columns when they are on the device, else copies held in `own`
    double *host[7] = {out->x, out->y, out->z, out->dx, out->dy, out->dz, out->e};
    double *d[7];
    uint64_t *d_rid = out->rid;
    DevBuf<double> own[7];
    DevBuf<uint64_t> own_rid;
    for (int i = 0; i < 7; ++i) d[i] = host[i];
    if (!out->on_device) {
        for (int i = 0; i < 7; ++i) { TRC_TRY(own[i].alloc((size_t)n)); d[i] = own[i].get(); }
        if (out->rid) TRC_TRY(own_rid.alloc((size_t)n));
        d_rid = own_rid.get();
    }
    DevBuf<trc_source_desc> d_src;
    TRC_TRY(source_generate_start(ctx, src, d_src, n, seed, ray_offset, d, d_rid));
    hipError_t se = hipStreamSynchronize(ctx->stream);
    if (se != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "k_source_generate failed: %s", hipGetErrorString(se));
    if (!out->on_device) {
        for (int i = 0; i < 7; ++i) TRC_TRY(dev_download(host[i], d[i], (size_t)n));
        if (out->rid) TRC_TRY(dev_download(out->rid, d_rid, (size_t)n));
    }
    return TRC_OK;
}

// ================================================================================================
// source spectra (trc_source_spectrum): one wavelength per source ray, drawn from (seed, stream id)
// ================================================================================================
// wl[i], ref[i] of source rays offset + i: CONSTANT writes the constant, TABLE draws (trc_spectrum_draw; tab = wl | val | cdf)
__global__ __launch_bounds__(256) void k_source_spectrum(const double *tab, int n_tab, int kind, double wl_const, double ref_index,
                                                         long long n, unsigned long long seed, unsigned long long offset,
                                                         double *wl, double *ref) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (wl) wl[i] = kind == TRC_SPECTRUM_TABLE ? trc_spectrum_draw(tab, tab + n_tab, tab + 2 * n_tab, n_tab, seed, offset + (unsigned long long)i)
                                                   : wl_const;
        if (ref) ref[i] = ref_index;
    }
}

// A carried spectrum (TRC_SPECTRUM_CARRIED): every ray i brings all n_tab points -- sample w at [w * stride + i]: the grid's
// wavelength, and e[i] * val[w], whose trapezoid integral is the ray's energy (tab = wl | val | cdf)
__global__ __launch_bounds__(256) void k_source_carried(const double *tab, int n_tab, long long n, long long stride, const double *e,
                                                        double *spec_wl, double *spectra) {
    const long long total = (long long)n_tab * n;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
        const long long w = k / n, i = k - w * n;
        if (spec_wl) spec_wl[w * stride + i] = tab[w];
        if (spectra) spectra[w * stride + i] = e[i] * tab[n_tab + w];
    }
}

int source_spectrum_make(const trc_source_spectrum *spec, const trc_rays *in, const trc_source_desc *src, const char *who, SourceSpectrum *out) {
    if (!spectrum_given(spec)) return TRC_OK;
    if (in) return trc_fail(TRC_ERR_INVALID, "%s: a spectrum belongs to a source descriptor, not to a given bundle", who);
    if (!src) return trc_fail(TRC_ERR_INVALID, "%s: a spectrum needs a source descriptor", who);
    char msg[512];
    TRC_TRY(refused(trc_spectrum_make(spec, who, out->tab, msg, sizeof(msg)), msg));
    out->desc = spec;
    return TRC_OK;
}

int spectrum_fill(trc_ctx *ctx, const trc_source_spectrum *sp, const std::vector<double> &tab, int64_t n, uint64_t seed,
                  uint64_t ray_offset, double *wl, double *ref) {
    if (n == 0 || (!wl && !ref)) return TRC_OK;
    DevBuf<double> d_tab;
    const int n_tab = sp->kind == TRC_SPECTRUM_TABLE ? sp->n : 0;
    if (n_tab) TRC_TRY(dev_upload(d_tab, tab.data(), tab.size(), "spectrum upload failed"));
    // (a carried spectrum: no wavelength is drawn, the rays' scalar wavelength is 0 as for a given polychromatic bundle)
    return launch_wait(ctx, "k_source_spectrum", k_source_spectrum, n, 8192, d_tab.get(), n_tab, sp->kind,
                       spectrum_carried(sp) ? 0.0 : sp->wavelength, sp->ref_index, n, seed, ray_offset, wl, ref);
}

int carried_fill(trc_ctx *ctx, const trc_source_spectrum *sp, const std::vector<double> &tab, int64_t n, int64_t stride, const double *e,
                 double *spec_wl, double *spectra) {
    if (n == 0 || (!spec_wl && !spectra)) return TRC_OK;
    DevBuf<double> d_tab;
    TRC_TRY(dev_upload(d_tab, tab.data(), tab.size(), "spectrum upload failed"));
    return launch_wait(ctx, "k_source_carried", k_source_carried, (long long)sp->n * n, 8192, d_tab.get(), sp->n, n, stride, e, spec_wl, spectra);
}

extern "C" int trc_source_generate_x(trc_ctx *ctx, const trc_source_desc *src, const trc_source_spectrum *spec, int64_t n,
                                     uint64_t seed, uint64_t ray_offset, trc_rays *out) {
    if (!spectrum_given(spec)) return trc_source_generate(ctx, src, n, seed, ray_offset, out);
    if (!ctx || !src || n < 0) return trc_fail(TRC_ERR_INVALID, "trc_source_generate_x: bad arguments");
    std::vector<double> tab;
    char msg[512];
    TRC_TRY(refused(trc_spectrum_make(spec, "trc_source_generate_x", tab, msg, sizeof(msg)), msg));
    if (spectrum_carried(spec) && (!out || !out->spec_wl || !out->spectra || out->n_spec != spec->n))
        return trc_fail(TRC_ERR_INVALID, "trc_source_generate_x: a carried spectrum of %d points fills out->spec_wl and out->spectra, which need n_spec == %d",
                        spec->n, spec->n);
    TRC_TRY(trc_source_generate(ctx, src, n, seed, ray_offset, out));
    if (spectrum_carried(spec) && n > 0) {
        if (out->on_device) TRC_TRY(carried_fill(ctx, spec, tab, n, out->n, out->e, out->spec_wl, out->spectra));
        else {
            DevBuf<double> d_e, d_x[2];
            TRC_TRY(dev_upload(d_e, out->e, (size_t)n, "energy upload failed"));
            for (auto &b : d_x) TRC_TRY(b.alloc((size_t)spec->n * (size_t)n));
            TRC_TRY(carried_fill(ctx, spec, tab, n, n, d_e.get(), d_x[0].get(), d_x[1].get()));
            double *host[2] = {out->spec_wl, out->spectra};
            for (int i = 0; i < 2; ++i)
                HIP_TRY(hipMemcpy2D(host[i], (size_t)out->n * 8, d_x[i].get(), (size_t)n * 8, (size_t)n * 8, (size_t)spec->n, hipMemcpyDeviceToHost));
        }
    }
    if (n == 0 || (!out->wavelength && !out->ref_index)) return TRC_OK;
    if (out->on_device) return spectrum_fill(ctx, spec, tab, n, seed, ray_offset, out->wavelength, out->ref_index);
    DevBuf<double> d[2];
    double *host[2] = {out->wavelength, out->ref_index};
    for (int i = 0; i < 2; ++i) if (host[i]) TRC_TRY(d[i].alloc((size_t)n));
    TRC_TRY(spectrum_fill(ctx, spec, tab, n, seed, ray_offset, d[0].get(), d[1].get()));
    for (int i = 0; i < 2; ++i) if (host[i]) TRC_TRY(dev_download(host[i], d[i].get(), (size_t)n));
    return TRC_OK;
}

// ================================================================================================
// C-ABI: KdTree.traversal on its own (accel_tree.py:213-312)
// ================================================================================================
struct KdTravParams {
    const int32_t *flag, *child, *leaf_off, *leaf_cnt, *leaf_surfs;
    const double *split;
    double lo[3], hi[3];
    const double *x, *y, *z, *dx, *dy, *dz;
    long long n;
    uint8_t *rel;       // n_surf rows of n bytes
    int *flags;         // [0]: some ray meets the root box; [1]: a ray needed more than KD_TRAV_STACK pending nodes
};

#define KD_TRAV_STACK 64

// numpy's maximum / minimum hand a nan on (intersect_bounds :325-326)
__device__ inline double np_maximum(double a, double b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }
__device__ inline double np_minimum(double a, double b) { return (a != a || b != b) ? NAN : (a < b ? a : b); }

__global__ __launch_bounds__(256) void k_kd_traversal(KdTravParams P) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.n) return;
    const double pos[3] = {P.x[r], P.y[r], P.z[r]}, dir[3] = {P.dx[r], P.dy[r], P.dz[r]};
    const double inv[3] = {1.0 / dir[0], 1.0 / dir[1], 1.0 / dir[2]};     // :224
    double t_lo = 0.0, t_hi = INFINITY;                                     // intersect_bounds :314-330
    for (int i = 0; i < 3; ++i) {
        const bool neg = dir[i] < 0.0;
        double a = ((neg ? P.hi[i] : P.lo[i]) - pos[i]) * inv[i];
        double b = ((neg ? P.lo[i] : P.hi[i]) - pos[i]) * inv[i];
        if (a > b) { const double t = a; a = b; b = t; }
        t_lo = np_maximum(t_lo, a);
        t_hi = np_minimum(t_hi, b);
    }
    if (!(t_hi > 0.0) || (t_lo > t_hi)) return;
    P.flags[0] = 1;
    int node = 0, top = 0;
    int st_node[KD_TRAV_STACK];
    double st_min[KD_TRAV_STACK], st_max[KD_TRAV_STACK];
    double t_min = t_lo, t_max = t_hi;
    while (true) {
        if (t_hi < t_min) break;                                            // :243 (the root's exit against the current entry)
        const int f = P.flag[node];
        if (f != 3) {
            const double sp = P.split[node];
            const double t_plane = (sp - pos[f]) * inv[f];                  // :249
            int c1 = P.child[node], c2 = c1 + 1;
            const bool below_first = (pos[f] < sp) || (pos[f] == sp && dir[f] <= 0.0);
            if (!below_first) { const int t = c1; c1 = c2; c2 = t; }
            if (t_plane > t_max || t_plane <= 0.0) node = c1;               // :258-259
            else if (t_plane < t_min) node = c2;
            else {
                if (top >= KD_TRAV_STACK) { P.flags[1] = 1; return; }
                st_node[top] = c2; st_min[top] = t_plane; st_max[top] = t_max;
                ++top;
                node = c1;
                t_max = t_plane;
            }
        } else {
            const int off = P.leaf_off[node], cnt = P.leaf_cnt[node];
            for (int k = 0; k < cnt; ++k) P.rel[(size_t)P.leaf_surfs[off + k] * P.n + r] = 1;       // :288
            if (top > 0) { --top; node = st_node[top]; t_min = st_min[top]; t_max = st_max[top]; }
            else break;
        }
    }
}

extern "C" int trc_kdtree_traversal(trc_ctx *ctx, const trc_kdtree_desc *kd, int32_t n_surf, const trc_rays *rays, int64_t n,
                                    uint8_t *relevancy, int32_t *any_inter) {
    if (!ctx || !kd || !relevancy || n_surf <= 0 || n < 0) return trc_fail(TRC_ERR_INVALID, "trc_kdtree_traversal: bad arguments");
    TRC_TRY(check_rays(rays, n, "trc_kdtree_traversal"));
    if (rays->on_device) return trc_fail(TRC_ERR_INVALID, "trc_kdtree_traversal: host bundle expected");
    char why[160];
    int depth = 0;      // (not refused here: a ray that runs out of stack raises the kernel's flag)
    const int st = trc_kd_check(kd, n_surf, &depth, why, sizeof(why));
    if (st != TRC_OK) return trc_fail(st, "trc_kdtree_traversal: %s", why);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<int32_t> d_i32[5];
    DevBuf<double> d_split, d_r[6];
    DevBuf<uint8_t> d_rel;
    DevBuf<int> d_flags;
    int any = 0;
    const int32_t *hs[5] = {kd->flag, kd->child, kd->leaf_off, kd->leaf_cnt, kd->leaf_surfs};
    const size_t cnt[5] = {(size_t)kd->n_nodes, (size_t)kd->n_nodes, (size_t)kd->n_nodes, (size_t)kd->n_nodes, (size_t)kd->n_leaf_surfs};
    for (int i = 0; i < 5; ++i) TRC_TRY(dev_upload(d_i32[i], hs[i], cnt[i], "memcpy failed"));
    TRC_TRY(dev_upload(d_split, kd->split, (size_t)kd->n_nodes, "memcpy failed"));
    TRC_TRY(d_flags.alloc(2));
    (void)hipMemset(d_flags.get(), 0, 8);
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    TRC_TRY(d_rel.alloc((size_t)n_surf * nn));
    (void)hipMemset(d_rel.get(), 0, (size_t)n_surf * nn);
    for (int i = 0; i < kd->n_always; ++i) (void)hipMemset(d_rel.get() + (size_t)kd->always_relevant[i] * nn, 1, nn);        // :236
    if (n > 0) {
        const double *src[6] = {rays->x, rays->y, rays->z, rays->dx, rays->dy, rays->dz};
        for (int i = 0; i < 6; ++i) TRC_TRY(dev_upload(d_r[i], src[i], (size_t)n, "memcpy failed"));
        KdTravParams P;
        P.flag = d_i32[0].get(); P.child = d_i32[1].get(); P.leaf_off = d_i32[2].get(); P.leaf_cnt = d_i32[3].get(); P.leaf_surfs = d_i32[4].get();
        P.split = d_split.get();
        for (int i = 0; i < 3; ++i) { P.lo[i] = kd->bounds[i]; P.hi[i] = kd->bounds[3 + i]; }
        P.x = d_r[0].get(); P.y = d_r[1].get(); P.z = d_r[2].get(); P.dx = d_r[3].get(); P.dy = d_r[4].get(); P.dz = d_r[5].get();
        P.n = n; P.rel = d_rel.get(); P.flags = d_flags.get();
        TRC_TRY(launch_wait(ctx, "k_kd_traversal", k_kd_traversal, n, 0, P));
        int fl[2] = {0, 0};
        TRC_TRY(dev_download(fl, d_flags.get(), 2));
        if (fl[1]) return trc_fail(TRC_ERR_CAPACITY, "a ray had more than %d pending nodes: the tree is deeper than the traversal's stack", KD_TRAV_STACK);
        any = fl[0];
        TRC_TRY(dev_download(relevancy, d_rel.get(), (size_t)n_surf * (size_t)n));
    }
    // `if inters.any() or self.always_relevant.any()` (:238): any() of the array of surface indices -- a non-zero index
    for (int i = 0; i < kd->n_always; ++i) if (kd->always_relevant[i] != 0) any = 1;
    if (any_inter) *any_inter = any;
    return TRC_OK;
}

// ================================================================================================
// C-ABI: per-surface protocol
// ================================================================================================
// one surface on the device: its record, its optics parameters (unless d_opt is NULL) and its extra values
static int upload_record(const trc_surface_desc *surf, int32_t n_extra, const double *extra, DevBuf<double> &d_rec, DevBuf<double> *d_opt,
                         DevBuf<double> &d_extra) {
    TRC_TRY(validate_surface(*surf, 0, n_extra));
    int stride = TRC_REC_HDR + 16;
    std::vector<double> rec(stride);
    trc_pack_record(*surf, rec.data(), stride);
    TRC_TRY(dev_upload(d_rec, rec.data(), (size_t)stride));
    if (d_opt) TRC_TRY(dev_upload(*d_opt, surf->opt, 8));
    TRC_TRY(d_extra.alloc((size_t)(n_extra > 0 ? n_extra : 1)));
    if (n_extra > 0 && extra) HIP_TRY(hipMemcpy(d_extra.get(), extra, (size_t)n_extra * sizeof(double), hipMemcpyHostToDevice));
    return TRC_OK;
}

extern "C" int trc_gm_find_intersections(trc_ctx *ctx, const trc_surface_desc *surf, int32_t n_extra, const double *extra,
                                         const trc_rays *rays, double *t_out, double *hx, double *hy, double *hz) {
    if (!ctx || !surf || !rays || !t_out) return trc_fail(TRC_ERR_INVALID, "trc_gm_find_intersections: bad arguments");
    if (rays->on_device) return trc_fail(TRC_ERR_INVALID, "host bundle expected");
    const int64_t n = rays->n;
    TRC_TRY(check_rays(rays, n, "trc_gm_find_intersections"));
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return TRC_OK;
    DevBuf<double> d_rec, d_extra, d_t, d_h[3];
    DevRays dr;
    TRC_TRY(upload_record(surf, n_extra, extra, d_rec, nullptr, d_extra));
    TRC_TRY(stage_rays(rays, n, false, &dr));
    TRC_TRY(d_t.alloc((size_t)n));
    const bool want_h = hx && hy && hz;
    if (want_h) for (auto &col : d_h) TRC_TRY(col.alloc((size_t)n));
    TRC_TRY(launch_wait(ctx, "k_gm_intersect", k_gm_intersect, n, 0, d_rec.get(), d_extra.get(), n, dr.x, dr.y, dr.z, dr.dx, dr.dy, dr.dz,
                        d_t.get(), d_h[0].get(), d_h[1].get(), d_h[2].get()));
    TRC_TRY(dev_download(t_out, d_t.get(), (size_t)n));
    if (want_h) {
        double *dst[3] = {hx, hy, hz};
        for (int i = 0; i < 3; ++i) TRC_TRY(dev_download(dst[i], d_h[i].get(), (size_t)n));
    }
    return TRC_OK;
}

extern "C" int trc_gm_get_normals(trc_ctx *ctx, const trc_surface_desc *surf, int64_t n, const double *hx, const double *hy,
                                  const double *hz, const double *dx, const double *dy, const double *dz, double *nx,
                                  double *ny, double *nz) {
    if (!ctx || !surf || n < 0) return trc_fail(TRC_ERR_INVALID, "trc_gm_get_normals: bad arguments");
    if (n == 0) return TRC_OK;
    if (!hx || !hy || !hz || !dx || !dy || !dz || !nx || !ny || !nz) return trc_fail(TRC_ERR_INVALID, "trc_gm_get_normals: NULL array");
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<double> d_rec, d_extra, d[9];
    const double *src[6] = {hx, hy, hz, dx, dy, dz};
    trc_surface_desc tmp = *surf;
    tmp.optics_kind = TRC_OPT_TRANSPARENT;   // normals do not depend on the optics
    if (tmp.gm_kind == TRC_GM_RECT_PERFORATED) { tmp.gm_kind = TRC_GM_RECT; }
    TRC_TRY(upload_record(&tmp, 0, nullptr, d_rec, nullptr, d_extra));
    for (auto &col : d) TRC_TRY(col.alloc((size_t)n));
    for (int i = 0; i < 6; ++i)
        if (hipMemcpy(d[i].get(), src[i], (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "memcpy failed");
    TRC_TRY(launch_wait(ctx, "k_gm_normals", k_gm_normals, n, 0, d_rec.get(), n, d[0].get(), d[1].get(), d[2].get(), d[3].get(), d[4].get(),
                        d[5].get(), d[6].get(), d[7].get(), d[8].get()));
    double *dst[3] = {nx, ny, nz};
    for (int i = 0; i < 3; ++i) TRC_TRY(dev_download(dst[i], d[6 + i].get(), (size_t)n));
    return TRC_OK;
}

__global__ __launch_bounds__(256) void k_fresnel_attenuating(long long n, double n1, const double *m_re, const double *m_im,
                                                             const double *th, double *rp, double *rs, double *t2) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) trc_fresnel_attenuating(th[i], n1, m_re[i], m_im[i], &rp[i], &rs[i], &t2[i]);
}

extern "C" int trc_optics_fresnel_attenuating(trc_ctx *ctx, int64_t n, double n1, const double *m_re, const double *m_im,
                                              const double *theta1, double *r_p, double *r_s, double *theta2) {
    if (!ctx || n < 0 || (n > 0 && (!m_re || !m_im || !theta1 || !r_p || !r_s || !theta2)))
        return trc_fail(TRC_ERR_INVALID, "trc_optics_fresnel_attenuating: bad arguments");
    if (n == 0) return TRC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<double> d[6];
    const double *src[3] = {m_re, m_im, theta1};
    double *dst[3] = {r_p, r_s, theta2};
    for (auto &col : d) TRC_TRY(col.alloc((size_t)n));
    for (int i = 0; i < 3; ++i)
        if (hipMemcpy(d[i].get(), src[i], (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "memcpy failed");
    TRC_TRY(launch_wait(ctx, "k_fresnel_attenuating", k_fresnel_attenuating, n, 0, n, n1, d[0].get(), d[1].get(), d[2].get(), d[3].get(),
                        d[4].get(), d[5].get()));
    for (int i = 0; i < 3; ++i) TRC_TRY(dev_download(dst[i], d[3 + i].get(), (size_t)n));
    return TRC_OK;
}

extern "C" int trc_optics_apply(trc_ctx *ctx, const trc_surface_desc *surf, int32_t n_extra, const double *extra,
                                const trc_rays *in, const double *hx, const double *hy, const double *hz, const double *nx,
                                const double *ny, const double *nz, uint64_t seed, int32_t bounce, trc_rays *out) {
    if (!ctx || !surf || !in || !out) return trc_fail(TRC_ERR_INVALID, "trc_optics_apply: bad arguments");
    if (in->on_device || out->on_device) return trc_fail(TRC_ERR_INVALID, "host bundles expected");
    const int64_t n = in->n;
    if (out->n < 2 * n) return trc_fail(TRC_ERR_CAPACITY, "output bundle must hold 2n rays");
    if (n == 0) { out->n = 0; return TRC_OK; }
    if (!in->dx || !in->dy || !in->dz || !in->e || !hx || !hy || !hz || !nx || !ny || !nz)
        return trc_fail(TRC_ERR_INVALID, "trc_optics_apply: directions, energies, hit points and normals are required");
    if (!out->x || !out->y || !out->z || !out->dx || !out->dy || !out->dz || !out->e || !out->parent)
        return trc_fail(TRC_ERR_INVALID, "trc_optics_apply: output needs x..e and parent");
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<double> d_rec, d_opt, d_extra;
    DevBuf<double> d_in[9];      // dx dy dz e ref wl nx ny nz
    DevBuf<uint64_t> d_rid;
    DevBuf<double> d_path;
    DevBuf<double> d_out[5];
    DevBuf<int32_t> d_blk;
    DevBuf<double> d_shift;
    // complex indices, material rows, spectra
    const int W = (in->spectra && in->spec_wl) ? in->n_spec : 0;
    const int n_mat = in->mat ? (int)in->n_mat : 0;
    if (W < 0 || W > 4096 || n_mat < 0 || n_mat > 64) return trc_fail(TRC_ERR_INVALID, "trc_optics_apply: n_spec or n_mat out of range");
    if (surf->optics_kind == TRC_OPT_LAMBERTIAN_POLYCHROMATIC && (W < 2 || !out->spectra))
        return trc_fail(TRC_ERR_INVALID, "polychromatic optics: the bundles need spectra (trc_rays.spectra, spec_wl)");
    if (surf->optics_kind == TRC_OPT_REFRACTIVE_MATERIAL && (!in->wavelength || n_mat <= std::max((int)surf->opt[4], (int)surf->opt[5]) || !out->ref_index_im))
        return trc_fail(TRC_ERR_INVALID, "refraction between tabulated materials: the bundle needs wavelengths and the materials' indices at them (trc_rays.mat), the output ref_index_im");
    if (W > 0 && out->spectra && out->n_spec != W) return trc_fail(TRC_ERR_INVALID, "trc_optics_apply: the output's n_spec differs from the input's");
    const int64_t out_cap = out->n;
    DevBuf<double> d_im, d_mat, d_swl, d_spec, d_oim, d_ospec;
    TRC_TRY(upload_record(surf, n_extra, extra, d_rec, &d_opt, d_extra));
    if (in->ref_index_im) TRC_TRY(dev_upload(d_im, in->ref_index_im, (size_t)n, "memcpy failed"));
    struct { const double *src; int rows; DevBuf<double> &dst; } blk2[3] = {{in->mat, 2 * n_mat, d_mat}, {in->spec_wl, W, d_swl}, {in->spectra, W, d_spec}};
    for (auto &b : blk2) {
        if (b.rows <= 0) continue;
        TRC_TRY(b.dst.alloc((size_t)n * b.rows));
        if (hipMemcpy2D(b.dst.get(), (size_t)n * 8, b.src, (size_t)in->n * 8, (size_t)n * 8, (size_t)b.rows, hipMemcpyHostToDevice) != hipSuccess)
            return trc_fail(TRC_ERR_DEVICE, "memcpy failed");
    }
    if (out->ref_index_im) TRC_TRY(d_oim.alloc((size_t)(2 * n)));
    if (W > 0 && out->spectra) TRC_TRY(d_ospec.alloc((size_t)(2 * n) * W));
    const double *src[9] = {in->dx, in->dy, in->dz, in->e, in->ref_index, in->wavelength, nx, ny, nz};
    for (int i = 0; i < 9; ++i)
        if (src[i]) TRC_TRY(dev_upload(d_in[i], src[i], (size_t)n, "memcpy failed"));
    if (in->x && in->y && in->z) {      // path lengths for the attenuating optics (Absorbant.attenuate, :874-877)
        std::vector<double> path((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            double ax = hx[i] - in->x[i], ay = hy[i] - in->y[i], az = hz[i] - in->z[i];
            path[(size_t)i] = std::sqrt(ax * ax + ay * ay + az * az);
        }
        TRC_TRY(dev_upload(d_path, path.data(), (size_t)n, "memcpy failed"));
    }
    if (in->rid) TRC_TRY(dev_upload(d_rid, in->rid, (size_t)n, "memcpy failed"));
    for (auto &col : d_out) TRC_TRY(col.alloc((size_t)(2 * n)));
    TRC_TRY(d_blk.alloc((size_t)(2 * n)));
    TRC_TRY(d_shift.alloc((size_t)(2 * n)));
    OpticsParams P;
    memset(&P, 0, sizeof(P));
    P.rec = d_rec.get(); P.opt = d_opt.get(); P.extra = d_extra.get(); P.n = n;
    P.dx = d_in[0].get(); P.dy = d_in[1].get(); P.dz = d_in[2].get(); P.e = d_in[3].get(); P.ref = d_in[4].get(); P.wl = d_in[5].get();
    P.rid = d_rid.get(); P.ray_offset = 0;
    P.nx = d_in[6].get(); P.ny = d_in[7].get(); P.nz = d_in[8].get(); P.path = d_path.get();
    P.seed = seed; P.event = bounce;
    P.odx = d_out[0].get(); P.ody = d_out[1].get(); P.odz = d_out[2].get(); P.oe = d_out[3].get(); P.oref = d_out[4].get();
    P.oblk = d_blk.get(); P.oshift = d_shift.get();
    P.ref_im = d_im.get(); P.mat = d_mat.get(); P.spec_wl = d_swl.get(); P.spec = d_spec.get(); P.n_mat = n_mat; P.W = W;
    P.o_im = d_oim.get(); P.o_spec = d_ospec.get();
    TRC_TRY(launch_wait(ctx, "k_optics_apply", k_optics_apply, n, 0, P));
    std::vector<double> h[5];
    std::vector<int32_t> blk((size_t)(2 * n));
    for (int i = 0; i < 5; ++i) {
        h[i].resize((size_t)(2 * n));
        TRC_TRY(dev_download(h[i].data(), d_out[i].get(), (size_t)(2 * n)));
    }
    TRC_TRY(dev_download(blk.data(), d_blk.get(), (size_t)(2 * n)));
    std::vector<double> h_shift((size_t)(2 * n));
    TRC_TRY(dev_download(h_shift.data(), d_shift.get(), (size_t)(2 * n)));
    std::vector<double> h_im, h_spec;
    if (d_oim) {
        h_im.resize((size_t)(2 * n));
        TRC_TRY(dev_download(h_im.data(), d_oim.get(), (size_t)(2 * n)));
    }
    if (d_ospec) {
        h_spec.resize((size_t)(2 * n) * W);
        TRC_TRY(dev_download(h_spec.data(), d_ospec.get(), h_spec.size()));
    }
    // reflected block first, then refracted block, each in selector order (optics_callables.py:852-857)
    int64_t m = 0;
    for (int b = 0; b < 2; ++b)
        for (int64_t slot = 0; slot < 2 * n; ++slot) {
            if (blk[(size_t)slot] != b) continue;
            int64_t i = slot < n ? slot : slot - n;
            const double sh = h_shift[(size_t)slot];        // (0 but for a periodic boundary: the ray goes on one period along the normal)
            out->x[m] = hx[i] + sh * nx[i]; out->y[m] = hy[i] + sh * ny[i]; out->z[m] = hz[i] + sh * nz[i];
            out->dx[m] = h[0][(size_t)slot]; out->dy[m] = h[1][(size_t)slot]; out->dz[m] = h[2][(size_t)slot];
            out->e[m] = h[3][(size_t)slot];
            if (out->ref_index) out->ref_index[m] = h[4][(size_t)slot];
            if (out->wavelength) out->wavelength[m] = in->wavelength ? in->wavelength[i] : 0.0;
            if (out->ref_index_im) out->ref_index_im[m] = h_im[(size_t)slot];
            if (d_ospec)
                for (int w = 0; w < W; ++w) {
                    out->spectra[(size_t)w * out_cap + m] = h_spec[(size_t)w * 2 * n + slot];
                    if (out->spec_wl) out->spec_wl[(size_t)w * out_cap + m] = in->spec_wl[(size_t)w * in->n + i];
                }
            out->parent[m] = i;
            ++m;
        }
    out->n = m;
    return TRC_OK;
}
