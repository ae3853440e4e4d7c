// trc_host.h -- the host plumbing the library's units share: the thread's error string and the macros that fill it, device memory
// behind the block cache and its owners, the context, a bundle's columns staged on the device, and the few functions of the
// scene-free unit (trc_protocol.hip) that the engines (trc_kernels.hip) call.  The scene itself is trc_scene.h, on top of this
// header.  The error string and the device block cache are one object each in the built library, whichever unit reaches them.
#ifndef TRC_HOST_H
#define TRC_HOST_H

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "trc_core.h"
#include "trc_pool.h"
#include "trc_scene_host.h"

// ================================================================================================
// error handling
// ================================================================================================
inline thread_local std::string g_last_error;      // what trc_last_error reads

static int trc_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return trc_fail(TRC_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),      \
                            __FILE__, __LINE__);                                                        \
    } while (0)

#define TRC_TRY(expr)                   \
    do {                                \
        int _s = (expr);                \
        if (_s != TRC_OK) return _s;    \
    } while (0)

// Device memory goes through a block cache (trc_pool.h: the policy and its reasons): a freed block of up to 128 MiB waits for the
// next request of its size class, a larger one for the next request of exactly its size, 2 GiB of each at most.  Keeping a block
// waits for the device as hipFree would have -- for the *current* device, as it always did, which need not be the block's own.
// TRC_DEV_POOL=0, read when the first block is asked for, turns the cache off.
struct DevBackend {
    static inline thread_local hipError_t err = hipSuccess;       // why this thread's last alloc() gave nothing
    void *alloc(size_t bytes) {
        void *p = nullptr;
        err = hipMalloc(&p, bytes);
        if (err == hipSuccess) return p;
        (void)hipGetLastError();      // (the failure is reported by err: it is not left for the next kernel launch to find)
        return nullptr;
    }
    void release(void *p) { (void)hipFree(p); }
    void quiesce() { (void)hipDeviceSynchronize(); }      // nothing in flight may still use the block when the next owner gets it
    int device() { int d = 0; (void)hipGetDevice(&d); return d; }
};
inline trc_block_cache<DevBackend> &dev_cache() {
    static const char *const e = getenv("TRC_DEV_POOL");
    static trc_block_cache<DevBackend> cache({(size_t)128 << 20, (size_t)2 << 30, (size_t)2 << 30, true, true}, !(e && e[0] == '0'));
    return cache;
}

template <class T>
static int dev_alloc(T **p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    *p = (T *)dev_cache().alloc(n * sizeof(T));
    if (!*p) return trc_fail(TRC_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(DevBackend::err));
    return TRC_OK;
}
template <class T>
static void dev_free(T *&p) {
    if (p) (void)dev_cache().free((void *)p);
    p = nullptr;
}

// Owner of one block of dev_alloc: freed when it is reset, replaced or goes out of scope.  Kernel parameter structs take get().
template <class T>
class DevBuf {
    T *p_ = nullptr;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~DevBuf() { reset(); }
    int alloc(size_t n) { reset(); return dev_alloc(&p_, n); }
    void reset() { dev_free(p_); }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// A DevBuf kept between calls that only grows.  reserve(n) leaves a buffer of n elements or more alone; a smaller one is replaced
// by a new one of n, contents not kept.  A reserve that fails leaves size() 0, so a buffer half grown claims nothing.
template <class T>
class GrowBuf {
    DevBuf<T> b_;
    size_t n_ = 0;
public:
    int reserve(size_t n) {
        if (n <= n_) return TRC_OK;
        n_ = 0;
        TRC_TRY(b_.alloc(n));
        n_ = n;
        return TRC_OK;
    }
    void reset() { b_.reset(); n_ = 0; }
    T *get() const { return b_.get(); }
    size_t size() const { return n_; }
};

// a new block of n elements for `b`, and the n elements of host `src` copied into it (nothing is copied for n == 0 or no src);
// a failed copy reports `fail` when given
template <class T>
static int dev_upload(DevBuf<T> &b, const T *src, size_t n, const char *fail = nullptr) {
    TRC_TRY(b.alloc(n));
    if (n == 0 || !src) return TRC_OK;
    if (fail) {
        if (hipMemcpy(b.get(), src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "%s", fail);
    } else HIP_TRY(hipMemcpy(b.get(), src, n * sizeof(T), hipMemcpyHostToDevice));
    return TRC_OK;
}

// n elements of device `src` to host `dst`
template <class T>
static int dev_download(T *dst, const T *src, size_t n) {
    if (hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "memcpy failed");
    return TRC_OK;
}

// Owner of a HIP handle that FREE releases -- a stream, an event, a pinned host block -- in the style of DevBuf.  own() takes a
// handle this object made and releases with FREE; borrow() takes somebody else's, which is only forgotten.
template <class H, auto FREE>
class HipHandle {
    H h_ = nullptr;
    bool owned_ = false;
public:
    HipHandle() = default;
    HipHandle(const HipHandle &) = delete;
    HipHandle &operator=(const HipHandle &) = delete;
    ~HipHandle() { reset(); }
    void reset() { if (h_ && owned_) (void)FREE(h_); h_ = nullptr; owned_ = false; }
    void own(H h) { reset(); h_ = h; owned_ = true; }
    void borrow(H h) { reset(); h_ = h; }
    H get() const { return h_; }
};
using StreamHandle = HipHandle<hipStream_t, hipStreamDestroy>;
using EventHandle = HipHandle<hipEvent_t, hipEventDestroy>;
using PinnedWords = HipHandle<unsigned long long *, hipHostFree>;

// ================================================================================================
// host-side objects
// ================================================================================================
struct trc_ctx {
    int device;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    int n_cu;
};

// `kern`, one thread per item and 256 per workgroup, over n items on the context's stream, and the wait for it: a failure names
// the kernel.  grid_cap: the most workgroups launched, for a kernel that strides over its grid (0: as many as n asks for).  The
// arguments are converted to the kernel's parameter types as a call would convert them.
template <class... P, class... A>
static int launch_wait(trc_ctx *ctx, const char *name, void (*kern)(P...), long long n, long long grid_cap, A... args) {
    long long grid = (n + 255) / 256;
    if (grid_cap && grid > grid_cap) grid = grid_cap;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (P)args...);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (se != hipSuccess) return trc_fail(TRC_ERR_DEVICE, "%s failed: %s", name, hipGetErrorString(se));
    return TRC_OK;
}

static int validate_surface(const trc_surface_desc &s, int idx, int n_extra) {
    char why[512];
    const int st = trc_surface_check(s, idx, n_extra, why, sizeof(why));
    return st == TRC_OK ? TRC_OK : trc_fail(st, "%s", why);
}

// ================================================================================================
// ray staging helpers
// ================================================================================================
// the columns of a bundle as the kernels read them: the caller's own when they are on the device, else copies held in `own`
struct DevRays {
    double *x = nullptr, *y = nullptr, *z = nullptr, *dx = nullptr, *dy = nullptr, *dz = nullptr, *e = nullptr;
    double *ref = nullptr, *wl = nullptr;
    uint64_t *rid = nullptr;
    DevBuf<double> own[9];
    DevBuf<uint64_t> own_rid;
};

static int check_rays(const trc_rays *r, int64_t n, const char *who) {
    if (!r) return trc_fail(TRC_ERR_INVALID, "%s: rays is NULL", who);
    if (r->n < n) return trc_fail(TRC_ERR_INVALID, "%s: bundle holds %lld rays, %lld requested", who, (long long)r->n, (long long)n);
    if (n > 0 && (!r->x || !r->y || !r->z || !r->dx || !r->dy || !r->dz))
        return trc_fail(TRC_ERR_INVALID, "%s: vertices and directions are required", who);
    return TRC_OK;
}

// bring the required columns of a bundle to the device (no copy when already there)
static int stage_rays(const trc_rays *r, int64_t n, bool need_energy, DevRays *d) {
    const double *src[9] = {r->x, r->y, r->z, r->dx, r->dy, r->dz, r->e, r->ref_index, r->wavelength};
    double **dst[9] = {&d->x, &d->y, &d->z, &d->dx, &d->dy, &d->dz, &d->e, &d->ref, &d->wl};
    if (need_energy && !r->e) return trc_fail(TRC_ERR_INVALID, "ray energies are required");
    for (int i = 0; i < 9; ++i) {
        if (!src[i]) continue;
        if (r->on_device) { *dst[i] = (double *)src[i]; continue; }
        TRC_TRY(dev_upload(d->own[i], src[i], (size_t)n));
        *dst[i] = d->own[i].get();
    }
    if (r->rid) {
        if (r->on_device) d->rid = r->rid;
        else {
            TRC_TRY(dev_upload(d->own_rid, r->rid, (size_t)n));
            d->rid = d->own_rid.get();
        }
    }
    return TRC_OK;
}

// ================================================================================================
// rocprim's device-wide scan and sort over 32-bit words, instantiated once for the library
// ================================================================================================
// Defined in the engines' unit (trc_kernels.hip), where the ordered engine sorts its slots with the same instantiation as the hit
// buffer's reader (trc_scene.hip): the library holds rocprim's kernels once, and the engines' unit the same ones as ever -- the
// compiler specialises the HIP headers' shuffle functions for the callers it sees in a module, so the listings of the engine kernels
// that reduce over a wave depend on them (profiles/scene_unit.txt).  tmp null: the size query, as in rocprim.
hipError_t dev_exclusive_scan_u32(void *tmp, size_t &tmp_bytes, uint32_t *in, uint32_t *out, size_t n, hipStream_t stream);
// stable, by bits [0, end_bit) of the keys
hipError_t dev_sort_pairs_u32(void *tmp, size_t &tmp_bytes, uint32_t *key_in, uint32_t *key_out, uint32_t *val_in, uint32_t *val_out, size_t n,
                              unsigned end_bit, hipStream_t stream);

// ================================================================================================
// what the engines call of the scene-free unit (trc_protocol.hip)
// ================================================================================================
static inline bool spectrum_given(const trc_source_spectrum *sp) { return sp && sp->kind != TRC_SPECTRUM_NONE; }
static inline bool spectrum_carried(const trc_source_spectrum *sp) { return sp && sp->kind == TRC_SPECTRUM_CARRIED; }

// The spectrum of a source descriptor as the engines take it: checked, its table packed (trc_spectrum_make).  desc NULL: none.
struct SourceSpectrum {
    const trc_source_spectrum *desc = nullptr;
    std::vector<double> tab;
    int carried() const { return spectrum_carried(desc) ? desc->n : 0; }      // the samples W every ray carries (TRC_SPECTRUM_CARRIED), else 0
};

// ... made by the _x entry points (`who`) from their arguments; a spectrum belongs to a source descriptor
int source_spectrum_make(const trc_source_spectrum *spec, const trc_rays *in, const trc_source_desc *src, const char *who, SourceSpectrum *out);

// A sunshape descriptor as the kernels read it: `tmp` = *src with theta_c, u_c, n in p[] and the table's device address in
// buie[0]; `src` then points to it.  Other kinds are left as they are.  A host-side lookup: no device traffic.
int source_resolve(trc_ctx *ctx, const trc_source_desc *&src, trc_source_desc &tmp, const char *who);

int source_kind_check(const trc_source_desc *src);

// The descriptor `src` (as source_resolve left it) into a new block `d_src`, and the generation kernel of its kind launched on the
// context's stream for rays ray_offset .. ray_offset + n - 1: positions, directions and energies into col[0..6], stream ids into rid
// (null: not wanted).  No wait: d_src lives until the caller has waited for the stream.
int source_generate_start(trc_ctx *ctx, const trc_source_desc *src, DevBuf<trc_source_desc> &d_src, int64_t n, uint64_t seed,
                          uint64_t ray_offset, double *const col[7], uint64_t *rid);

// wl / ref (device columns, either may be NULL) of source rays offset .. offset+n-1 on the context's stream
int spectrum_fill(trc_ctx *ctx, const trc_source_spectrum *sp, const std::vector<double> &tab, int64_t n, uint64_t seed,
                  uint64_t ray_offset, double *wl, double *ref);

// spec_wl / spectra (device, rows `stride` apart, either may be NULL) of n source rays of energies e (device) under a carried spectrum
int carried_fill(trc_ctx *ctx, const trc_source_spectrum *sp, const std::vector<double> &tab, int64_t n, int64_t stride, const double *e,
                 double *spec_wl, double *spectra);

#endif
