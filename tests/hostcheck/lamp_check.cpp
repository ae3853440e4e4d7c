// lamp_check.cpp -- TEST-ONLY host build of the arc-lamp parts of the per-ray core (tracer_amd/csrc/trc_core.h: trc_lamp_local_u,
// trc_lamp_ray_t through trc_source_ray, trc_angle_table_pack) and of the decisions trc_forms.h makes for their kinds.  Built by
// `make hostcheck` into tests/hostcheck/, loaded only by the lamp tests; not a product path.
#include <string.h>
#include "../../tracer_amd/csrc/trc_forms.h"

extern "C" {

long hl_sizeof_source_desc(void) { return (long)sizeof(trc_source_desc); }
int hl_kind(int which) { return which == 0 ? TRC_SRC_ARC_VOLUME : which == 1 ? TRC_SRC_EMIT_SPHERE : TRC_SRC_EMIT_CYLINDER; }

// tab[3n] = angle | density | cdf as trc_angle_table_create packs them; 0 for a table without mass
int hl_angle_table_pack(int n, const double *angle, const double *density, double *tab) {
    return trc_angle_table_pack(n, angle, density, tab) ? 1 : 0;
}

static trc_source_desc hl_resolved(const trc_source_desc *src_in, const double *tab, int n_tab) {
    trc_source_desc src = *src_in;
    if (src.kind == TRC_SRC_ARC_VOLUME) {       // as source_resolve leaves it
        src.p[TRC_SUNSHAPE_P_N] = (double)n_tab;
        memset(src.buie, 0, sizeof(src.buie));
        src.buie[0] = __builtin_bit_cast(double, (uint64_t)(uintptr_t)tab);
    }
    return src;
}

// m rays of a lamp descriptor from GIVEN uniforms u[5][m] (u0..u4; u4 is read by ARC_VOLUME alone) in place of the Philox draws:
// what trc_lamp_ray_t computes behind its draws, posed
void hl_lamp_rays_u(const trc_source_desc *src_in, const double *tab, int n_tab, long m, const double *u, double *x, double *y, double *z,
                    double *dx, double *dy, double *dz) {
    const trc_source_desc src = hl_resolved(src_in, tab, n_tab);
    for (long k = 0; k < m; ++k) {
        double lx, ly, lz, ax, ay, az;
        trc_lamp_local_u(src.kind, src.p, tab, n_tab, u[k], u[m + k], u[2 * m + k], u[3 * m + k], u[4 * m + k], &lx, &ly, &lz, &ax, &ay, &az);
        trc_lamp_pose(&src, lx, ly, lz, ax, ay, az, &x[k], &y[k], &z[k], &dx[k], &dy[k], &dz[k]);
    }
}

// rays rid0 .. rid0+m-1 with their Philox draws, through the entry every engine's generation goes through
void hl_lamp_rays(const trc_source_desc *src_in, const double *tab, int n_tab, unsigned long long seed, unsigned long long rid0, long m,
                  double *x, double *y, double *z, double *dx, double *dy, double *dz) {
    const trc_source_desc src = hl_resolved(src_in, tab, n_tab);
    for (long k = 0; k < m; ++k)
        trc_source_ray(&src, src.buie, nullptr, seed, rid0 + (unsigned long long)k, &x[k], &y[k], &z[k], &dx[k], &dy[k], &dz[k]);
}

// the uniforms of ray rid: u[0..3] of event 0, block `block`
void hl_uniforms(unsigned long long seed, unsigned long long rid, unsigned block, double *u) {
    trc_uniform_quad(seed, rid, 0, block, &u[0], &u[1], &u[2], &u[3]);
}

// The decisions for a call with source kind `kind` (-1: given rays) on a scene of n_surf surfaces with an LDS-sized grid: names of the
// megakernel's instance, of gen0, of `first`, whether a footprint map applies and whether fresh rays go through k_s_bounce<.., FRESH>.
// walk_ok = 0: a scene whose search tables do not fit LDS (the large grid).  Returns use_stream of trc_fast_choose_engine.
int hl_decide(int kind, int n_surf, long long n, int flags, int spec, int walk_ok, char *mega, char *gen0, char *first, int len, int *has_map,
              int *use_first, int *valid) {
    trc_facts f = {};
    trc_scene_facts &s = f.scene;
    s.n_surf = n_surf; s.stride = 17; s.accel_ok = true; s.grid_ok = walk_ok != 0; s.big_ok = true;
    s.grid_cells = 64; s.grid_list = 4 * n_surf; s.brute_list = n_surf; s.big_occ_words = 64;
    s.walked = true; s.cls_moving = s.cls_all = 1u << TRC_CLS_MIRROR;
    f.call = {n, flags, kind, spec != 0, false, false, true, 0, 0};
    f.knobs = {2, true, true, false, true, -1, true, false, 0, 0, 0, true, 2};
    const trc_engine_choice E = trc_fast_choose_engine(f.scene, f.call, f.knobs);
    const MegaPlan M = mega_plan(f.scene, f.call);
    trc_kernel_name(M.id, mega, (size_t)len);
    *valid = trc_kernel_id_valid(M.id) ? 1 : 0;
    *has_map = trc_src_kind_has_map(kind) ? 1 : 0;
    gen0[0] = first[0] = 0;
    *use_first = -1;
    StreamPlan plan = {0, 0, true};
    if (stream_plan(f.scene, (flags & TRC_TRACE_ACCEL) != 0, f.knobs, &plan)) {
        trc_stream_forms F;
        if (trc_stream_decide(f, plan, &F)) {
            trc_kernel_name(F.gen0.id, gen0, (size_t)len);
            trc_kernel_name(F.first.id, first, (size_t)len);
            *use_first = F.use_first ? 1 : 0;
            *valid = *valid && trc_kernel_id_valid(F.gen0.id);
        }
    }
    return E.use_stream ? 1 : 0;
}

}
