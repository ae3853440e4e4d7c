// material_check.cpp -- TEST-ONLY host build of the tabulated materials' lookup of the per-ray core (tracer_amd/csrc/trc_core.h,
// trc_material_index).  Built by `make hostcheck` into tests/hostcheck/, loaded only by the material-table tests; not a product path.
#include "../../tracer_amd/csrc/trc_core.h"

extern "C" {

// re[i], im[i] = material k of the packed table `tab` (n_mat | offset, n per material | per material n | wl | re | im) at wavelength wl[i]
void hm_material_index(const double *tab, int k, long m, const double *wl, double *re, double *im) {
    for (long i = 0; i < m; ++i) trc_material_index(tab, k, wl[i], re + i, im + i);
}

// the same for two materials at once, as a surface between them asks (trc_material_index2)
void hm_material_index2(const double *tab, int k0, int k1, long m, const double *wl, double *re0, double *im0, double *re1, double *im1) {
    for (long i = 0; i < m; ++i) trc_material_index2(tab, k0, k1, wl[i], re0 + i, im0 + i, re1 + i, im1 + i);
}

int hm_max_points(void) { return TRC_MATERIAL_MAX_POINTS; }
int hm_max_materials(void) { return TRC_MATERIAL_MAX; }

}
