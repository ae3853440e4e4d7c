// fluxmap_check.cpp -- TEST-ONLY host build of the flux-map binning of the per-ray core (tracer_amd/csrc/trc_core.h:
// trc_fluxmap_uv, trc_bin_index): what record_hit and k_ord_bounce run per hit on the device.  Built by `make hostcheck` into
// tests/hostcheck/, loaded only by the flux-map chart tests; not a product path.
#include "../../tracer_amd/csrc/trc_core.h"

extern "C" {

int hf_n_charts(void) { return TRC_FM_CHARTS; }

// (u, v)[k] of global point k in `chart` through proj12
void hf_fluxmap_uv(int chart, const double *proj12, long m, const double *x, const double *y, const double *z, double *u, double *v) {
    for (long k = 0; k < m; ++k) trc_fluxmap_uv(chart, proj12, x[k], y[k], z[k], &u[k], &v[k]);
}

// bin[k] = iu * nv + iv of global point k on the map's edges, -1 outside: the index the kernels add the absorbed energy at
void hf_fluxmap_bin(int chart, const double *proj12, int nu, int nv, const double *u_edges, const double *v_edges, long m, const double *x,
                    const double *y, const double *z, long *bin) {
    for (long k = 0; k < m; ++k) {
        double u, v;
        trc_fluxmap_uv(chart, proj12, x[k], y[k], z[k], &u, &v);
        const int iu = trc_bin_index(u_edges, nu, u), iv = trc_bin_index(v_edges, nv, v);
        bin[k] = (iu >= 0 && iv >= 0) ? (long)iu * nv + iv : -1;
    }
}

}
