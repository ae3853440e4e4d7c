// spectrum_check.cpp -- TEST-ONLY host build of the source-spectrum sampler of the per-ray core (tracer_amd/csrc/trc_core.h,
// trc_spectrum_sample / trc_spectrum_draw), and the size of trc_source_spectrum as the compiler lays it out.  Built by
// `make hostcheck` into tests/hostcheck/, loaded only by the spectrum tests; not a product path.
#include "../../tracer_amd/csrc/trc_core.h"

extern "C" {

long hs_sizeof_spectrum(void) { return (long)sizeof(trc_source_spectrum); }

// out[k] = the wavelength of uniform u[k] (wl | density normalised to a unit integral | its running integral, as packed)
void hs_spectrum_sample(const double *wl, const double *val, const double *cdf, int n, long m, const double *u, double *out) {
    for (long k = 0; k < m; ++k) out[k] = trc_spectrum_sample(wl, val, cdf, n, u[k]);
}

// out[k] = the wavelength of source ray rid0 + k under `seed`, and u[k] the uniform it was drawn from (host Philox)
void hs_spectrum_draw(const double *wl, const double *val, const double *cdf, int n, unsigned long long seed,
                      unsigned long long rid0, long m, double *u, double *out) {
    for (long k = 0; k < m; ++k) {
        double u0, u1;
        trc_uniform_pair(seed, rid0 + (unsigned long long)k, 0u, TRC_SPECTRUM_BLOCK, &u0, &u1);
        if (u) u[k] = u0;
        out[k] = trc_spectrum_draw(wl, val, cdf, n, seed, rid0 + (unsigned long long)k);
    }
}

}
