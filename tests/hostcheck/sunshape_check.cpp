// sunshape_check.cpp -- TEST-ONLY host build of the tabulated-sunshape parts of the per-ray core (tracer_amd/csrc/trc_core.h:
// trc_sunshape_pack, trc_sunshape_theta, the sunshape kinds of trc_source_ray), and the size of trc_source_desc as the compiler
// lays it out.  Built by `make hostcheck` into tests/hostcheck/, loaded only by the sunshape tests; not a product path.
#include <string.h>
#include "../../tracer_amd/csrc/trc_core.h"

extern "C" {

long hs_sizeof_source_desc(void) { return (long)sizeof(trc_source_desc); }

// tab[3n] = theta | g | cdf and the core (theta_c, u_c) as trc_sunshape_create packs them; 0 for a table without mass
int hs_sunshape_pack(int n, const double *angle, const double *intensity, double *tab, double *theta_c, double *u_c) {
    return trc_sunshape_pack(n, angle, intensity, tab, theta_c, u_c) ? 1 : 0;
}

// out[k] = the polar angle of uniform u[k]
void hs_sunshape_theta(const double *tab, int n, long m, const double *u, double *out) {
    for (long k = 0; k < m; ++k) out[k] = trc_sunshape_theta(tab, n, u[k]);
}

// rays rid0 .. rid0+m-1 of a sunshape descriptor (kind, frames, p[0..1], energy as the caller made it) over the packed table,
// resolved as the library resolves it: theta_c, u_c, n in p[5..7], the table's address in buie[0]
void hs_sunshape_rays(const trc_source_desc *src_in, const double *tab, int n, double theta_c, double u_c, unsigned long long seed,
                      unsigned long long rid0, long m, double *x, double *y, double *z, double *dx, double *dy, double *dz) {
    trc_source_desc src = *src_in;
    src.p[TRC_SUNSHAPE_P_THETA_C] = theta_c;
    src.p[TRC_SUNSHAPE_P_U_C] = u_c;
    src.p[TRC_SUNSHAPE_P_N] = (double)n;
    memset(src.buie, 0, sizeof(src.buie));
    src.buie[0] = __builtin_bit_cast(double, (uint64_t)(uintptr_t)tab);
    for (long k = 0; k < m; ++k)
        trc_source_ray(&src, src.buie, nullptr, seed, rid0 + (unsigned long long)k, &x[k], &y[k], &z[k], &dx[k], &dy[k], &dz[k]);
}

// the uniform of the polar angle of ray rid (event 0, block 0: the third of the four)
void hs_sunshape_u2(unsigned long long seed, unsigned long long rid0, long m, double *u) {
    for (long k = 0; k < m; ++k) {
        double u0, u1, u2, u3;
        trc_uniform_quad(seed, rid0 + (unsigned long long)k, 0, 0, &u0, &u1, &u2, &u3);
        u[k] = u2;
    }
}

}
