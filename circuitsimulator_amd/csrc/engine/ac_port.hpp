// ac_port.hpp -- the arithmetic of the S-parameter analysis, defined ONCE for host and device
// (include/csim.h "S-parameter analysis").
//
// One factorisation per (instance, frequency) of A = G + jwC of "AC analysis", carrying one right-hand side per
// port: the real unit vector at the branch equation of the port's V source.  The kernels (kernels_sp.hip) and the
// sequential routines below share ac_lu.hpp's primitives and their order:
//
//   multi-RHS solve  ac_lu.hpp ac_lu_solve_multi(), one column per port
//   Y                Y(i,j) = -x(j)[k_i], both parts negated (the branch current flows from + through the source)
//   S                M(i,j) = delta_ij + (s_i Y(i,j)) s_j with s_i = sqrt(Z0_i), the two products in that order on re
//                    and im separately, the diagonal as 1.0 + re;  M X = 2 I by the same multi-RHS solve (n = K = P);
//                    S(i,j) = X(i,j) - delta_ij, the real part alone and only on the diagonal
//   failures         A fails: Y and S all +0.0.  M fails: S all +0.0, Y kept.  CSIM_ST_LU_TINY_PIVOT either way.
#pragma once

#include "ac_lu.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

enum { SP_MAX_PORTS = 4 };

// Y [P][P] (row i, column j) from the P solutions (solution j at x[j * ldx ...]); all +0.0 when A failed
CSIM_AC_HD inline void sp_read_y(int P, const int32_t* portEq, bool failed, const double* xr, const double* xi, int ldx,
                                 double* Yr, double* Yi)
{
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j) {
            Yr[i * P + j] = failed ? 0.0 : -xr[j * ldx + portEq[i]];
            Yi[i * P + j] = failed ? 0.0 : -xi[j * ldx + portEq[i]];
        }
}

// S [P][P] from Y [P][P]; sz[i] = sqrt(Z0_i).  Work: mr, mi 2 P P doubles each (M | 2 I, ld = 2 P), tr, ti P P each
// (X, column-wise).  Returns CSIM_ST_* flags; S is all +0.0 when M fails its pivot test.
CSIM_AC_HD inline unsigned sp_s_from_y(int P, const double* Yr, const double* Yi, const double* sz, double eps, double* mr,
                                       double* mi, double* tr, double* ti, double* Sr, double* Si)
{
    const int ld = 2 * P;
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j) {
            const double re = (sz[i] * Yr[i * P + j]) * sz[j];
            const double im = (sz[i] * Yi[i * P + j]) * sz[j];
            mr[i * ld + j] = i == j ? 1.0 + re : re;
            mi[i * ld + j] = im;
            mr[i * ld + P + j] = i == j ? 2.0 : 0.0;
            mi[i * ld + P + j] = 0.0;
        }
    const unsigned fl = ac_lu_solve_multi(P, P, ld, mr, mi, eps, tr, ti, P);
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j) {
            const double xr = tr[j * P + i];
            Sr[i * P + j] = fl ? 0.0 : (i == j ? xr - 1.0 : xr);
            Si[i * P + j] = fl ? 0.0 : ti[j * P + i];
        }
    return fl;
}

// Sequential statement of one (system, frequency).  G, C row-major [n][n]; ar, ai work planes of n * ld doubles
// (ld >= n + P); xr, xi P * n doubles; Y, S [P][P]; mr, mi, tr, ti as sp_s_from_y (Sr null: Y only).
CSIM_AC_HD inline unsigned ac_sp_solve(int n, const double* G, const double* C, double w, int P, const int32_t* portEq,
                                       const double* sz, double eps, int ld, double* ar, double* ai, double* xr,
                                       double* xi, double* Yr, double* Yi, double* mr, double* mi, double* tr, double* ti,
                                       double* Sr, double* Si)
{
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            ar[i * ld + j] = G[i * n + j];
            ai[i * ld + j] = w * C[i * n + j];
        }
        for (int c = 0; c < P; ++c) {
            ar[i * ld + n + c] = i == portEq[c] ? 1.0 : 0.0;
            ai[i * ld + n + c] = 0.0;
        }
    }
    unsigned fl = ac_lu_solve_multi(n, P, ld, ar, ai, eps, xr, xi, n);
    sp_read_y(P, portEq, fl != 0u, xr, xi, n, Yr, Yi);
    if (!Sr) return fl;
    if (fl) {
        for (int e = 0; e < P * P; ++e) { Sr[e] = 0.0; Si[e] = 0.0; }
        return fl;
    }
    fl |= sp_s_from_y(P, Yr, Yi, sz, eps, mr, mi, tr, ti, Sr, Si);
    return fl;
}

} // namespace csim
