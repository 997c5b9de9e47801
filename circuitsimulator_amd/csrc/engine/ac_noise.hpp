// ac_noise.hpp -- the arithmetic of the small-signal noise analysis, defined ONCE for host and device
// (include/csim.h "Noise analysis").
//
// One adjoint solve per (instance, frequency): A^T y = d with A = G + jwC of "AC analysis" and d = +1 at out_p,
// -1 at out_m.  y(a) - y(b) is then the transfer impedance from a current generator between equations (a, b)
// to the output, for every generator at once.  The solve is ac_lu.hpp's, applied to the matrix A^T; the kernels
// (kernels_noise.hip) and the sequential ac_noise_solve() below share the primitives and their order:
//
//   load         A^T(i,j) = G(j,i) + j (w * C(j,i)), the product rounded once; RHS d, real
//   solve        ac_lu_solve(): pivot rule, multiplier, elimination order, zero-multiplier skip, ascending
//                back substitution
//   generator s  z = y(a) - y(b) (cpx_sub; ground = (0, 0));  contrib(s) = (z.re z.re + z.im z.im) psd(s)
//   onoise       0.0 + contrib(0) + contrib(1) + ..., ascending
//   gain         V source with branch equation k: y(k);  I source (p, m): y(m) - y(p)
//   failed LU    onoise, every contrib and the gain are +0.0, CSIM_ST_LU_TINY_PIVOT
#pragma once

#include "ac_lu.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

enum { NOISE_IN_NONE = 0, NOISE_IN_V = 1, NOISE_IN_I = 2 };

CSIM_AC_HD inline cpx noise_at(const double* yr, const double* yi, int eq)
{
    return eq >= 0 ? cpx{yr[eq], yi[eq]} : cpx{0.0, 0.0};
}
// transfer impedance of a generator between equations (a, b)
CSIM_AC_HD inline cpx noise_transfer(const double* yr, const double* yi, int a, int b)
{
    return cpx_sub(noise_at(yr, yi, a), noise_at(yr, yi, b));
}
CSIM_AC_HD inline double noise_contrib(cpx z, double psd) { return (z.re * z.re + z.im * z.im) * psd; }
// in_kind NOISE_IN_V: in_a = branch equation.  NOISE_IN_I: in_a = equation of the minus node, in_b = of the plus node
CSIM_AC_HD inline cpx noise_gain(const double* yr, const double* yi, int inKind, int inA, int inB)
{
    if (inKind == NOISE_IN_V) return noise_at(yr, yi, inA);
    if (inKind == NOISE_IN_I) return noise_transfer(yr, yi, inA, inB);
    return {0.0, 0.0};
}

// Sequential statement of one (system, frequency).  G, C row-major [n][n]; ar, ai work planes of n * ld doubles
// (ld >= n + 1); y gets n values; contrib S values (may be null).  Returns CSIM_ST_* flags.
CSIM_AC_HD inline unsigned ac_noise_solve(int n, const double* G, const double* C, double w, int outP, int outM, int S,
                                          const int32_t* srcA, const int32_t* srcB, const double* psd, int inKind,
                                          int inA, int inB, double eps, int ld, double* ar, double* ai, double* yr,
                                          double* yi, double* contrib, double* onoise, cpx* gain)
{
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            ar[i * ld + j] = G[j * n + i];
            ai[i * ld + j] = w * C[j * n + i];
        }
        ar[i * ld + n] = i == outP ? 1.0 : (i == outM ? -1.0 : 0.0);
        ai[i * ld + n] = 0.0;
    }
    const unsigned fl = ac_lu_solve(n, ld, ar, ai, eps, yr, yi);
    double total = 0.0;
    for (int s = 0; s < S; ++s) {
        const double c = fl ? 0.0 : noise_contrib(noise_transfer(yr, yi, srcA[s], srcB[s]), psd[s]);
        if (contrib) contrib[s] = c;
        total = total + c;
    }
    *onoise = total;
    if (gain) *gain = fl ? cpx{0.0, 0.0} : noise_gain(yr, yi, inKind, inA, inB);
    return fl;
}

} // namespace csim
