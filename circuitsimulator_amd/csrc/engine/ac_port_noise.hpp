// ac_port_noise.hpp -- the arithmetic of the two-port noise analysis, defined ONCE for host and device
// (include/csim.h "Two-port noise analysis").
//
// One factorisation per (instance, frequency) of A^T, A = G + jwC of "AC analysis", carrying one adjoint right-hand
// side per port: the real unit vector at the branch equation k_i of the port's V source.  Column i of the solution,
// lambda_i, holds the transfer from every equation to the current of port i: lambda_i[k_j] is (minus) Y(i,j), and
// lambda_i(a) - lambda_i(b) the transfer of a current generator between (a, b), for every generator at once.  The
// kernels (kernels_spnoise.hip) and the sequential ac_spnoise_solve() below share the primitives and their order:
//
//   load        A^T(i,j) = G(j,i) + j (w * C(j,i)), the product rounded once (ac_noise.hpp); RHS c real, e_{k_c}
//   solve       ac_lu.hpp ac_lu_solve_multi(), one column per port
//   Y           Y(i,j) = -lambda_i[k_j], both parts negated
//   generator s t_i = noise_transfer(lambda_i, a_s, b_s);  for i <= j  q = spn_corr(t_i, t_j, psd_s)
//   Cy          Cy(i,j) = 0.0 + q(0) + q(1) + ..., ascending, re and im separately (i < j); the diagonal sums re
//               alone, its im is +0.0;  Cy(j,i) = (re, -im)
//   two-port    spn_two_port() below, P == 2 only
//   failed LU   Y, Cy and the noise parameters all +0.0, CSIM_ST_LU_TINY_PIVOT
//
// Every real division is x * (1.0 / y) with the reciprocal formed first; complex divisions are cpx_div.
#pragma once

#include <math.h>

#include "ac_lu.hpp"
#include "ac_noise.hpp"
#include "ac_port.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __clang__
#define CSIM_SPN_UNROLL _Pragma("unroll")
#else
#define CSIM_SPN_UNROLL
#endif

namespace csim {

// t_i conj(t_j) psd: the contribution of one generator to Cy(i,j).  With i == j the real part is noise_contrib().
CSIM_AC_HD inline cpx spn_corr(cpx ti, cpx tj, double psd)
{
    return {(ti.re * tj.re + ti.im * tj.im) * psd, (ti.im * tj.re - ti.re * tj.im) * psd};
}

// index of the pair (i, j), i <= j < K, in the packed upper triangle
CSIM_AC_HD constexpr int spn_pair(int K, int i, int j) { return i * K - (i * (i - 1)) / 2 + (j - i); }

CSIM_AC_HD inline double spn_max0(double x) { return x < 0.0 ? 0.0 : x; }      // a NaN passes through

struct TwoPortNoise { double nf, fmin, rn, yoptRe, yoptIm; };

// Noise parameters of a two-port (port 1 the input) from Y11, Y21 and Cy: the chain-matrix correlation (Cvv, Cii,
// Cvi), then Rn, Ycor = Gcor + j Bcor, Gu, Yopt, Fmin, and NF at the source conductance gs.  kT40 = 4 k 290.
// All linear.  c11, c22 the diagonal of Cy, c12 = Cy(1,2).  Y21 == 0 gets what IEEE arithmetic gives.
CSIM_AC_HD inline TwoPortNoise spn_two_port(cpx y11, cpx y21, double c11, double c22, cpx c12, double kT40, double gs)
{
    const double ikt = 1.0 / kT40, igs = 1.0 / gs;
    const double d = cpx_abs2(y21);
    const cpx r = cpx_div(y11, y21);
    const double cvv = c22 * (1.0 / d);
    const double rc = r.re * c12.re + r.im * c12.im;                 // Re(conj(r) Cy12)
    const double cii = (c11 - 2.0 * rc) + cpx_abs2(r) * c22;
    TwoPortNoise o;
    if (!(cvv > 0.0)) {                                              // no voltage noise: nothing to match against
        o.rn = 0.0;
        o.yoptRe = 0.0;
        o.yoptIm = 0.0;
        o.fmin = 1.0;
        o.nf = 1.0 + (cii * ikt) * igs;
        return o;
    }
    // Cvi = -(Cy21 - conj(r) Cy22) / Y21 with Cy21 = conj(Cy12);  Ycor = conj(Cvi) / Cvv
    const cpx q = cpx_div({c12.re - r.re * c22, r.im * c22 - c12.im}, y21);
    const double icvv = 1.0 / cvv;
    const double gcor = (-q.re) * icvv, bcor = q.im * icvv;
    const double rn = cvv * ikt;
    const double gu = (cii - (gcor * gcor + bcor * bcor) * cvv) * ikt;
    const double gopt = sqrt(spn_max0(gu * (1.0 / rn) + gcor * gcor));
    const double gsc = gs + gcor;
    o.rn = rn;
    o.yoptRe = gopt;
    o.yoptIm = -bcor;
    o.fmin = 1.0 + (2.0 * rn) * (gcor + gopt);
    o.nf = 1.0 + (gu + rn * (gsc * gsc + bcor * bcor)) * igs;
    return o;
}

// Y [P][P] from the adjoint solutions (solution i at x[i * ldx ...]); all +0.0 when the factorisation failed
CSIM_AC_HD inline void spn_read_y(int P, const int32_t* portEq, bool failed, const double* xr, const double* xi, int ldx,
                                  double* Yr, double* Yi)
{
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j) {
            Yr[i * P + j] = failed ? 0.0 : -xr[i * ldx + portEq[j]];
            Yi[i * P + j] = failed ? 0.0 : -xi[i * ldx + portEq[j]];
        }
}

// Cy [P][P] from the sums over the generators of the upper triangle (pair (i, j) at spn_pair(K, i, j)).  The loops
// have constant bounds so that a kernel holding the sums in registers indexes them with constants.
template <int K>
CSIM_AC_HD inline void spn_fill_cy(int P, bool failed, const double (&sumRe)[K * (K + 1) / 2],
                                   const double (&sumIm)[K * (K + 1) / 2], double* Cr, double* Ci)
{
    CSIM_SPN_UNROLL
    for (int i = 0; i < K; ++i) {
        CSIM_SPN_UNROLL
        for (int j = i; j < K; ++j) {
            if (j >= P) continue;
            const int p = spn_pair(K, i, j);
            Cr[i * P + j] = failed ? 0.0 : sumRe[p];
            Ci[i * P + j] = (failed || i == j) ? 0.0 : sumIm[p];
            if (i != j) {
                Cr[j * P + i] = failed ? 0.0 : sumRe[p];
                Ci[j * P + i] = failed ? 0.0 : -sumIm[p];
            }
        }
    }
}

// the noise parameters of a failed (instance, frequency)
CSIM_AC_HD inline TwoPortNoise spn_failed() { return {0.0, 0.0, 0.0, 0.0, 0.0}; }

// Sequential statement of one (system, frequency).  G, C row-major [n][n]; ar, ai work planes of n * ld doubles
// (ld >= n + P); xr, xi P * n doubles (the adjoint solutions); Y, Cy [P][P]; tp filled when P == 2 and not null.
CSIM_AC_HD inline unsigned ac_spnoise_solve(int n, const double* G, const double* C, double w, int P, const int32_t* portEq,
                                            int S, const int32_t* srcA, const int32_t* srcB, const double* psd, double kT40,
                                            double gs, double eps, int ld, double* ar, double* ai, double* xr, double* xi,
                                            double* Yr, double* Yi, double* Cr, double* Ci, TwoPortNoise* tp)
{
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            ar[i * ld + j] = G[j * n + i];
            ai[i * ld + j] = w * C[j * n + i];
        }
        for (int c = 0; c < P; ++c) {
            ar[i * ld + n + c] = i == portEq[c] ? 1.0 : 0.0;
            ai[i * ld + n + c] = 0.0;
        }
    }
    const unsigned fl = ac_lu_solve_multi(n, P, ld, ar, ai, eps, xr, xi, n);
    const bool failed = fl != 0u;
    spn_read_y(P, portEq, failed, xr, xi, n, Yr, Yi);
    double sumRe[SP_MAX_PORTS * (SP_MAX_PORTS + 1) / 2], sumIm[SP_MAX_PORTS * (SP_MAX_PORTS + 1) / 2];
    for (int i = 0; i < P; ++i)
        for (int j = i; j < P; ++j) {
            double re = 0.0, im = 0.0;
            for (int s = 0; s < S && !failed; ++s) {
                const cpx q = spn_corr(noise_transfer(xr + i * n, xi + i * n, srcA[s], srcB[s]),
                                       noise_transfer(xr + j * n, xi + j * n, srcA[s], srcB[s]), psd[s]);
                re = re + q.re;
                if (i != j) im = im + q.im;
            }
            sumRe[spn_pair(SP_MAX_PORTS, i, j)] = re;
            sumIm[spn_pair(SP_MAX_PORTS, i, j)] = im;
        }
    spn_fill_cy<SP_MAX_PORTS>(P, failed, sumRe, sumIm, Cr, Ci);
    if (tp && P == 2)
        *tp = failed ? spn_failed() : spn_two_port({Yr[0], Yi[0]}, {Yr[2], Yi[2]}, Cr[0], Cr[3], {Cr[1], Ci[1]}, kT40, gs);
    return fl;
}

} // namespace csim
