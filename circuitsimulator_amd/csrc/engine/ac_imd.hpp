// ac_imd.hpp -- the arithmetic of the two-tone intermodulation analysis, defined ONCE for host and device
// (include/csim.h "Intermodulation analysis").
//
// Volterra series at the operating point with two tones w1 and w2: six dependent solves per point on ac_lu.hpp's LU.
// The kernels (kernels_imd.hip) and the sequential ac_imd_solve() below share the primitives and their order.  A
// "pair" is the two controlling voltages of a device, (Ug, Ud) = (x[g] - x[s], x[d] - x[s]) (disto_u); c are the
// seven coefficients of disto_coef (ac_disto.hpp); * is the conjugate.
//
//   Q(A, B)     0.5 ((c_gg (Ag Bg) + c_gd ((Ag Bd) + (Ad Bg))) + c_dd (Ad Bd))                                  imd_q()
//   T(A, A, B)  ((((c_ggg (GG Bg) + c_ggd ((GG Bd) + 2.0 (GD Bg))) + c_gdd (2.0 (GD Bd) + (DD Bg))) + c_ddd (DD Bd))
//               / 6.0, with GG = Ag Ag, GD = Ag Ad, DD = Ad Ad                                                    imd_t()
//
//   k  frequency             drain current of a device (Ua, Ub, Vd, Vh: the pairs of x0, x1, x3, x4)
//   0  w1                    -- (right-hand side J1)
//   1  w2                    -- (right-hand side J2)
//   2  w1 + w2               Q(Ua, Ub)
//   3  w1 - w2               Q(Ua, Ub*)
//   4  2.0 w1                disto_i2(Ua)                     = 0.5 Q(Ua, Ua)
//   5  (2.0 w1) - w2         (0.75 T(Ua, Ua, Ub*) + Q(Ua, Vd)) + Q(Ub*, Vh)
//
//   right-hand    every entry starts at +0.0; the devices in ascending order subtract their current at d, then add
//   side          it at s (re and im separately)
//   failure       a failed solve zeroes itself and every later one (+0.0), all six factorisations are attempted
//   IM            v_k = x_k[out_p] - x_k[out_m]; IM2+ = |v_2| / |v_0|, IM2- = |v_3| / |v_0|, IM3 = |v_5| / |v_0| by
//                 disto_abs and disto_hd: +0.0 where |v_0| == 0
//
// A real factor times a complex value scales re and im, one product (or quotient) each.  Sums run left to right.
#pragma once

#include "ac_disto.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

enum { IMD_NSOLVE = 6, IMD_NRATIO = 3 };

CSIM_AC_HD inline cpx cpx_conj(cpx a) { return {a.re, -a.im}; }

// the frequency of solve k
CSIM_AC_HD inline double imd_freq(int k, double w1, double w2)
{
    switch (k) {
    case 0: return w1;
    case 1: return w2;
    case 2: return w1 + w2;
    case 3: return w1 - w2;
    case 4: return 2.0 * w1;
    default: return 2.0 * w1 - w2;
    }
}

// second-order mixing current of the pairs (Ag, Ad) and (Bg, Bd)
CSIM_AC_HD inline cpx imd_q(const double* c, cpx Ag, cpx Ad, cpx Bg, cpx Bd)
{
    cpx t = cpx_scale(c[DC_GG], cpx_mul(Ag, Bg));
    t = cpx_add(t, cpx_scale(c[DC_GD], cpx_add(cpx_mul(Ag, Bd), cpx_mul(Ad, Bg))));
    t = cpx_add(t, cpx_scale(c[DC_DD], cpx_mul(Ad, Bd)));
    return cpx_scale(0.5, t);
}

// third-order mixing current of the pair (Ag, Ad) taken twice and (Bg, Bd) once
CSIM_AC_HD inline cpx imd_t(const double* c, cpx Ag, cpx Ad, cpx Bg, cpx Bd)
{
    const cpx gg = cpx_mul(Ag, Ag), gd = cpx_mul(Ag, Ad), dd = cpx_mul(Ad, Ad);
    cpx t = cpx_scale(c[DC_GGG], cpx_mul(gg, Bg));
    t = cpx_add(t, cpx_scale(c[DC_GGD], cpx_add(cpx_mul(gg, Bd), cpx_scale(2.0, cpx_mul(gd, Bg)))));
    t = cpx_add(t, cpx_scale(c[DC_GDD], cpx_add(cpx_scale(2.0, cpx_mul(gd, Bd)), cpx_mul(dd, Bg))));
    t = cpx_add(t, cpx_scale(c[DC_DDD], cpx_mul(dd, Bd)));
    return {t.re / 6.0, t.im / 6.0};
}

// drain current of a device with terminals (d, g, s) in solve k (2 .. 5).  X0, X1, X3, X4: re and im of the kept
// solutions (each indexed by equation; the later ones are not read before their solve)
CSIM_AC_HD inline cpx imd_current(int k, const double* c, int d, int g, int s, const double* X0r, const double* X0i,
                                  const double* X1r, const double* X1i, const double* X3r, const double* X3i,
                                  const double* X4r, const double* X4i)
{
    const cpx Uag = disto_u(X0r, X0i, g, s), Uad = disto_u(X0r, X0i, d, s);
    if (k == 4) return disto_i2(c, Uag, Uad);
    const cpx Ubg = disto_u(X1r, X1i, g, s), Ubd = disto_u(X1r, X1i, d, s);
    if (k == 2) return imd_q(c, Uag, Uad, Ubg, Ubd);
    const cpx Cbg = cpx_conj(Ubg), Cbd = cpx_conj(Ubd);
    if (k == 3) return imd_q(c, Uag, Uad, Cbg, Cbd);
    cpx t = cpx_scale(0.75, imd_t(c, Uag, Uad, Cbg, Cbd));
    t = cpx_add(t, imd_q(c, Uag, Uad, disto_u(X3r, X3i, g, s), disto_u(X3r, X3i, d, s)));
    return cpx_add(t, imd_q(c, Cbg, Cbd, disto_u(X4r, X4i, g, s), disto_u(X4r, X4i, d, s)));
}

// Sequential statement of one (system, tone pair).  G, C row-major [n][n]; J1, J2 re and im [n]; devices devD, devG,
// devS [M] (equations, -1 ground) with coef [M][7]; ar, ai work planes of n * ld doubles (ld >= n + 1); x gets 6 * n
// values per part (solve k at x[k * n]); im gets IM2+, IM2-, IM3.  Returns CSIM_ST_* flags.
CSIM_AC_HD inline unsigned ac_imd_solve(int n, const double* G, const double* C, const double* J1r, const double* J1i,
                                        const double* J2r, const double* J2i, double w1, double w2, int M,
                                        const int32_t* devD, const int32_t* devG, const int32_t* devS, const double* coef,
                                        int outP, int outM, double eps, int ld, double* ar, double* ai, double* xr,
                                        double* xi, double* im)
{
    unsigned flags = 0u;
    bool failed = false;
    for (int k = 0; k < IMD_NSOLVE; ++k) {
        const double wk = imd_freq(k, w1, w2);
        double* yr = xr + k * n;
        double* yi = xi + k * n;
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j) {
                ar[i * ld + j] = G[i * n + j];
                ai[i * ld + j] = wk * C[i * n + j];
            }
            ar[i * ld + n] = k == 0 ? J1r[i] : (k == 1 ? J2r[i] : 0.0);
            ai[i * ld + n] = k == 0 ? J1i[i] : (k == 1 ? J2i[i] : 0.0);
        }
        if (k > 1)
            for (int m = 0; m < M; ++m) {
                const int d = devD[m], g = devG[m], s = devS[m];
                const cpx I = imd_current(k, coef + m * DISTO_NCOEF, d, g, s, xr, xi, xr + n, xi + n, xr + 3 * n, xi + 3 * n,
                                          xr + 4 * n, xi + 4 * n);
                if (d >= 0) { ar[d * ld + n] = ar[d * ld + n] - I.re; ai[d * ld + n] = ai[d * ld + n] - I.im; }
                if (s >= 0) { ar[s * ld + n] = ar[s * ld + n] + I.re; ai[s * ld + n] = ai[s * ld + n] + I.im; }
            }
        const unsigned fl = ac_lu_solve(n, ld, ar, ai, eps, yr, yi);
        flags |= fl;
        failed = failed || fl != 0u;
        if (failed)
            for (int i = 0; i < n; ++i) { yr[i] = 0.0; yi[i] = 0.0; }
    }
    const double v0 = disto_abs(disto_u(xr, xi, outP, outM));
    im[0] = disto_hd(disto_abs(disto_u(xr + 2 * n, xi + 2 * n, outP, outM)), v0);
    im[1] = disto_hd(disto_abs(disto_u(xr + 3 * n, xi + 3 * n, outP, outM)), v0);
    im[2] = disto_hd(disto_abs(disto_u(xr + 5 * n, xi + 5 * n, outP, outM)), v0);
    return flags;
}

} // namespace csim
