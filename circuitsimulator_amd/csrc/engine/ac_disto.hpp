// ac_disto.hpp -- the arithmetic of the small-signal distortion analysis, defined ONCE for host and device
// (include/csim.h "Distortion analysis").
//
// Volterra series at the operating point, single tone: a first-order AC solve at w, a second-order solve at 2 w
// driven by the quadratic terms of the MOSFET drain currents, a third-order solve at 3 w driven by the cubic terms
// and by the mix of first and second order.  The solves are ac_lu.hpp's; the kernels (kernels_disto.hip) and the
// sequential ac_disto_solve() below share the primitives and their order:
//
//   coefficients  disto_coef(): the second and third derivatives of the level-1 drain current at x_op, region
//                 decided by the comparisons of mos_eval (device_common.hpp); seven per device, DC_*
//   device m      Ug = x[g] - x[s], Ud = x[d] - x[s] (ground = (0, 0)); disto_i2(), disto_i3()
//   right-hand    every entry starts at +0.0; the devices in ascending order subtract their current at d, then add
//   side          it at s (re and im separately)
//   orders        A(w) x1 = J, A(2.0 w) x2 = rhs2, A(3.0 w) x3 = rhs3; a failed order zeroes itself and every higher
//                 one (+0.0), all three factorisations are attempted
//   HD            v_k = x_k[out_p] - x_k[out_m]; |z| = sqrt(re re + im im); HD_k = |v_k| / |v_1|, +0.0 where |v_1| == 0
//
// A real factor times a complex value scales re and im, one product each.  Sums run left to right.
#pragma once

#include <math.h>

#include "ac_lu.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

// order of the seven coefficients of a device: d2I/dUg2, d2I/dUgdUd, d2I/dUd2, d3I/dUg3, d3I/dUg2dUd, d3I/dUgdUd2, d3I/dUd3
enum { DC_GG = 0, DC_GD = 1, DC_DD = 2, DC_GGG = 3, DC_GGD = 4, DC_GDD = 5, DC_DDD = 6, DISTO_NCOEF = 7 };

struct DistoCoef { double c[DISTO_NCOEF]; };

// Derivatives of the drain current (drain -> source) in Ug = Vg - Vs, Ud = Vd - Vs at (Vd, Vg, Vs).  The current is
// piecewise a polynomial of degree <= 3, so inside a region these are its exact Taylor data.
CSIM_AC_HD inline DistoCoef disto_coef(bool isP, double Vth, double K, double lambda, double Vd, double Vg, double Vs)
{
    DistoCoef r;
    for (int i = 0; i < DISTO_NCOEF; ++i) r.c[i] = 0.0;
    const double p = isP ? -1.0 : 1.0;
    const double Vgs = p * (Vg - Vs);
    const double Vds = p * (Vd - Vs);
    if (!(Vgs > Vth && Vds >= 0.0)) return r;               // off
    const double factor = 1.0 + lambda * Vds;
    if (factor < 0.0) return r;                             // mos_eval clamps it to 0: no current
    const double Vov = Vgs - Vth;
    double gg = 0.0, gd = 0.0, dd = 0.0;
    if (Vds < Vov) {                                        // triode
        gd = K * factor + (K * Vds) * lambda;
        dd = 2.0 * ((K * (Vov - Vds)) * lambda) - K * factor;
        r.c[DC_GDD] = 2.0 * (K * lambda);
        r.c[DC_DDD] = -3.0 * (K * lambda);
    } else {                                                // saturation
        gg = K * factor;
        gd = (K * Vov) * lambda;
        r.c[DC_GGD] = K * lambda;
    }
    r.c[DC_GG] = p * gg;                                    // I = p Ieff(p Ug, p Ud): second order p p^2, third p p^3 = 1
    r.c[DC_GD] = p * gd;
    r.c[DC_DD] = p * dd;
    return r;
}

CSIM_AC_HD inline cpx cpx_add(cpx a, cpx b) { return {a.re + b.re, a.im + b.im}; }
CSIM_AC_HD inline cpx cpx_scale(double s, cpx a) { return {s * a.re, s * a.im}; }
CSIM_AC_HD inline cpx disto_at(const double* xr, const double* xi, int eq)
{
    return eq >= 0 ? cpx{xr[eq], xi[eq]} : cpx{0.0, 0.0};
}
// controlling voltage of a device: x[a] - x[s]
CSIM_AC_HD inline cpx disto_u(const double* xr, const double* xi, int a, int s)
{
    return cpx_sub(disto_at(xr, xi, a), disto_at(xr, xi, s));
}

// second-order drain current at 2 w from the first-order voltages
CSIM_AC_HD inline cpx disto_i2(const double* c, cpx Ug, cpx Ud)
{
    cpx t = cpx_scale(0.5 * c[DC_GG], cpx_mul(Ug, Ug));
    t = cpx_add(t, cpx_scale(c[DC_GD], cpx_mul(Ug, Ud)));
    t = cpx_add(t, cpx_scale(0.5 * c[DC_DD], cpx_mul(Ud, Ud)));
    return cpx_scale(0.5, t);
}

// third-order drain current at 3 w from the first-order (Ug, Ud) and second-order (Ug2, Ud2) voltages
CSIM_AC_HD inline cpx disto_i3(const double* c, cpx Ug, cpx Ud, cpx Ug2, cpx Ud2)
{
    const cpx gg = cpx_mul(Ug, Ug), dd = cpx_mul(Ud, Ud);
    cpx a = cpx_scale(c[DC_GGG] / 6.0, cpx_mul(gg, Ug));
    a = cpx_add(a, cpx_scale(0.5 * c[DC_GGD], cpx_mul(gg, Ud)));
    a = cpx_add(a, cpx_scale(0.5 * c[DC_GDD], cpx_mul(Ug, dd)));
    a = cpx_add(a, cpx_scale(c[DC_DDD] / 6.0, cpx_mul(dd, Ud)));
    cpx b = cpx_scale(c[DC_GG], cpx_mul(Ug, Ug2));
    b = cpx_add(b, cpx_scale(c[DC_GD], cpx_add(cpx_mul(Ug, Ud2), cpx_mul(Ud, Ug2))));
    b = cpx_add(b, cpx_scale(c[DC_DD], cpx_mul(Ud, Ud2)));
    return cpx_add(cpx_scale(0.25, a), cpx_scale(0.5, b));
}

CSIM_AC_HD inline double disto_abs(cpx z) { return sqrt(z.re * z.re + z.im * z.im); }
CSIM_AC_HD inline double disto_hd(double vk, double v1) { return v1 == 0.0 ? 0.0 : vk / v1; }

// Sequential statement of one (system, frequency).  G, C row-major [n][n]; Jr, Ji [n]; devices devD, devG, devS [M]
// (equations, -1 ground) with coef [M][7]; ar, ai work planes of n * ld doubles (ld >= n + 1); x gets 3 * n values
// per part (order k at x[(k - 1) * n]); hd gets HD2, HD3.  Returns CSIM_ST_* flags.
CSIM_AC_HD inline unsigned ac_disto_solve(int n, const double* G, const double* C, const double* Jr, const double* Ji,
                                          double w, int M, const int32_t* devD, const int32_t* devG, const int32_t* devS,
                                          const double* coef, int outP, int outM, double eps, int ld, double* ar,
                                          double* ai, double* xr, double* xi, double* hd)
{
    unsigned flags = 0u;
    bool failed = false;
    for (int k = 1; k <= 3; ++k) {
        const double wk = k == 1 ? w : (double)k * w;
        double* yr = xr + (k - 1) * n;
        double* yi = xi + (k - 1) * n;
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j) {
                ar[i * ld + j] = G[i * n + j];
                ai[i * ld + j] = wk * C[i * n + j];
            }
            ar[i * ld + n] = k == 1 ? Jr[i] : 0.0;
            ai[i * ld + n] = k == 1 ? Ji[i] : 0.0;
        }
        if (k > 1)
            for (int m = 0; m < M; ++m) {
                const int d = devD[m], g = devG[m], s = devS[m];
                const cpx Ug = disto_u(xr, xi, g, s), Ud = disto_u(xr, xi, d, s);
                const cpx I = k == 2 ? disto_i2(coef + m * DISTO_NCOEF, Ug, Ud)
                                     : disto_i3(coef + m * DISTO_NCOEF, Ug, Ud, disto_u(xr + n, xi + n, g, s),
                                                disto_u(xr + n, xi + n, d, s));
                if (d >= 0) { ar[d * ld + n] = ar[d * ld + n] - I.re; ai[d * ld + n] = ai[d * ld + n] - I.im; }
                if (s >= 0) { ar[s * ld + n] = ar[s * ld + n] + I.re; ai[s * ld + n] = ai[s * ld + n] + I.im; }
            }
        const unsigned fl = ac_lu_solve(n, ld, ar, ai, eps, yr, yi);
        flags |= fl;
        failed = failed || fl != 0u;
        if (failed)
            for (int i = 0; i < n; ++i) { yr[i] = 0.0; yi[i] = 0.0; }
    }
    double v[3];
    for (int k = 0; k < 3; ++k) v[k] = disto_abs(disto_u(xr + k * n, xi + k * n, outP, outM));
    hd[0] = disto_hd(v[1], v[0]);
    hd[1] = disto_hd(v[2], v[0]);
    return flags;
}

} // namespace csim
