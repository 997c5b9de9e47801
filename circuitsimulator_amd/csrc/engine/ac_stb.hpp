// ac_stb.hpp -- the arithmetic of the loop-gain analysis, defined ONCE for host and device
// (include/csim.h "Loop-gain analysis").
//
// Middlebrook's double injection at a V source in series in the loop (+ node on the driving side, equation x; - node
// on the receiving side, equation y; branch equation k).  One factorisation per (instance, frequency) of A = G + jwC
// of "AC analysis" with two right-hand sides.  The kernels (kernels_stb.hip) and the sequential routines below share
// ac_lu.hpp's primitives and their order:
//
//   column 0     voltage injection: the real unit vector at row k (an S-parameter port column); vx = X0[x], vy = X0[y]
//   column 1     current injection: +1.0 at row x, what the AC assembly leaves for `Iinj 0 <+node> AC 1` (an I source
//                stamps J(its first node) -= I, J(its second node) += I); ib = X1[k]
//   loop gain    a = 1 - ib, b = 1 + ib (re and im separately, the real 1.0 has im +0.0)
//                num = -(vx a) - (vy ib)        den = (vy b) - (vx ib)        T = num / den
//                the products cpx_mul, the quotient cpx_div, the negation exact
//   failures     A fails its pivot test, or den is exactly zero: T = +0.0 + 0.0j, CSIM_ST_LU_TINY_PIVOT
//   margins      stb_margins(): one walk over the frequencies of an instance (include/csim.h states every step)
#pragma once

#include <math.h>
#include <stddef.h>

#include "ac_lu.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

// T from the three numbers read off the two solutions; `failed`: the factorisation failed.  OR-s into *flags.
CSIM_AC_HD inline cpx stb_loop_gain(cpx vx, cpx vy, cpx ib, bool failed, unsigned* flags)
{
    const cpx a = {1.0 - ib.re, 0.0 - ib.im};
    const cpx b = {1.0 + ib.re, 0.0 + ib.im};
    const cpx p1 = cpx_mul(vx, a);
    const cpx p2 = cpx_mul(vy, ib);
    const cpx num = {-p1.re - p2.re, -p1.im - p2.im};
    const cpx den = cpx_sub(cpx_mul(vy, b), cpx_mul(vx, ib));
    if (failed || cpx_is_zero(den)) {
        *flags |= CSIM_ST_LU_TINY_PIVOT;
        return {0.0, 0.0};
    }
    return cpx_div(num, den);
}

// Sequential statement of one (system, frequency).  G, C row-major [n][n]; eqP, eqM, eqBr the probe's equations; ar, ai
// work planes of n * ld doubles (ld >= n + 2); xr, xi get 2 * n values (solution c at c * n); T gets re, im.
// Returns CSIM_ST_* flags.
CSIM_AC_HD inline unsigned ac_stb_solve(int n, const double* G, const double* C, double w, int eqP, int eqM, int eqBr,
                                        double eps, int ld, double* ar, double* ai, double* xr, double* xi, double* T)
{
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            ar[i * ld + j] = G[i * n + j];
            ai[i * ld + j] = w * C[i * n + j];
        }
        ar[i * ld + n] = i == eqBr ? 1.0 : 0.0;
        ai[i * ld + n] = 0.0;
        ar[i * ld + n + 1] = i == eqP ? 1.0 : 0.0;
        ai[i * ld + n + 1] = 0.0;
    }
    unsigned fl = ac_lu_solve_multi(n, 2, ld, ar, ai, eps, xr, xi, n);
    const cpx t = stb_loop_gain({xr[eqP], xi[eqP]}, {xr[eqM], xi[eqM]}, {xr[n + eqBr], xi[n + eqBr]}, fl != 0u, &fl);
    T[0] = t.re;
    T[1] = t.im;
    return fl;
}

// ---- margins
enum { STB_FOUND_UNITY = 1, STB_FOUND_PHASE = 2 };
constexpr double STB_PI = 3.14159265358979323846;

struct StbMargins { double pm, fc, gm, f180; int found; };

// f(k-1) * exp(t * log(f(k) / f(k-1))): the crossing between two grid points, linear in log f
CSIM_AC_HD inline double stb_interp_freq(double f0, double f1, double t) { return f0 * exp(t * log(f1 / f0)); }

// The margins of one instance from T(0) .. T(F-1) at strictly increasing positive frequencies (Hz).  T(k) is at
// t[2 * k * stride] (re) and t[2 * k * stride + 1] (im).  A pair that is not found is NaN.
CSIM_AC_HD inline StbMargins stb_margins(int F, const double* freqs, const double* t, size_t stride)
{
    const double nan = NAN;
    StbMargins r = {nan, nan, nan, nan, 0};
    cpx prev = {0.0, 0.0};
    double mp = 0.0, gp = 0.0, pp = 0.0;
    for (int k = 0; k < F; ++k) {
        const cpx T = {t[2 * (size_t)k * stride], t[2 * (size_t)k * stride + 1]};
        if (cpx_is_zero(T) || !isfinite(T.re) || !isfinite(T.im)) break;
        const double m = cpx_abs2(T);
        const double g = 10.0 * log10(m);
        double d = 0.0, p;
        if (k == 0) {
            p = atan2(T.im, T.re);
        } else {
            const cpx q = cpx_mul(T, {prev.re, -prev.im});
            d = atan2(q.im, q.re);
            p = pp + d;
            if (!(r.found & STB_FOUND_UNITY) && mp >= 1.0 && 1.0 > m) {
                const double u = gp / (gp - g);
                r.fc = stb_interp_freq(freqs[k - 1], freqs[k], u);
                r.pm = 180.0 + (pp + u * d) * 180.0 / STB_PI;
                r.found |= STB_FOUND_UNITY;
            }
            if (!(r.found & STB_FOUND_PHASE) && pp > -STB_PI && -STB_PI >= p) {
                const double u = (pp + STB_PI) / (pp - p);
                r.f180 = stb_interp_freq(freqs[k - 1], freqs[k], u);
                r.gm = -(gp + u * (g - gp));
                r.found |= STB_FOUND_PHASE;
            }
        }
        prev = T;
        mp = m;
        gp = g;
        pp = p;
    }
    return r;
}

} // namespace csim
