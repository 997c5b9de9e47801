// ac_lu.hpp -- the arithmetic of the AC small-signal solve, defined ONCE for host and device.
//
// The AC kernels (kernels_ac.hip) factor (G + jwC) v = J, complex, with partial pivoting in the shape
// of Solver::solveLinearSystemLU (include/solver.hpp:30-131).  Both of them -- the wave-per-system
// kernel (matrix in LDS) and the register-resident kernel (matrix in registers) -- call the primitives
// below and apply them to every entry in the same order, so their results are bit-identical; the
// sequential ac_lu_solve() states that order and is what the host tests compile (g++ -ffp-contract=off).
//
//   pivot        the FIRST row (ascending) with the largest re^2 + im^2 (strict '>'); a NaN diagonal
//                keeps the pivot; a maximum below lu_eps^2 fails the system: zero vector,
//                CSIM_ST_LU_TINY_PIVOT
//   multiplier   l = a * conj(p) * (1 / (pr^2 + pi^2))            (one true division)
//   elimination  a(i,j) -= l(i) * u(j) for j > k and the RHS; rows whose multiplier is exactly zero
//                are skipped (a - 0*u == a for finite u)
//   back subst.  x(i) = (y(i) - sum_{j>i, ascending} U(i,j) x(j)) / U(i,i), the division as above
//
// std::complex / hipDoubleComplex division is not used: host and device implement it differently.
#pragma once

#include <stdint.h>

#include "csim_ir.h"

#if defined(__HIPCC__)
#define CSIM_AC_HD __host__ __device__
#else
#define CSIM_AC_HD
#endif

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

struct cpx { double re, im; };

CSIM_AC_HD inline cpx cpx_mul(cpx a, cpx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
CSIM_AC_HD inline cpx cpx_sub(cpx a, cpx b) { return {a.re - b.re, a.im - b.im}; }
CSIM_AC_HD inline double cpx_abs2(cpx a) { return a.re * a.re + a.im * a.im; }
// a / p as a * conj(p) * (1 / |p|^2)
CSIM_AC_HD inline cpx cpx_div(cpx a, cpx p)
{
    const double inv = 1.0 / (p.re * p.re + p.im * p.im);
    return {(a.re * p.re + a.im * p.im) * inv, (a.im * p.re - a.re * p.im) * inv};
}
CSIM_AC_HD inline bool cpx_is_zero(cpx a) { return a.re == 0.0 && a.im == 0.0; }
// one elimination update a - l * u
CSIM_AC_HD inline cpx cpx_elim(cpx a, cpx l, cpx u) { return cpx_sub(a, cpx_mul(l, u)); }

// Sequential statement of the solve on a row-major augmented matrix: re/im planes, row i at i * ld,
// RHS in column n (ld >= n + 1).  Overwrites the planes; x gets n values.  Returns CSIM_ST_* flags.
CSIM_AC_HD inline unsigned ac_lu_solve(int n, int ld, double* ar, double* ai, double eps, double* xr, double* xi)
{
    const double eps2 = eps * eps;
    for (int k = 0; k < n; ++k) {
        int piv = k;
        double maxv = cpx_abs2({ar[k * ld + k], ai[k * ld + k]});
        if (maxv == maxv) {
            for (int i = k + 1; i < n; ++i) {
                const double v = cpx_abs2({ar[i * ld + k], ai[i * ld + k]});
                if (v > maxv) { maxv = v; piv = i; }
            }
        }
        if (maxv < eps2) {
            for (int i = 0; i < n; ++i) { xr[i] = 0.0; xi[i] = 0.0; }
            return CSIM_ST_LU_TINY_PIVOT;
        }
        if (piv != k)
            for (int j = k; j <= n; ++j) {
                double t = ar[k * ld + j]; ar[k * ld + j] = ar[piv * ld + j]; ar[piv * ld + j] = t;
                t = ai[k * ld + j]; ai[k * ld + j] = ai[piv * ld + j]; ai[piv * ld + j] = t;
            }
        const cpx p = {ar[k * ld + k], ai[k * ld + k]};
        for (int i = k + 1; i < n; ++i) {
            const cpx l = cpx_div({ar[i * ld + k], ai[i * ld + k]}, p);
            if (cpx_is_zero(l)) continue;
            for (int j = k + 1; j <= n; ++j) {
                const cpx r = cpx_elim({ar[i * ld + j], ai[i * ld + j]}, l, {ar[k * ld + j], ai[k * ld + j]});
                ar[i * ld + j] = r.re;
                ai[i * ld + j] = r.im;
            }
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        cpx s = {ar[i * ld + n], ai[i * ld + n]};
        for (int j = i + 1; j < n; ++j) s = cpx_sub(s, cpx_mul({ar[i * ld + j], ai[i * ld + j]}, {xr[j], xi[j]}));
        const cpx x = cpx_div(s, {ar[i * ld + i], ai[i * ld + i]});
        xr[i] = x.re;
        xi[i] = x.im;
    }
    return 0u;
}

} // namespace csim
