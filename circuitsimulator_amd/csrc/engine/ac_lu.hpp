// ac_lu.hpp -- the arithmetic of the complex small-signal solve, defined ONCE for host and device.
//
// The AC, noise and S-parameter kernels (kernels_ac.hip, kernels_noise.hip, kernels_sp.hip through ac_sweep.hpp)
// factor A = G + jwC, complex, with partial pivoting in the shape of Solver::solveLinearSystemLU
// (include/solver.hpp:30-131), carrying K >= 1 right-hand sides as the columns n .. n+K-1.  Both kernel shapes --
// wave per system (matrix in LDS) and register-resident (matrix in registers) -- call the primitives below and apply
// them to every entry in the same order, so their results are bit-identical; the sequential ac_lu_solve_multi()
// states that order and is what the host tests compile (g++ -ffp-contract=off).  AC and noise are K = 1.
//
//   pivot        the FIRST row (ascending) with the largest re^2 + im^2 (strict '>'); a NaN diagonal
//                keeps the pivot; a maximum below lu_eps^2 fails the system: all K vectors zero,
//                CSIM_ST_LU_TINY_PIVOT.  Pivoting never looks at a right-hand side: column c of the result is
//                bit for bit the single-RHS solve with that column alone.
//   multiplier   l = a * conj(p) * (1 / (pr^2 + pi^2))            (one true division)
//   elimination  a(i,j) -= l(i) * u(j) for j = k+1 .. n+K-1; rows whose multiplier is exactly zero
//                are skipped (a - 0*u == a for finite u)
//   back subst.  per column: x(i) = (y(i) - sum_{j>i, ascending} U(i,j) x(j)) / U(i,i), the division as above
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

// Sequential statement of the solve on a row-major augmented matrix with K right-hand sides: re/im planes, row i at
// i * ld, RHS c in column n + c (ld >= n + K).  Overwrites the planes; solution c goes to xr/xi[c * ldx + 0 .. n-1].
// Returns CSIM_ST_* flags.
CSIM_AC_HD inline unsigned ac_lu_solve_multi(int n, int K, int ld, double* ar, double* ai, double eps, double* xr,
                                             double* xi, int ldx)
{
    const double eps2 = eps * eps;
    const int w = n + K;
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
            for (int c = 0; c < K; ++c)
                for (int i = 0; i < n; ++i) { xr[c * ldx + i] = 0.0; xi[c * ldx + i] = 0.0; }
            return CSIM_ST_LU_TINY_PIVOT;
        }
        if (piv != k)
            for (int j = k; j < w; ++j) {
                double t = ar[k * ld + j]; ar[k * ld + j] = ar[piv * ld + j]; ar[piv * ld + j] = t;
                t = ai[k * ld + j]; ai[k * ld + j] = ai[piv * ld + j]; ai[piv * ld + j] = t;
            }
        const cpx p = {ar[k * ld + k], ai[k * ld + k]};
        for (int i = k + 1; i < n; ++i) {
            const cpx l = cpx_div({ar[i * ld + k], ai[i * ld + k]}, p);
            if (cpx_is_zero(l)) continue;
            for (int j = k + 1; j < w; ++j) {
                const cpx r = cpx_elim({ar[i * ld + j], ai[i * ld + j]}, l, {ar[k * ld + j], ai[k * ld + j]});
                ar[i * ld + j] = r.re;
                ai[i * ld + j] = r.im;
            }
        }
    }
    for (int c = 0; c < K; ++c)
        for (int i = n - 1; i >= 0; --i) {
            cpx s = {ar[i * ld + n + c], ai[i * ld + n + c]};
            for (int j = i + 1; j < n; ++j)
                s = cpx_sub(s, cpx_mul({ar[i * ld + j], ai[i * ld + j]}, {xr[c * ldx + j], xi[c * ldx + j]}));
            const cpx x = cpx_div(s, {ar[i * ld + i], ai[i * ld + i]});
            xr[c * ldx + i] = x.re;
            xi[c * ldx + i] = x.im;
        }
    return 0u;
}

// the single-RHS solve: RHS in column n (ld >= n + 1), x gets n values
CSIM_AC_HD inline unsigned ac_lu_solve(int n, int ld, double* ar, double* ai, double eps, double* xr, double* xi)
{
    return ac_lu_solve_multi(n, 1, ld, ar, ai, eps, xr, xi, n);
}

} // namespace csim
