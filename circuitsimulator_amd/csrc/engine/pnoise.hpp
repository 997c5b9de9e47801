// pnoise.hpp -- the arithmetic of the periodic noise analysis, defined ONCE for host and device
// (include/csim.h "Periodic noise analysis").
//
// The period kernel (kernels_pnoise.hip) runs the adjoint of the periodic AC recursion backwards over the stored orbit
// and solves every step's transposed system with the engine's real LU on 2 Fc real columns; the closure goes through
// the engine's complex LU (ac_lu.hpp).  z, z_K, the table index, the product's step and the scale are pac.hpp's (pac_z,
// pac_tw_index, pac_hm_add, pac_sum_finish).  Everything else the analysis computes is here, so a host build of this
// header (the CPU tests compile it with g++ -ffp-contract=off) and the kernels compute the same bits:
//
//   product      g(i) = sum over the non-zero Hm(l, i), l ascending, of Hm(l, i) q(l): product and sum rounded
//                separately, real and imaginary columns on their own (pac_hm_add)
//   step         J_k^T q_k = z g_k + d: re = (zr gr - zi gi) + d, im = (zr gi + zi gr) + 0.0 (pnoise_step_rhs)
//   closure      (I - z_K W_K^T) g_K = r, entry (i, j) = pac_close_entry(i, j, W_K(j, i)) (pnoise_close_entry)
//   generators   psd = kT4 (1 / R), 0 for R == 0 (pnoise_psd_r); psd = kT4 ((2 / 3) |gg|) (pnoise_psd_mos);
//                sigma = sqrt(psd) (pnoise_sigma)
//   transfers    w = sigma (q(a) - q(b)), ground = 0, re and im one product each; re += wr c - wi s,
//                im += wi c + wr s with c, s = the table at j = ((m k) mod K + K) mod K, k = K .. 1 DESCENDING (the order
//                the kernel visits the steps); T = (1 / K) (re + j im), the scale multiplies the finished sums
//                (pac_sum_finish)
//   outputs      |T|^2 = re re + im im (pnoise_abs2); contrib(s) = 0.0 + sum_m |T(s, m)|^2, m ascending;
//                side(m) = 0.0 + sum_s |T(s, m)|^2, s ascending; onoise = 0.0 + sum_s contrib(s), s ascending
#pragma once

#include "pac.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

// bytes of device memory the stored orbit of one instance chunk may take: chunk * K * N * 8 stays at or below it
constexpr size_t PNOISE_ORBIT_BUDGET = (size_t)256 << 20;

CSIM_PAC_HD inline void pnoise_step_rhs(double zr, double zi, double gr, double gi, double d, double* re, double* im)
{
    pac_step_rhs(zr, zi, gr, gi, d, 0.0, re, im);
}

// entry (i, j) of I - z_K W^T; W row-major [N][N]
CSIM_PAC_HD inline void pnoise_close_entry(int i, int j, int N, const double* W, double zKr, double zKi, double* re, double* im)
{
    pac_close_entry(i, j, W[j * N + i], zKr, zKi, re, im);
}

CSIM_PAC_HD inline double pnoise_psd_r(double kT4, double R) { return (R == 0.0) ? 0.0 : kT4 * (1.0 / R); }
CSIM_PAC_HD inline double pnoise_psd_mos(double kT4, double gg) { return kT4 * ((2.0 / 3.0) * fabs(gg)); }
CSIM_PAC_HD inline double pnoise_sigma(double psd) { return sqrt(psd); }

// q(a) - q(b) of one frequency in the plane q [N][R] (re at column 2 f, im at 2 f + 1); equation -1 is ground
CSIM_PAC_HD inline void pnoise_diff(const double* q, int R, int f, int a, int b, double* dr, double* di)
{
    const double ar = a >= 0 ? q[a * R + 2 * f] : 0.0, ai = a >= 0 ? q[a * R + 2 * f + 1] : 0.0;
    const double br = b >= 0 ? q[b * R + 2 * f] : 0.0, bi = b >= 0 ? q[b * R + 2 * f + 1] : 0.0;
    *dr = ar - br;
    *di = ai - bi;
}

// one step's term of a transfer sum: w = sigma (dr + j di), sum += w (c + j s)
CSIM_PAC_HD inline void pnoise_sum_add(double sigma, double dr, double di, double c, double s, double* re, double* im)
{
    const double wr = sigma * dr, wi = sigma * di;
    const double a = wr * c, b = wi * s;
    const double t = a - b;
    *re = *re + t;
    const double d = wi * c, e = wr * s;
    const double v = d + e;
    *im = *im + v;
}

CSIM_PAC_HD inline double pnoise_abs2(double re, double im)
{
    const double a = re * re, b = im * im;
    return a + b;
}

} // namespace csim
