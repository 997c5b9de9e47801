// pac.hpp -- the arithmetic of the periodic AC analysis, defined ONCE for host and device
// (include/csim.h "Periodic AC analysis").
//
// The period kernel (kernels_pac.hip) integrates the orbit with the general transient's own device functions and
// solves every step's linear system with the engine's real LU on 2 Fc real columns; the closure goes through the
// engine's complex LU (ac_lu.hpp).  Everything else the analysis computes is here, so a host build of this header (the
// CPU tests compile it with g++ -ffp-contract=off) and the kernels compute the same bits:
//
//   z            cos(theta) - j sin(theta), theta = 2 pi f h; z_K the same with theta_K = 2 pi (f / f0 - floor(f / f0)):
//                pac_z(), made on the host in double, z_K never by powering z
//   product      q = sum over the non-zero Hm(i, l), l ascending, of Hm(i, l) p(l): product and sum rounded separately,
//                real and imaginary columns on their own (pac_hm_add)
//   step         J_k p_k = z q + u: re = (zr qr - zi qi) + ur, im = (zr qi + zi qr) + ui (pac_step_rhs)
//   closure      (I - z_K W_K) p_0 = r_K, entry (i, j) = ((i == j ? 1 : 0) - zKr w) + j (0 - zKi w) (pac_close_entry)
//   sidebands    re += pr c + pi s, im += pi c - pr s with c, s = the table at j = ((m k) mod K + K) mod K, k = 1 .. K
//                ascending; P_m = (1 / K) (re + j im): one division, the scale multiplies the finished sums
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CSIM_PAC_HD __host__ __device__
#else
#define CSIM_PAC_HD
#endif

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

constexpr double PAC_PI = 3.14159265358979323846;
constexpr int PAC_MAX_FC = 32;                          // frequencies per launch: 2 Fc real columns, one per lane
constexpr size_t PAC_LDS_LIMIT = 160 * 1024;            // bytes of LDS a workgroup of the period kernel may take

// z = e^{-j 2 pi f h} and z_K = e^{-j 2 pi f / f0} = z^K, the latter from the fractional part of f / f0
inline void pac_z(double f, double h, double f0, double* zr, double* zi, double* zKr, double* zKi)
{
    const double th = 2.0 * PAC_PI * f * h;
    *zr = cos(th);
    *zi = -sin(th);
    const double ratio = f / f0;
    const double thK = 2.0 * PAC_PI * (ratio - floor(ratio));
    *zKr = cos(thK);
    *zKi = -sin(thK);
}

CSIM_PAC_HD inline int pac_tw_index(int m, int64_t k, int64_t K) { return (int)((((int64_t)m * k) % K + K) % K); }

CSIM_PAC_HD inline double pac_hm_add(double acc, double h, double p)
{
    const double t = h * p;
    return acc + t;
}

CSIM_PAC_HD inline void pac_step_rhs(double zr, double zi, double qr, double qi, double ur, double ui, double* re, double* im)
{
    const double a = zr * qr, b = zi * qi;
    const double t = a - b;
    *re = t + ur;
    const double c = zr * qi, d = zi * qr;
    const double v = c + d;
    *im = v + ui;
}

CSIM_PAC_HD inline void pac_close_entry(int i, int j, double w, double zKr, double zKi, double* re, double* im)
{
    const double a = zKr * w, b = zKi * w;
    *re = (i == j ? 1.0 : 0.0) - a;
    *im = 0.0 - b;
}

CSIM_PAC_HD inline void pac_sum_add(double pr, double pi, double c, double s, double* re, double* im)
{
    const double a = pr * c, b = pi * s;
    const double t = a + b;
    *re = *re + t;
    const double d = pi * c, e = pr * s;
    const double v = d - e;
    *im = *im + v;
}

CSIM_PAC_HD inline void pac_sum_finish(int64_t K, double* re, double* im)
{
    const double scale = 1.0 / (double)K;
    const double r = scale * *re, i = scale * *im;
    *re = r;
    *im = i;
}

} // namespace csim
