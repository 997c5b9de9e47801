// pss.hpp -- the arithmetic of the periodic-steady-state analysis, defined ONCE for host and device
// (include/csim.h "Periodic steady state").
//
// The period kernel (kernels_pss.hip) integrates K backward-Euler steps with the general transient's own device
// functions; everything the analysis adds to them that is arithmetic is here, so a host build of this header (the CPU
// tests compile it with g++ -ffp-contract=off) and the kernels compute the same bits:
//
//   K            pss_num_steps(h, f0) = round((1 / f0) / h), refused unless |K h f0 - 1| <= 1e-9 and 1 <= K <= 2^22
//   table        c[j] = cos(2 pi j / K), s[j] = sin(2 pi j / K), j = 0 .. K-1: pss_twiddles(), made once on the host
//   DFT          sums re += x c[(m k) mod K], im += x s[(m k) mod K] for k = 1 .. K ascending, product and sum rounded
//                separately; X[0] = (1/K) re (imaginary part +0.0), X[m] = (2/K) re - j (2/K) im
//   closure      r = x_K - x0, ||r||_inf < tol
//   update       x0 + d, d the solution of (I - W_K) d = r, the matrix formed as (i == j ? 1.0 : 0.0) - W_K(i, j)
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CSIM_PSS_HD __host__ __device__
#else
#define CSIM_PSS_HD
#endif

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

constexpr int64_t PSS_MAX_STEPS = (int64_t)1 << 22;     // bounds the table and keeps tran_time's int cast safe
constexpr double PSS_PI = 3.14159265358979323846;
constexpr int PSS_REFUSED_ARG = -1;                     // CSIM_ERR_ARG
constexpr int PSS_REFUSED_CONFIG = -7;                  // CSIM_ERR_CONFIG

// K, or PSS_REFUSED_*: numbers that are not finite are an argument error, a period the step does not divide (or
// more than PSS_MAX_STEPS steps of it) a configuration error
CSIM_PSS_HD inline int64_t pss_num_steps(double h, double f0)
{
    if (!isfinite(h) || !isfinite(f0)) return PSS_REFUSED_ARG;
    if (!(h > 0.0) || !(f0 > 0.0)) return PSS_REFUSED_CONFIG;
    const double kd = round((1.0 / f0) / h);
    if (!(kd >= 1.0) || kd > (double)PSS_MAX_STEPS) return PSS_REFUSED_CONFIG;
    if (fabs(kd * h * f0 - 1.0) > 1e-9) return PSS_REFUSED_CONFIG;
    return (int64_t)kd;
}

inline void pss_twiddles(int64_t K, double* c, double* s)
{
    for (int64_t j = 0; j < K; ++j) {
        const double ang = 2.0 * PSS_PI * (double)j / (double)K;
        c[j] = cos(ang);
        s[j] = sin(ang);
    }
}

CSIM_PSS_HD inline int pss_tw_index(int m, int64_t k, int64_t K) { return (int)(((int64_t)m * k) % K); }

CSIM_PSS_HD inline void pss_dft_add(double x, double c, double s, double* re, double* im)
{
    const double pc = x * c, ps = x * s;
    *re = *re + pc;
    *im = *im + ps;
}

CSIM_PSS_HD inline void pss_dft_finish(int m, int64_t K, double* re, double* im)
{
    const double scale = (m == 0 ? 1.0 : 2.0) / (double)K;
    const double r = scale * *re, i = scale * *im;
    *re = r;
    *im = m == 0 ? 0.0 : -i;
}

CSIM_PSS_HD inline double pss_residual(double xK, double x0) { return xK - x0; }

CSIM_PSS_HD inline double pss_norm_inf(const double* r, int n)
{
    double m = 0.0;
    for (int i = 0; i < n; ++i) {
        const double a = fabs(r[i]);
        m = a > m ? a : m;
    }
    return m;
}

CSIM_PSS_HD inline bool pss_closed(double norm, double tol) { return norm < tol; }

CSIM_PSS_HD inline double pss_shoot_entry(int i, int j, double w) { return (i == j ? 1.0 : 0.0) - w; }

CSIM_PSS_HD inline double pss_update(double x0, double d) { return x0 + d; }

} // namespace csim
