// pz.hpp -- the arithmetic of the pole analysis, defined ONCE for host and device (include/csim.h "Pole analysis").
//
// The poles of an instance are the finite generalised eigenvalues of (G, C) of "AC analysis": s with det(G + sC) = 0.
// The kernel (kernels_pz.hip) and the sequential pz_poles() below apply the same primitives to every entry in the same
// order, so a host build of this header (the CPU tests compile it with g++ -ffp-contract=off) and the kernel compute
// the same bits.  All arithmetic is real; sqrt is the only library function.
//
//   A0           G + sigma0 * C, one product and one sum per entry (pz_shift)
//   M            -A0^-1 C by a real LU with partial pivoting on [A0 | C], the N columns of C as right-hand sides, in the
//                shape of lu_solve_multi_wave (device_common.hpp): pivot = largest |a|, the lowest row on ties, a NaN
//                diagonal keeps the pivot; a column maximum below lu_eps is CSIM_ST_PZ_SINGULAR; rows whose entry in the
//                pivot column is exactly zero are skipped; back substitution per column with the products U(i,l) x(l)
//                subtracted for l ascending, zero U(i,l) skipped; then the negation
//   balance      Gauss-Seidel sweeps over i = 0 .. n-1 in index order (EISPACK balanc without its permutations): c and r
//                the sums of |M(j,i)| and |M(i,j)| over j != i, j ascending; f a power of two by pz_balance_factor();
//                row i times 1/f, then column i times f, before the next index is looked at.  The sweeps end when one
//                changes nothing, or after PZ_BALANCE_SWEEPS of them
//   elmhes       per column m-1: pivot = largest |a(j,m-1)| over j = m .. n-1, the lowest index on ties; rows, then
//                columns m and the pivot's exchanged; y(i) = a(i,m-1) / x stored in place; ROW phase a(i,j) -= y(i) a(m,j)
//                for every i > m and j >= m; then COLUMN phase a(j,m) += y(i) a(j,i) for every row j, i ascending, zero
//                y(i) skipped.  Afterwards the entries below the subdiagonal are set to +0.0
//   hqr          Francis double-shift QR as in EISPACK hqr: deflation test |h(l,l-1)| + s == s, exceptional shifts at
//                iterations 10 and 20, CSIM_ST_PZ_NONCONV at iteration 30.  Per bulge step k the reflector's scalars
//                come from pz_hqr_reflector(); the ROW phase (pz_hqr_row, columns k .. nn) is finished before the
//                COLUMN phase (pz_hqr_col, rows l .. min(nn, k+3)) starts
//   cut          an eigenvalue mu of M is a finite pole iff (mur^2 + mui^2) * wmax^2 >= 1.0, wmax = 2 pi fmax
//   pole         s = sigma0 + conj(mu) / (mur^2 + mui^2): re = sigma0 + mur / m2, im = (0.0 - mui) / m2
//   order        descending m2, then descending Im mu, then descending Re mu, then the eigenvalue's index (pz_before);
//                slot = the number of finite poles that come before
//   summary      n_poles; n_rhp = the count with Re s > 0.0; max_re = the largest Re s walking the slots in order (NaN
//                when n_poles == 0).  Slots n_poles .. n-1 are NaN + NaN j; on a flag every slot is
#pragma once

#include <math.h>
#include <stddef.h>

#include "ac_lu.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace csim {

constexpr double PZ_PI = 3.14159265358979323846;       // as STB_PI (ac_stb.hpp)
constexpr int PZ_MAX_N = 63;
constexpr int PZ_BALANCE_SWEEPS = 16;
constexpr int PZ_HQR_ITS = 30;

CSIM_AC_HD inline double pz_wmax(double fmax) { return 2.0 * PZ_PI * fmax; }

CSIM_AC_HD inline double pz_shift(double g, double c, double sigma0)
{
    const double p = sigma0 * c;
    return g + p;
}

CSIM_AC_HD inline double pz_sign(double a, double b) { return b >= 0.0 ? fabs(a) : -fabs(a); }

// ---- balancing: the factor of index i from its column sum c and row sum r (both off-diagonal); 1.0 = leave it
CSIM_AC_HD inline double pz_balance_factor(double c, double r)
{
    if (!(c > 0.0) || !(r > 0.0) || !isfinite(c) || !isfinite(r)) return 1.0;
    const double s = c + r;
    double f = 1.0, g = r / 2.0;
    while (c < g) { f = f * 2.0; c = c * 4.0; }
    g = r * 2.0;
    while (c > g) { f = f / 2.0; c = c / 4.0; }
    return (c + r) / f < 0.95 * s ? f : 1.0;
}

// ---- elmhes
CSIM_AC_HD inline double pz_elm_row(double a, double y, double am) { const double p = y * am; return a - p; }
CSIM_AC_HD inline double pz_elm_col(double a, double y, double ai) { const double p = y * ai; return a + p; }

// ---- hqr: the scalars of one bulge step
struct PzReflector { double p, q, r, x, y, z; bool three; };

// Householder scalars of step k from the column (p, q, r) it annihilates.  `first`: k == m, (p, q, r) come from the
// shift; otherwise they are a(k,k-1), a(k+1,k-1), a(k+2,k-1) and are scaled here.  Returns false when the step does
// nothing (s == 0).  *sub gets what a(k,k-1) becomes; *setSub whether it is written at all.
CSIM_AC_HD inline bool pz_hqr_reflector(bool first, bool lIsM, double akk1, double p, double q, double r, PzReflector* h,
                                        double* sub, bool* setSub)
{
    double x = 0.0;
    *setSub = false;
    if (!first) {
        x = fabs(p) + fabs(q) + fabs(r);
        if (x != 0.0) { p = p / x; q = q / x; r = r / x; }
    }
    const double s = pz_sign(sqrt(p * p + q * q + r * r), p);
    if (s == 0.0 || s != s) return false;
    if (first) {
        if (!lIsM) { *sub = -akk1; *setSub = true; }
    } else {
        *sub = -s * x;
        *setSub = true;
    }
    p = p + s;
    h->x = p / s;
    h->y = q / s;
    h->z = r / s;
    h->q = q / p;
    h->r = r / p;
    h->p = p;
    return true;
}

// row phase on column j: rows k, k+1 (and k+2 when `three`)
CSIM_AC_HD inline void pz_hqr_row(const PzReflector& h, double* a0, double* a1, double* a2)
{
    double p = *a0 + h.q * *a1;
    if (h.three) {
        p = p + h.r * *a2;
        *a2 = *a2 - p * h.z;
    }
    *a1 = *a1 - p * h.y;
    *a0 = *a0 - p * h.x;
}

// column phase on row i: columns k, k+1 (and k+2 when `three`)
CSIM_AC_HD inline void pz_hqr_col(const PzReflector& h, double* a0, double* a1, double* a2)
{
    double p = h.x * *a0 + h.y * *a1;
    if (h.three) {
        p = p + h.z * *a2;
        *a2 = *a2 - p * h.r;
    }
    *a1 = *a1 - p * h.q;
    *a0 = *a0 - p;
}

// the two phases on the matrix: at = &a(k,j) with rows ld apart, at = &a(i,k) with columns one apart
CSIM_AC_HD inline void pz_hqr_row_at(const PzReflector& h, double* at, int ld)
{
    double a0 = at[0], a1 = at[ld], a2 = h.three ? at[2 * ld] : 0.0;
    pz_hqr_row(h, &a0, &a1, &a2);
    at[0] = a0;
    at[ld] = a1;
    if (h.three) at[2 * ld] = a2;
}
CSIM_AC_HD inline void pz_hqr_col_at(const PzReflector& h, double* at)
{
    double a0 = at[0], a1 = at[1], a2 = h.three ? at[2] : 0.0;
    pz_hqr_col(h, &a0, &a1, &a2);
    at[0] = a0;
    at[1] = a1;
    if (h.three) at[2] = a2;
}

// anorm is the sum over the rows, ascending, of these: |a(i,j)| summed over j = max(i-1, 0) .. n-1, ascending
CSIM_AC_HD inline double pz_hess_row_norm(const double* a, int ld, int n, int i)
{
    double s = 0.0;
    for (int j = (i > 0 ? i - 1 : 0); j < n; ++j) s = s + fabs(a[i * ld + j]);
    return s;
}

// the deflation search: the largest l >= 1 from nn downwards with a negligible a(l,l-1), or 0
CSIM_AC_HD inline int pz_hqr_find_l(const double* a, int ld, int nn, double anorm)
{
    int l = nn;
    for (; l >= 1; --l) {
        double s = fabs(a[(l - 1) * ld + l - 1]) + fabs(a[l * ld + l]);
        if (s == 0.0) s = anorm;
        if (fabs(a[l * ld + l - 1]) + s == s) break;
    }
    return l;
}

// the two eigenvalues of the trailing 2 x 2 block: x = a(nn,nn), y = a(nn-1,nn-1), w = a(nn,nn-1) a(nn-1,nn), t the shift
CSIM_AC_HD inline void pz_hqr_pair(double x, double y, double w, double t, double* wr, double* wi)   // [0]: nn-1, [1]: nn
{
    const double p = 0.5 * (y - x);
    const double q = p * p + w;
    double z = sqrt(fabs(q));
    x = x + t;
    if (q >= 0.0) {
        z = p + pz_sign(z, p);
        wr[0] = wr[1] = x + z;
        if (z != 0.0) wr[1] = x - w / z;
        wi[0] = wi[1] = 0.0;
    } else {
        wr[0] = wr[1] = x + p;
        wi[0] = z;
        wi[1] = -z;
    }
}

// the start m of the bulge and the first column (p, q, r), from the shift (x, y, w)
CSIM_AC_HD inline int pz_hqr_start(const double* a, int ld, int l, int nn, double x, double y, double w, double* p, double* q,
                                   double* r)
{
    int m = nn - 2;
    for (; m >= l; --m) {
        const double z = a[m * ld + m];
        double rr = x - z, s = y - z;
        *p = (rr * s - w) / a[(m + 1) * ld + m] + a[m * ld + m + 1];
        *q = a[(m + 1) * ld + m + 1] - z - rr - s;
        *r = a[(m + 2) * ld + m + 1];
        s = fabs(*p) + fabs(*q) + fabs(*r);
        *p = *p / s;
        *q = *q / s;
        *r = *r / s;
        if (m == l) break;
        const double u = fabs(a[m * ld + m - 1]) * (fabs(*q) + fabs(*r));
        const double v = fabs(*p) * (fabs(a[(m - 1) * ld + m - 1]) + fabs(z) + fabs(a[(m + 1) * ld + m + 1]));
        if (u + v == v) break;
    }
    return m;
}

// ---- epilogue
CSIM_AC_HD inline double pz_mag2(double mr, double mi) { return mr * mr + mi * mi; }
CSIM_AC_HD inline bool pz_finite_pole(double m2, double wmax) { return m2 * (wmax * wmax) >= 1.0; }
CSIM_AC_HD inline cpx pz_pole(double mr, double mi, double m2, double sigma0) { return {sigma0 + mr / m2, (0.0 - mi) / m2}; }
// does eigenvalue a (index ia) come before eigenvalue b (index ib)?
CSIM_AC_HD inline bool pz_before(double m2a, double mra, double mia, int ia, double m2b, double mrb, double mib, int ib)
{
    if (m2a != m2b) return m2a > m2b;
    if (mia != mib) return mia > mib;
    if (mra != mrb) return mra > mrb;
    return ia < ib;
}

// ---- sequential statements ----------------------------------------------------------------------------------------

// [A | M] -> A^-1 M in M (A n x n at lda, M n x n at ldm, both row-major); false: singular
CSIM_AC_HD inline bool pz_lu_solve(int n, double* A, int lda, double* M, int ldm, double eps)
{
    for (int k = 0; k < n; ++k) {
        int piv = k;
        double maxAbs = fabs(A[k * lda + k]);
        if (maxAbs == maxAbs)
            for (int i = k + 1; i < n; ++i) {
                const double v = fabs(A[i * lda + k]);
                if (v > maxAbs) { maxAbs = v; piv = i; }
            }
        if (maxAbs < eps) return false;
        if (piv != k) {
            for (int j = k; j < n; ++j) { const double t = A[k * lda + j]; A[k * lda + j] = A[piv * lda + j]; A[piv * lda + j] = t; }
            for (int j = 0; j < n; ++j) { const double t = M[k * ldm + j]; M[k * ldm + j] = M[piv * ldm + j]; M[piv * ldm + j] = t; }
        }
        const double pivv = A[k * lda + k];
        for (int i = k + 1; i < n; ++i) {
            const double c = A[i * lda + k];
            if (c == 0.0) continue;
            const double f = c / pivv;
            for (int j = k + 1; j < n; ++j) A[i * lda + j] -= f * A[k * lda + j];
            for (int j = 0; j < n; ++j) M[i * ldm + j] -= f * M[k * ldm + j];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        const double d = A[i * lda + i];
        for (int c = 0; c < n; ++c) {
            double sum = M[i * ldm + c];
            for (int l = i + 1; l < n; ++l) {
                const double u = A[i * lda + l];
                if (u != 0.0) sum -= u * M[l * ldm + c];
            }
            M[i * ldm + c] = sum / d;
        }
    }
    return true;
}

// balancing in place; scale[i] (may be null) gets D(i,i): the result is D^-1 M D.  Returns the number of sweeps.
CSIM_AC_HD inline int pz_balance(int n, double* a, int ld, double* scale)
{
    if (scale)
        for (int i = 0; i < n; ++i) scale[i] = 1.0;
    int sweeps = 0;
    for (; sweeps < PZ_BALANCE_SWEEPS; ++sweeps) {
        bool changed = false;
        for (int i = 0; i < n; ++i) {
            double c = 0.0, r = 0.0;
            for (int j = 0; j < n; ++j) {
                c = c + (j == i ? 0.0 : fabs(a[j * ld + i]));
                r = r + (j == i ? 0.0 : fabs(a[i * ld + j]));
            }
            const double f = pz_balance_factor(c, r);
            if (f == 1.0) continue;
            const double g = 1.0 / f;
            changed = true;
            if (scale) scale[i] = scale[i] * f;
            for (int j = 0; j < n; ++j) a[i * ld + j] = a[i * ld + j] * g;
            for (int j = 0; j < n; ++j) a[j * ld + i] = a[j * ld + i] * f;
        }
        if (!changed) break;
    }
    return sweeps;
}

CSIM_AC_HD inline void pz_elmhes(int n, double* a, int ld)
{
    for (int m = 1; m < n - 1; ++m) {
        double best = 0.0;
        int piv = m;
        for (int j = m; j < n; ++j) {
            const double v = fabs(a[j * ld + m - 1]);
            if (v > best) { best = v; piv = j; }
        }
        if (!(best > 0.0)) continue;
        if (piv != m) {
            for (int j = m - 1; j < n; ++j) { const double t = a[piv * ld + j]; a[piv * ld + j] = a[m * ld + j]; a[m * ld + j] = t; }
            for (int j = 0; j < n; ++j) { const double t = a[j * ld + piv]; a[j * ld + piv] = a[j * ld + m]; a[j * ld + m] = t; }
        }
        const double x = a[m * ld + m - 1];
        for (int i = m + 1; i < n; ++i) {                       // row phase
            double y = a[i * ld + m - 1];
            if (y == 0.0) continue;
            y = y / x;
            a[i * ld + m - 1] = y;
            for (int j = m; j < n; ++j) a[i * ld + j] = pz_elm_row(a[i * ld + j], y, a[m * ld + j]);
        }
        for (int j = 0; j < n; ++j)                             // column phase
            for (int i = m + 1; i < n; ++i) {
                const double y = a[i * ld + m - 1];
                if (y != 0.0) a[j * ld + m] = pz_elm_col(a[j * ld + m], y, a[j * ld + i]);
            }
    }
    for (int i = 2; i < n; ++i)
        for (int j = 0; j < i - 1; ++j) a[i * ld + j] = 0.0;
}

// the eigenvalues of an upper Hessenberg matrix (destroyed) into wr, wi; 0 or CSIM_ST_PZ_NONCONV
CSIM_AC_HD inline unsigned pz_hqr(int n, double* a, int ld, double* wr, double* wi)
{
    double anorm = 0.0;
    for (int i = 0; i < n; ++i) anorm = anorm + pz_hess_row_norm(a, ld, n, i);
    int nn = n - 1;
    double t = 0.0;
    while (nn >= 0) {
        int its = 0, l;
        do {
            l = pz_hqr_find_l(a, ld, nn, anorm);
            if (l >= 1) a[l * ld + l - 1] = 0.0;
            double x = a[nn * ld + nn];
            if (l == nn) {
                wr[nn] = x + t;
                wi[nn] = 0.0;
                nn -= 1;
            } else {
                double y = a[(nn - 1) * ld + nn - 1];
                double w = a[nn * ld + nn - 1] * a[(nn - 1) * ld + nn];
                if (l == nn - 1) {
                    pz_hqr_pair(x, y, w, t, wr + nn - 1, wi + nn - 1);
                    nn -= 2;
                } else {
                    if (its == PZ_HQR_ITS) return CSIM_ST_PZ_NONCONV;
                    if (its == 10 || its == 20) {
                        t = t + x;
                        for (int i = 0; i <= nn; ++i) a[i * ld + i] = a[i * ld + i] - x;
                        const double s = fabs(a[nn * ld + nn - 1]) + fabs(a[(nn - 1) * ld + nn - 2]);
                        y = x = 0.75 * s;
                        w = -0.4375 * s * s;
                    }
                    ++its;
                    double p, q, r;
                    const int m = pz_hqr_start(a, ld, l, nn, x, y, w, &p, &q, &r);
                    for (int i = m + 2; i <= nn; ++i) {
                        a[i * ld + i - 2] = 0.0;
                        if (i != m + 2) a[i * ld + i - 3] = 0.0;
                    }
                    for (int k = m; k <= nn - 1; ++k) {
                        if (k != m) {
                            p = a[k * ld + k - 1];
                            q = a[(k + 1) * ld + k - 1];
                            r = k != nn - 1 ? a[(k + 2) * ld + k - 1] : 0.0;
                        }
                        PzReflector h;
                        double sub;
                        bool setSub;
                        const double akk1 = k > 0 ? a[k * ld + k - 1] : 0.0;
                        if (!pz_hqr_reflector(k == m, l == m, akk1, p, q, r, &h, &sub, &setSub)) continue;
                        if (setSub) a[k * ld + k - 1] = sub;
                        h.three = k != nn - 1;
                        for (int j = k; j <= nn; ++j) pz_hqr_row_at(h, a + k * ld + j, ld);
                        const int mmin = nn < k + 3 ? nn : k + 3;
                        for (int i = l; i <= mmin; ++i) pz_hqr_col_at(h, a + i * ld + k);
                    }
                }
            }
        } while (l < nn - 1);
    }
    return 0u;
}

// cut, poles, order and summary from the n eigenvalues of M; poles [n] complex (re, im interleaved)
CSIM_AC_HD inline void pz_finish(int n, const double* wr, const double* wi, double sigma0, double wmax, double* poles,
                                 int* n_poles, int* n_rhp, double* max_re)
{
    const double nan = NAN;
    int np = 0;
    for (int e = 0; e < n; ++e) {
        const double m2 = pz_mag2(wr[e], wi[e]);
        if (!pz_finite_pole(m2, wmax)) continue;
        int rank = 0;
        for (int o = 0; o < n; ++o) {
            const double m2o = pz_mag2(wr[o], wi[o]);
            if (o != e && pz_finite_pole(m2o, wmax) && pz_before(m2o, wr[o], wi[o], o, m2, wr[e], wi[e], e)) ++rank;
        }
        const cpx s = pz_pole(wr[e], wi[e], m2, sigma0);
        poles[2 * rank] = s.re;
        poles[2 * rank + 1] = s.im;
        ++np;
    }
    for (int k = np; k < n; ++k) { poles[2 * k] = nan; poles[2 * k + 1] = nan; }
    int rhp = 0;
    double mx = nan;
    for (int k = 0; k < np; ++k) {
        const double re = poles[2 * k];
        if (re > 0.0) ++rhp;
        if (k == 0 || re > mx) mx = re;
    }
    *n_poles = np;
    *n_rhp = rhp;
    *max_re = mx;
}

// a flagged instance: no pole, every slot NaN
CSIM_AC_HD inline void pz_fail(int n, double* poles, int* n_poles, int* n_rhp, double* max_re)
{
    const double nan = NAN;
    for (int k = 0; k < n; ++k) { poles[2 * k] = nan; poles[2 * k + 1] = nan; }
    *n_poles = 0;
    *n_rhp = 0;
    *max_re = nan;
}

// Sequential statement of one instance.  G, C row-major [n][n]; a0, m work planes of n * ld doubles (ld >= n); wr, wi
// n doubles each; poles gets n complex values.  Returns CSIM_ST_* flags.
CSIM_AC_HD inline unsigned pz_poles(int n, const double* G, const double* C, double sigma0, double wmax, double eps, int ld,
                                    double* a0, double* m, double* wr, double* wi, double* poles, int* n_poles, int* n_rhp,
                                    double* max_re)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            a0[i * ld + j] = pz_shift(G[i * n + j], C[i * n + j], sigma0);
            m[i * ld + j] = C[i * n + j];
        }
    if (!pz_lu_solve(n, a0, ld, m, ld, eps)) {
        pz_fail(n, poles, n_poles, n_rhp, max_re);
        return CSIM_ST_PZ_SINGULAR;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) m[i * ld + j] = -m[i * ld + j];
    pz_balance(n, m, ld, nullptr);
    pz_elmhes(n, m, ld);
    if (const unsigned fl = pz_hqr(n, m, ld, wr, wi)) {
        pz_fail(n, poles, n_poles, n_rhp, max_re);
        return fl;
    }
    pz_finish(n, wr, wi, sigma0, wmax, poles, n_poles, n_rhp, max_re);
    return 0u;
}

} // namespace csim
