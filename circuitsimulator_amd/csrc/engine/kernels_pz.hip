// kernels_pz.hip -- pole analysis: the finite poles of B instances as the eigenvalues of M = -(G + sigma0 C)^-1 C by
// balancing, elimination to Hessenberg form and Francis double-shift QR (include/csim.h "Pole analysis", arithmetic in
// pz.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major; its J is not read).  One kernel,
// pz_wave_kernel: one wavefront per instance, N <= 63, everything in LDS:
//
//   A   N x LD    G + sigma0 C, factored in place by lu_solve_multi_wave (device_common.hpp)
//   H   N x LD    C, then A^-1 C, then M, its balanced form, the Hessenberg form and what hqr leaves
//   wr, wi, m2, pr, pi   64 doubles each: eigenvalues, their squared magnitudes, the ordered poles
//
// LD = N | 1 is odd: the row phases (lanes over the columns of a row) read consecutive words, the column phases
// (lanes over the rows of a column) read words LD apart, and an odd stride of 8-byte words spreads 64 lanes over the
// banks as evenly as consecutive words do.  Neither phase pays.  At N = 63 this is 66 064 bytes: two workgroups per
// compute unit of 160 KiB.
//
// What is uniform (pivot choices, shifts, deflation, the reflector's scalars) every lane computes from LDS with the
// functions of pz.hpp; lane 0 stores what they write.  What is per element runs lane-parallel with the same
// expression per element as pz.hpp's loops, the phases separated by wave_sync() exactly where pz.hpp finishes one loop
// before it starts the next.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "kernels.hpp"
#include "pz.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double pz_ordered_sum(double v, int N)
{
    double s = 0.0;
    for (int j = 0; j < N; ++j) s = s + read_lane(v, j);
    return s;
}

// pz_balance()
__device__ __forceinline__ void pzw_balance(int N, int LD, double* H, int lane)
{
    for (int sweep = 0; sweep < PZ_BALANCE_SWEEPS; ++sweep) {
        bool changed = false;
        for (int i = 0; i < N; ++i) {
            const bool on = lane < N && lane != i;
            const double c = pz_ordered_sum(on ? fabs(H[lane * LD + i]) : 0.0, N);
            const double r = pz_ordered_sum(on ? fabs(H[i * LD + lane]) : 0.0, N);
            const double f = pz_balance_factor(c, r);
            if (f == 1.0) continue;
            const double g = 1.0 / f;
            changed = true;
            if (lane < N) {
                H[i * LD + lane] = H[i * LD + lane] * g;
                H[lane * LD + i] = H[lane * LD + i] * f;
            }
            wave_sync();
        }
        if (!changed) break;
    }
}

// pz_elmhes()
__device__ __forceinline__ void pzw_elmhes(int N, int LD, double* H, int lane)
{
    for (int m = 1; m < N - 1; ++m) {
        const bool cand = lane >= m && lane < N;
        const double v = cand ? fabs(H[lane * LD + m - 1]) : -1.0;
        const double best = wave_max(v);
        if (!(best > 0.0)) continue;
        const int piv = __ffsll((long long)__ballot(cand && v == best)) - 1;
        if (piv != m) {
            if (lane >= m - 1 && lane < N) {
                const double t = H[piv * LD + lane];
                H[piv * LD + lane] = H[m * LD + lane];
                H[m * LD + lane] = t;
            }
            wave_sync();
            if (lane < N) {
                const double t = H[lane * LD + piv];
                H[lane * LD + piv] = H[lane * LD + m];
                H[lane * LD + m] = t;
            }
            wave_sync();
        }
        const double x = H[m * LD + m - 1];
        if (lane > m && lane < N) {
            const double y = H[lane * LD + m - 1];
            if (y != 0.0) H[lane * LD + m - 1] = y / x;
        }
        wave_sync();
        const int cols = N - m, total = (N - m - 1) * cols;
        for (int e = lane; e < total; e += 64) {                // row phase
            const int di = e / cols;
            const int i = m + 1 + di, j = m + (e - di * cols);
            const double y = H[i * LD + m - 1];
            if (y != 0.0) H[i * LD + j] = pz_elm_row(H[i * LD + j], y, H[m * LD + j]);
        }
        wave_sync();
        if (lane < N) {                                         // column phase
            double acc = H[lane * LD + m];
            for (int i = m + 1; i < N; ++i) {
                const double y = H[i * LD + m - 1];
                if (y != 0.0) acc = pz_elm_col(acc, y, H[lane * LD + i]);
            }
            H[lane * LD + m] = acc;
        }
        wave_sync();
    }
    if (lane >= 2 && lane < N)
        for (int j = 0; j < lane - 1; ++j) H[lane * LD + j] = 0.0;
    wave_sync();
}

// pz_hqr()
__device__ __forceinline__ unsigned pzw_hqr(int N, int LD, double* H, double* wr, double* wi, int lane)
{
    const double anorm = pz_ordered_sum(lane < N ? pz_hess_row_norm(H, LD, N, lane) : 0.0, N);
    int nn = N - 1;
    double t = 0.0;
    while (nn >= 0) {
        int its = 0, l;
        do {
            l = pz_hqr_find_l(H, LD, nn, anorm);
            wave_sync();
            if (l >= 1 && lane == 0) H[l * LD + l - 1] = 0.0;
            wave_sync();
            double x = H[nn * LD + nn];
            if (l == nn) {
                if (lane == 0) { wr[nn] = x + t; wi[nn] = 0.0; }
                nn -= 1;
            } else {
                double y = H[(nn - 1) * LD + nn - 1];
                double w = H[nn * LD + nn - 1] * H[(nn - 1) * LD + nn];
                if (l == nn - 1) {
                    double pr[2], pi[2];
                    pz_hqr_pair(x, y, w, t, pr, pi);
                    if (lane == 0) { wr[nn - 1] = pr[0]; wr[nn] = pr[1]; wi[nn - 1] = pi[0]; wi[nn] = pi[1]; }
                    nn -= 2;
                } else {
                    if (its == PZ_HQR_ITS) return CSIM_ST_PZ_NONCONV;
                    if (its == 10 || its == 20) {
                        t = t + x;
                        wave_sync();
                        if (lane <= nn) H[lane * LD + lane] = H[lane * LD + lane] - x;
                        wave_sync();
                        const double s = fabs(H[nn * LD + nn - 1]) + fabs(H[(nn - 1) * LD + nn - 2]);
                        y = x = 0.75 * s;
                        w = -0.4375 * s * s;
                    }
                    ++its;
                    double p, q, r;
                    const int m = pz_hqr_start(H, LD, l, nn, x, y, w, &p, &q, &r);
                    wave_sync();
                    if (lane >= m + 2 && lane <= nn) {
                        H[lane * LD + lane - 2] = 0.0;
                        if (lane != m + 2) H[lane * LD + lane - 3] = 0.0;
                    }
                    wave_sync();
                    for (int k = m; k <= nn - 1; ++k) {
                        if (k != m) {
                            p = H[k * LD + k - 1];
                            q = H[(k + 1) * LD + k - 1];
                            r = k != nn - 1 ? H[(k + 2) * LD + k - 1] : 0.0;
                        }
                        PzReflector h;
                        double sub;
                        bool setSub;
                        const double akk1 = k > 0 ? H[k * LD + k - 1] : 0.0;
                        if (!pz_hqr_reflector(k == m, l == m, akk1, p, q, r, &h, &sub, &setSub)) continue;
                        h.three = k != nn - 1;
                        wave_sync();
                        if (setSub && lane == 0) H[k * LD + k - 1] = sub;
                        const int j = k + lane;                 // row phase: columns k .. nn
                        if (j <= nn) pz_hqr_row_at(h, H + k * LD + j, LD);
                        wave_sync();
                        const int mmin = nn < k + 3 ? nn : k + 3;
                        const int i = l + lane;                 // column phase: rows l .. mmin
                        if (i <= mmin) pz_hqr_col_at(h, H + i * LD + k);
                        wave_sync();
                    }
                }
            }
        } while (l < nn - 1);
    }
    wave_sync();
    return 0u;
}

__global__ void __launch_bounds__(64) pz_wave_kernel(PzArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int N = a.N;
    const int c0 = blockIdx.x, b = a.b0 + c0;
    const int LD = N | 1;
    double* const A = lds;
    double* const H = A + N * LD;
    double* const wr = H + N * LD;
    double* const wi = wr + 64;
    double* const m2 = wi + 64;
    double* const pr = m2 + 64;
    double* const pi = pr + 64;
    const double* Gt = a.sys + (size_t)c0 * (2 * N * N + 2 * N);
    const double* Ct = Gt + N * N;
    const double nan = NAN;

    for (int idx = lane; idx < N * N; idx += 64) {              // word q * N + m of a column-major plane is entry (m, q)
        const int q = idx / N, m = idx - q * N;
        const double cv = Ct[idx];
        A[m * LD + q] = pz_shift(Gt[idx], cv, a.sigma0);
        H[m * LD + q] = cv;
    }
    wave_sync();

    unsigned flags = 0u;
    if (!lu_solve_multi_wave(A, N, LD, H, N, LD, a.eps, lane)) flags = CSIM_ST_PZ_SINGULAR;
    if (!flags) {
        for (int idx = lane; idx < N * N; idx += 64) {
            const int i = idx / N, j = idx - i * N;
            H[i * LD + j] = -H[i * LD + j];
        }
        wave_sync();
        pzw_balance(N, LD, H, lane);
        pzw_elmhes(N, LD, H, lane);
        flags = pzw_hqr(N, LD, H, wr, wi, lane);
    }
    wave_sync();

    // pz_finish(): lane e owns eigenvalue e
    int np = 0, rhp = 0;
    double mx = nan;
    if (lane < N) { pr[lane] = nan; pi[lane] = nan; }
    if (!flags) {
        const double mr = lane < N ? wr[lane] : 0.0, mi = lane < N ? wi[lane] : 0.0;
        const double mm = pz_mag2(mr, mi);
        const bool keep = lane < N && pz_finite_pole(mm, a.wmax);
        m2[lane] = keep ? mm : nan;                             // NaN marks what the cut dropped
        wave_sync();
        if (keep) {
            int rank = 0;
            for (int o = 0; o < N; ++o) {
                const double mo = m2[o];
                if (o != lane && mo == mo && pz_before(mo, wr[o], wi[o], o, mm, mr, mi, lane)) ++rank;
            }
            const cpx s = pz_pole(mr, mi, mm, a.sigma0);
            pr[rank] = s.re;
            pi[rank] = s.im;
        }
        np = __popcll(__ballot(keep));
        wave_sync();
        for (int k = 0; k < np; ++k) {
            const double re = pr[k];
            if (re > 0.0) ++rhp;
            if (k == 0 || re > mx) mx = re;
        }
    }
    wave_sync();
    if (lane < N) {
        const size_t at = ((size_t)lane * (size_t)a.B + (size_t)b) * 2;
        a.poles[at] = pr[lane];
        a.poles[at + 1] = pi[lane];
    }
    if (lane == 0) {
        a.nPoles[b] = np;
        a.nRhp[b] = rhp;
        a.maxRe[b] = mx;
        if (flags) a.status[b] |= flags;
    }
}

} // namespace

size_t pzLdsBytes(int N) { return sizeof(double) * (2 * (size_t)N * (size_t)(N | 1) + 5 * 64); }

hipError_t launchPz(const PzArgs& a, hipStream_t stream)
{
    if (a.Bc <= 0) return hipSuccess;
    if (a.N < 1 || a.N > PZ_MAX_N) return hipErrorInvalidValue;
    if (!a.sys || !a.poles || !a.nPoles || !a.nRhp || !a.maxRe || !a.status) return hipErrorInvalidValue;
    const size_t lds = pzLdsBytes(a.N);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)pz_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(pz_wave_kernel, dim3(a.Bc), dim3(64), lds, stream, a);
    return hipGetLastError();
}

} // namespace csim
