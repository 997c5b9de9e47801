// kernels_imd.hip -- two-tone intermodulation analysis: IM2+, IM2- and IM3 of B instances x F tone pairs by a Volterra
// series at the operating point (include/csim.h "Intermodulation analysis", arithmetic in ac_imd.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major, J); the coefficients are those of
// disto_coef_kernel (kernels_disto.hip).  Six dependent solves per (instance, pair), k = 0 .. 5 at w1, w2, w1 + w2,
// w1 - w2, 2 w1 and 2 w1 - w2, in the two shapes of kernels_disto.hip:
//
//   ac_imd_wave_kernel     one wavefront per instance, N <= 63: A(w_k) in LDS, acw_load / acw_solve of ac_sweep.hpp;
//                          x0, x1, x3 and x4 kept in LDS beside the solution, x2 only written out, x5 stays in the
//                          solution.
//   ac_imd_packed_kernel   N <= 32: 32 lanes per instance, lane r owns row r, acp_column / acp_back; the solution and
//                          x0, x1, x3, x4 in a small LDS tile for the indexed gathers of the device voltages.
//
// Right-hand side of the solves 2 .. 5: the device round of kernels_disto.hip, restated here with imd_current.  The
// devices are taken a wave (or half-wave) at a time: lane t computes the current of device m0 + t from the kept
// solutions in LDS and leaves it there with its drain and source equations; then the lane that owns equation i walks
// those entries in ascending order and subtracts / adds into its two registers.  Every entry of the right-hand side so
// sees the devices in ascending order, whatever the kernel shape: the outputs of the two kernels are bit-identical.
// The matrix is loaded after the right-hand side is known, so the packed kernel holds no more live registers through
// a factorisation than the AC kernel does.
#include <hip/hip_runtime.h>

#include "ac_imd.hpp"
#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

// where a kept solution lives: x0, x1, x3, x4 -> slot 0 .. 3
__device__ __forceinline__ int imd_slot(int k) { return k < 2 ? k : k - 1; }

// the current of device m of chunk instance c in solve k (2 .. 5) from the kept solutions: slot q at K + q * 2 * stride,
// re then im
__device__ __forceinline__ cpx imd_device_current(const ImdArgs& a, int k, int m, int c, int d, int g, int s, const double* K,
                                                  int stride)
{
    double cf[DISTO_NCOEF];
#pragma unroll
    for (int q = 0; q < DISTO_NCOEF; ++q) cf[q] = a.coef[((size_t)m * DISTO_NCOEF + q) * a.coefStride + a.coefOff + (size_t)c];
    return imd_current(k, cf, d, g, s, K, K + stride, K + 2 * stride, K + 3 * stride, K + 4 * stride, K + 5 * stride,
                       K + 6 * stride, K + 7 * stride);
}

// where solve k (0 .. 5) of unknown p, pair f, instance b goes: complex pairs, 64-bit
__device__ __forceinline__ size_t imd_h_at(const ImdArgs& a, int f, int k, int p, int b)
{
    return ((((size_t)f * IMD_NSOLVE + (size_t)k) * (size_t)a.N + (size_t)p) * (size_t)a.B + (size_t)b) * 2;
}

// the three ratios of (pair f, instance b) from |v0|, |v2|, |v3|, |v5|: one lane
__device__ __forceinline__ void imd_store(const ImdArgs& a, int f, int b, double v0, double v2, double v3, double v5)
{
    a.im[((size_t)f * IMD_NRATIO + 0) * (size_t)a.B + (size_t)b] = disto_hd(v2, v0);
    a.im[((size_t)f * IMD_NRATIO + 1) * (size_t)a.B + (size_t)b] = disto_hd(v3, v0);
    a.im[((size_t)f * IMD_NRATIO + 2) * (size_t)a.B + (size_t)b] = disto_hd(v5, v0);
}

// ---- wave per system (N <= 63)
// dynamic LDS: the planes, Lr / Li and the solution (acw_carve), then x0, x1, x3 and x4 (re, im: N doubles each).
// Between two solves Lr / Li and the real part of the solution (already copied or consumed) are free: they take the
// currents of a round of 64 devices (re, im) and their drain and source equations (2 x 64 int32).  So the kernel asks
// for 64 N bytes more than the AC kernel, 4 KiB at most: 20400 bytes at N = 31, eight workgroups in the 160 KiB of a
// compute unit, as the AC and the single-tone kernel.  (With 64 doubles per part, as the solution has them, it was
// 22512 bytes and seven workgroups: three passes over a batch of 4096 instead of two.)
inline size_t imd_wave_extra(int N) { return (size_t)8 * (size_t)N; }      // doubles

__global__ void __launch_bounds__(64) ac_imd_wave_kernel(ImdArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int N = a.N, M = a.M;
    const int c = blockIdx.x, b = a.b0 + c;
    const int LD = acw_ld(N, 1);
    const AcwLds m = acw_carve(lds, N, 1, LD);
    double *const Ar = m.Ar, *const Ai = m.Ai, *const Xr = m.Xr, *const Xi = m.Xi;
    double* const H = m.Xi + 64;                            // kept solution of slot q at H + q * 2 * N: re, then im
    double *const Cr = m.Lr, *const Ci = m.Li;
    int32_t* const Ed = reinterpret_cast<int32_t*>(Xr);
    int32_t* const Es = Ed + 64;
    const double* Gt = ac_system_at(a.sys, c, N);
    const double* Ct = Gt + N * N;
    const double* J1r = Ct + N * N;
    const double* J2r = a.j2 ? a.j2 + (size_t)c * 2 * N : J1r;
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w1 = a.omega[f], w2 = a.omega2[f];
        bool failed = false;
        double v2 = 0.0;
#pragma unroll 1
        for (int k = 0; k < IMD_NSOLVE; ++k) {
            double rr = 0.0, ri = 0.0;                      // entry `lane` of the right-hand side
            if (k < 2) {
                const double* J = k == 0 ? J1r : J2r;
                if (lane < N) { rr = J[lane]; ri = J[N + lane]; }
            } else {
                for (int m0 = 0; m0 < M; m0 += 64) {
                    const int mm = m0 + lane;
                    if (mm < M) {
                        const int d = a.devD[mm], g = a.devG[mm], s = a.devS[mm];
                        const cpx I = imd_device_current(a, k, mm, c, d, g, s, H, N);
                        Cr[lane] = I.re;
                        Ci[lane] = I.im;
                        Ed[lane] = d;
                        Es[lane] = s;
                    }
                    wave_sync();
                    const int cnt = min(64, M - m0);
                    for (int t = 0; t < cnt; ++t) {
                        if (Ed[t] == lane) { rr = rr - Cr[t]; ri = ri - Ci[t]; }
                        if (Es[t] == lane) { rr = rr + Cr[t]; ri = ri + Ci[t]; }
                    }
                    wave_sync();
                }
            }
            acw_load<false>(N, LD, Gt, Ct, imd_freq(k, w1, w2), Ar, Ai, lane);
            if (lane < N) { Ar[lane * LD + N] = rr; Ai[lane * LD + N] = ri; }
            wave_sync();

            if (acw_solve(N, 1, LD, Ar, Ai, m.Lr, m.Li, Xr, Xi, eps2, lane)) {
                flags |= CSIM_ST_LU_TINY_PIVOT;
                failed = true;
            }
            const bool kept = k != 2 && k != 5;
            if (lane < N) {
                const double yr = failed ? 0.0 : Xr[lane], yi = failed ? 0.0 : Xi[lane];    // an earlier failed solve too
                double* const Yr = kept ? H + imd_slot(k) * 2 * N : Xr;
                double* const Yi = kept ? Yr + N : Xi;
                Yr[lane] = yr;
                Yi[lane] = yi;
                if (a.h) {
                    const size_t at = imd_h_at(a, f, k, lane, b);
                    a.h[at] = yr;
                    a.h[at + 1] = yi;
                }
            }
            wave_sync();
            if (k == 2) {                                   // x2 leaves the solution with the next round
                v2 = disto_abs(disto_u(Xr, Xi, a.outP, a.outM));
                wave_sync();
            }
        }
        if (lane == 0)
            imd_store(a, f, b, disto_abs(disto_u(H, H + N, a.outP, a.outM)), v2,
                      disto_abs(disto_u(H + 4 * N, H + 5 * N, a.outP, a.outM)), disto_abs(disto_u(Xr, Xi, a.outP, a.outM)));
        wave_sync();
    }
    if (lane == 0 && flags) a.status[b] |= flags;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32)
template <int NP>
__global__ void __launch_bounds__(64) ac_imd_packed_kernel(ImdArgs a)
{
    __shared__ double xs[2][2][ACP_LANES];                  // [instance][re, im][position]: the solution
    __shared__ double ks[2][4][2][ACP_LANES];               // [instance][slot: x0, x1, x3, x4][re, im][equation]
    __shared__ double cur[2][2][ACP_LANES];                 // [instance][re, im][device of the round]
    __shared__ int32_t ends[2][2][ACP_LANES];               // [instance][drain, source][device of the round]
    const int N = a.N, M = a.M;
    const AcpInstance t = acp_instance(a.b0, a.Bc);
    const int h = t.h, r = t.r, cc = t.cc, b = t.b;
    const bool on = t.on;
    const double* Gt = ac_system_at(a.sys, cc, N);
    const double* Ct = Gt + N * N;
    const double* J1r = Ct + N * N;
    const double* J2r = a.j2 ? a.j2 + (size_t)cc * 2 * N : J1r;
    double* Xr = xs[h][0];
    double* Xi = xs[h][1];
    const double* K = &ks[h][0][0][0];
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w1 = a.omega[f], w2 = a.omega2[f];
        bool failed = false;
        double v2 = 0.0, v5 = 0.0;
#pragma unroll 1
        for (int k = 0; k < IMD_NSOLVE; ++k) {
            double rr = 0.0, ri = 0.0;                      // entry r of the right-hand side
            if (k < 2) {
                const double* J = k == 0 ? J1r : J2r;
                if (r < N) { rr = J[r]; ri = J[N + r]; }
            } else {
                for (int m0 = 0; m0 < M; m0 += ACP_LANES) {
                    const int mm = m0 + r;
                    if (mm < M) {
                        const int d = a.devD[mm], g = a.devG[mm], s = a.devS[mm];
                        const cpx I = imd_device_current(a, k, mm, cc, d, g, s, K, ACP_LANES);
                        cur[h][0][r] = I.re;
                        cur[h][1][r] = I.im;
                        ends[h][0][r] = d;
                        ends[h][1][r] = s;
                    }
                    __syncthreads();
                    const int cnt = min(ACP_LANES, M - m0);
                    for (int q = 0; q < cnt; ++q) {
                        if (ends[h][0][q] == r) { rr = rr - cur[h][0][q]; ri = ri - cur[h][1][q]; }
                        if (ends[h][1][q] == r) { rr = rr + cur[h][0][q]; ri = ri + cur[h][1][q]; }
                    }
                    __syncthreads();
                }
            }
            const double wk = imd_freq(k, w1, w2);
            double ar[NP + 1], ai[NP + 1];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const bool in = r < N && j < N;
                ar[j] = in ? Gt[j * N + r] : 0.0;
                ai[j] = in ? wk * Ct[j * N + r] : 0.0;
            }
            ar[NP] = rr;
            ai[NP] = ri;
            int pos = r;
            bool bad = false;
            acp_column<NP, 1, 0>(ar, ai, N, pos, bad, eps2, h);
            acp_back<NP, 1, NP - 1>(ar, ai, N, pos, Xr, Xi);
            if (bad) {
                flags |= CSIM_ST_LU_TINY_PIVOT;
                failed = true;
            }
            const bool kept = k != 2 && k != 5;
            if (r < N) {
                const double yr = failed ? 0.0 : Xr[r], yi = failed ? 0.0 : Xi[r];          // an earlier failed solve too
                if (kept) {
                    ks[h][imd_slot(k)][0][r] = yr;
                    ks[h][imd_slot(k)][1][r] = yi;
                } else {
                    Xr[r] = yr;
                    Xi[r] = yi;
                }
                if (a.h && on) {
                    const size_t at = imd_h_at(a, f, k, r, b);
                    a.h[at] = yr;
                    a.h[at + 1] = yi;
                }
            }
            __syncthreads();
            if (!kept) {                                    // the solution is overwritten by the next solve
                const double v = disto_abs(disto_u(Xr, Xi, a.outP, a.outM));
                if (k == 2) v2 = v; else v5 = v;
                __syncthreads();
            }
        }
        if (on && r == 0)
            imd_store(a, f, b, disto_abs(disto_u(ks[h][0][0], ks[h][0][1], a.outP, a.outM)), v2,
                      disto_abs(disto_u(ks[h][2][0], ks[h][2][1], a.outP, a.outM)), v5);
        __syncthreads();
    }
    if (on && r == 0 && flags) a.status[b] |= flags;
}

} // namespace

hipError_t launchImdSweep(int which, const ImdArgs& a, const int32_t* hostD, const int32_t* hostG, const int32_t* hostS,
                          hipStream_t stream)
{
    if (a.Bc <= 0 || a.F <= 0) return hipSuccess;
    const int N = a.N;
    if (which != AC_KERNEL_WAVE && which != AC_KERNEL_PACKED) return hipErrorInvalidValue;
    if (!ac_sweep_covers(which, N)) return hipErrorInvalidValue;
    if (a.outP < 0 || a.outP >= N || a.outM < -1 || a.outM >= N || a.M < 0 || !a.im || !a.omega2) return hipErrorInvalidValue;
    if (a.M > 0 && (!hostD || !hostG || !hostS)) return hipErrorInvalidValue;
    for (int m = 0; m < a.M; ++m)
        if (hostD[m] < -1 || hostD[m] >= N || hostG[m] < -1 || hostG[m] >= N || hostS[m] < -1 || hostS[m] >= N)
            return hipErrorInvalidValue;
    if (which == AC_KERNEL_PACKED) {
        acp_dispatch(N, [&](auto np) {
            hipLaunchKernelGGL(ac_imd_packed_kernel<decltype(np)::value>, dim3((a.Bc + 1) / 2), dim3(64), 0, stream, a);
        });
    } else {
        const size_t lds = acw_lds_bytes(N, 1) + sizeof(double) * imd_wave_extra(N);
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute((const void*)ac_imd_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(ac_imd_wave_kernel, dim3(a.Bc), dim3(64), lds, stream, a);
    }
    return hipGetLastError();
}

} // namespace csim
