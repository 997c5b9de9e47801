// kernels_disto.hip -- small-signal distortion analysis: HD2 and HD3 of B instances x F frequencies by a Volterra
// series at the operating point (include/csim.h "Distortion analysis", arithmetic in ac_disto.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major, J).  Three kernels:
//
//   disto_coef_kernel        one thread per (MOSFET, instance), ONCE per instance: the seven derivatives of the drain
//                            current at x_op (disto_coef), region decided as mos_eval decides it.
//   ac_disto_wave_kernel     one wavefront per instance, N <= 63: A(k w) in LDS, acw_load / acw_solve of ac_sweep.hpp,
//                            three times per frequency; x1 and x2 kept in LDS beside the solution.
//   ac_disto_packed_kernel   N <= 32: 32 lanes per instance, lane r owns row r, acp_column / acp_back; x1, x2, x3 in a
//                            small LDS tile for the indexed gathers of the device voltages.
//
// Right-hand side of order 2 and 3.  The devices are taken a wave (or half-wave) at a time: lane t computes the current
// of device m0 + t from the lower orders in LDS and leaves it there with its drain and source equations; then the lane
// that owns equation i walks those entries in ascending order and subtracts / adds into its two registers.  Every entry
// of the right-hand side so sees the devices in ascending order, whatever the kernel shape: the outputs of the two
// kernels are bit-identical.  The matrix is loaded after the right-hand side is known, so the packed kernel holds no
// more live registers through a factorisation than the AC kernel does.
#include <hip/hip_runtime.h>

#include "ac_disto.hpp"
#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

__global__ void __launch_bounds__(256) disto_coef_kernel(GenPlan pl, const int32_t* __restrict__ devElem, int M,
                                                         const double* __restrict__ params, int B, int b0, int Bc,
                                                         const double* __restrict__ xop, double* __restrict__ coef,
                                                         size_t coefStride, size_t coefOff)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)M * (size_t)Bc) return;
    const int m = (int)(t / (size_t)Bc), c = (int)(t - (size_t)m * (size_t)Bc);
    const size_t b = (size_t)b0 + (size_t)c;
    const int e = devElem[m];
    const int kind = pl.kind[e], slot = pl.slot[e];
    auto P = [&](int p) { return params[(size_t)(slot + p) * (size_t)B + b]; };
    auto X = [&](int eq) { return eq >= 0 ? xop[(size_t)eq * (size_t)B + b] : 0.0; };
    const int32_t* q = pl.eq + 4 * e;
    const DistoCoef r = disto_coef(kind == CSIM_PMOS, P(0), P(1), P(2), X(q[0]), X(q[1]), X(q[2]));
#pragma unroll
    for (int k = 0; k < DISTO_NCOEF; ++k) coef[((size_t)m * DISTO_NCOEF + k) * coefStride + coefOff + (size_t)c] = r.c[k];
}

// the current of device m of chunk instance c at order k (2 or 3) from x1 (and x2) in LDS
__device__ __forceinline__ cpx disto_current(const DistoArgs& a, int k, int m, int c, int d, int g, int s, const double* X1r,
                                             const double* X1i, const double* X2r, const double* X2i)
{
    double cf[DISTO_NCOEF];
#pragma unroll
    for (int q = 0; q < DISTO_NCOEF; ++q) cf[q] = a.coef[((size_t)m * DISTO_NCOEF + q) * a.coefStride + a.coefOff + (size_t)c];
    const cpx Ug = disto_u(X1r, X1i, g, s), Ud = disto_u(X1r, X1i, d, s);
    if (k == 2) return disto_i2(cf, Ug, Ud);
    return disto_i3(cf, Ug, Ud, disto_u(X2r, X2i, g, s), disto_u(X2r, X2i, d, s));
}

// where order k (1 .. 3) of unknown p, frequency f, instance b goes: complex pairs, 64-bit
__device__ __forceinline__ size_t disto_h_at(const DistoArgs& a, int f, int k, int p, int b)
{
    return ((((size_t)f * 3 + (size_t)(k - 1)) * (size_t)a.N + (size_t)p) * (size_t)a.B + (size_t)b) * 2;
}

// HD2 and HD3 of (frequency f, instance b) from the three orders in LDS (x1, x2 at H, STRIDE doubles per part; x3 at
// X3r, X3i): one lane
template <int STRIDE>
__device__ __forceinline__ void disto_store_hd(const DistoArgs& a, int f, int b, const double* H, const double* X3r,
                                               const double* X3i)
{
    const double v1 = disto_abs(disto_u(H, H + STRIDE, a.outP, a.outM));
    const double v2 = disto_abs(disto_u(H + 2 * STRIDE, H + 3 * STRIDE, a.outP, a.outM));
    const double v3 = disto_abs(disto_u(X3r, X3i, a.outP, a.outM));
    a.hd[((size_t)f * 2 + 0) * (size_t)a.B + (size_t)b] = disto_hd(v2, v1);
    a.hd[((size_t)f * 2 + 1) * (size_t)a.B + (size_t)b] = disto_hd(v3, v1);
}

// ---- wave per system (N <= 63)
// dynamic LDS: the planes, Lr / Li and the solution (acw_carve), then x1 and x2 (re, im: 64 doubles each); x3 stays in
// the solution.  Between two solves Lr / Li and the real part of the solution (already copied) are free: they take the
// currents of a round of 64 devices (re, im) and their drain and source equations (2 x 64 int32).  So the kernel asks
// for 2 KiB more than the AC kernel and, at N = 31, still fits eight workgroups into the 160 KiB of a compute unit.
constexpr int DISTO_WAVE_EXTRA = 2 * 128;                   // doubles

__global__ void __launch_bounds__(64) ac_disto_wave_kernel(DistoArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int N = a.N, M = a.M;
    const int c = blockIdx.x, b = a.b0 + c;
    const int LD = acw_ld(N, 1);
    const AcwLds m = acw_carve(lds, N, 1, LD);
    double *const Ar = m.Ar, *const Ai = m.Ai, *const Xr = m.Xr, *const Xi = m.Xi;
    double* const H = m.Xi + 64;                            // order k = 1, 2 at H + (k - 1) * 128: re, then im
    double *const Cr = m.Lr, *const Ci = m.Li;
    int32_t* const Ed = reinterpret_cast<int32_t*>(Xr);
    int32_t* const Es = Ed + 64;
    const double* Gt = ac_system_at(a.sys, c, N);
    const double* Ct = Gt + N * N;
    const double* Jr = Ct + N * N;
    const double* Ji = Jr + N;
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        bool failed = false;
#pragma unroll 1
        for (int k = 1; k <= 3; ++k) {
            double rr = 0.0, ri = 0.0;                      // entry `lane` of the right-hand side
            if (k == 1) {
                if (lane < N) { rr = Jr[lane]; ri = Ji[lane]; }
            } else {
                for (int m0 = 0; m0 < M; m0 += 64) {
                    const int mm = m0 + lane;
                    if (mm < M) {
                        const int d = a.devD[mm], g = a.devG[mm], s = a.devS[mm];
                        const cpx I = disto_current(a, k, mm, c, d, g, s, H, H + 64, H + 128, H + 192);
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
            acw_load<false>(N, LD, Gt, Ct, (double)k * w, Ar, Ai, lane);
            if (lane < N) { Ar[lane * LD + N] = rr; Ai[lane * LD + N] = ri; }
            wave_sync();

            if (acw_solve(N, 1, LD, Ar, Ai, m.Lr, m.Li, Xr, Xi, eps2, lane)) {
                flags |= CSIM_ST_LU_TINY_PIVOT;
                failed = true;
            }
            if (lane < N) {
                const double yr = failed ? 0.0 : Xr[lane], yi = failed ? 0.0 : Xi[lane];    // a failed lower order too
                double* const Yr = k < 3 ? H + (k - 1) * 128 : Xr;
                double* const Yi = k < 3 ? Yr + 64 : Xi;
                Yr[lane] = yr;
                Yi[lane] = yi;
                if (a.h) {
                    const size_t at = disto_h_at(a, f, k, lane, b);
                    a.h[at] = yr;
                    a.h[at + 1] = yi;
                }
            }
            wave_sync();
        }
        if (lane == 0) disto_store_hd<64>(a, f, b, H, Xr, Xi);
        wave_sync();
    }
    if (lane == 0 && flags) a.status[b] |= flags;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32)
template <int NP>
__global__ void __launch_bounds__(64) ac_disto_packed_kernel(DistoArgs a)
{
    __shared__ double xs[2][2][ACP_LANES];                  // [instance][re, im][position]: the solution
    __shared__ double hs[2][3][2][ACP_LANES];               // [instance][order][re, im][equation]
    __shared__ double cur[2][2][ACP_LANES];                 // [instance][re, im][device of the round]
    __shared__ int32_t ends[2][2][ACP_LANES];               // [instance][drain, source][device of the round]
    const int N = a.N, M = a.M;
    const AcpInstance t = acp_instance(a.b0, a.Bc);
    const int h = t.h, r = t.r, cc = t.cc, b = t.b;
    const bool on = t.on;
    const double* Gt = ac_system_at(a.sys, cc, N);
    const double* Ct = Gt + N * N;
    const double* Jr = Ct + N * N;
    const double* Ji = Jr + N;
    double* Xr = xs[h][0];
    double* Xi = xs[h][1];
    const double* H = &hs[h][0][0][0];
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        bool failed = false;
#pragma unroll 1
        for (int k = 1; k <= 3; ++k) {
            double rr = 0.0, ri = 0.0;                      // entry r of the right-hand side
            if (k == 1) {
                if (r < N) { rr = Jr[r]; ri = Ji[r]; }
            } else {
                for (int m0 = 0; m0 < M; m0 += ACP_LANES) {
                    const int mm = m0 + r;
                    if (mm < M) {
                        const int d = a.devD[mm], g = a.devG[mm], s = a.devS[mm];
                        const cpx I = disto_current(a, k, mm, cc, d, g, s, hs[h][0][0], hs[h][0][1], hs[h][1][0], hs[h][1][1]);
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
            const double wk = (double)k * w;
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
            if (r < N) {
                const double yr = failed ? 0.0 : Xr[r], yi = failed ? 0.0 : Xi[r];          // a failed lower order too
                hs[h][k - 1][0][r] = yr;
                hs[h][k - 1][1][r] = yi;
                if (a.h && on) {
                    const size_t at = disto_h_at(a, f, k, r, b);
                    a.h[at] = yr;
                    a.h[at + 1] = yi;
                }
            }
            __syncthreads();
        }
        if (on && r == 0) disto_store_hd<ACP_LANES>(a, f, b, H, hs[h][2][0], hs[h][2][1]);
        __syncthreads();
    }
    if (on && r == 0 && flags) a.status[b] |= flags;
}

} // namespace

hipError_t launchDistoCoef(const GenPlan& pl, const int32_t* dDevElem, int M, const double* dParams, int B, int b0, int Bc,
                           const double* dXop, double* dCoef, size_t coefStride, size_t coefOff, hipStream_t stream)
{
    if (Bc <= 0 || M <= 0) return hipSuccess;
    const size_t total = (size_t)M * (size_t)Bc;
    hipLaunchKernelGGL(disto_coef_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, pl, dDevElem, M, dParams,
                       B, b0, Bc, dXop, dCoef, coefStride, coefOff);
    return hipGetLastError();
}

hipError_t launchDistoSweep(int which, const DistoArgs& a, hipStream_t stream)
{
    if (a.Bc <= 0 || a.F <= 0) return hipSuccess;
    const int N = a.N;
    if (which != AC_KERNEL_WAVE && which != AC_KERNEL_PACKED) return hipErrorInvalidValue;
    if (!ac_sweep_covers(which, N)) return hipErrorInvalidValue;
    if (a.outP < 0 || a.outP >= N || a.outM < -1 || a.outM >= N || a.M < 0 || !a.hd) return hipErrorInvalidValue;
    if (which == AC_KERNEL_PACKED) {
        acp_dispatch(N, [&](auto np) {
            hipLaunchKernelGGL(ac_disto_packed_kernel<decltype(np)::value>, dim3((a.Bc + 1) / 2), dim3(64), 0, stream, a);
        });
    } else {
        const size_t lds = acw_lds_bytes(N, 1) + sizeof(double) * DISTO_WAVE_EXTRA;
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute((const void*)ac_disto_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(ac_disto_wave_kernel, dim3(a.Bc), dim3(64), lds, stream, a);
    }
    return hipGetLastError();
}

} // namespace csim
