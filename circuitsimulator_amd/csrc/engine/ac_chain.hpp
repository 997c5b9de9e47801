// ac_chain.hpp -- the Volterra-type analyses (distortion, kernels_disto.hip; intermodulation, kernels_imd.hip) as ONE
// chain of dependent complex solves on G + jwC per (instance, point), in the two shapes of ac_sweep.hpp:
//
//   chain_wave     one wavefront per instance, N <= 63: A(w_k) in LDS, acw_load / acw_solve; the kept solutions in LDS
//                  beside the solution, N doubles per part.
//   chain_packed   N <= NP <= 32: 32 lanes per instance, lane r owns row r, acp_column / acp_back; the solution, the
//                  kept solutions and one device round in a small static LDS tile.
//
// A chain description says what differs between two analyses, all of it known at compile time:
//
//   NSOLVE, NTONE, NKEPT, NRATIO   solves 0 .. NTONE-1 take the excitations J1 / J2 as right-hand side, the later ones
//                                  the device round
//   slot(k)                        where solve k is kept for the currents of later solves (0 .. NKEPT-1), or -1
//   numerator(q)                   the solve whose |v| stands over |v_0| in ratio q
//   freq(k, w1, w2)                the frequency of solve k (w2 is 0.0 in a one-tone chain)
//   current(k, cf, d, g, s, K, stride)   drain current of a device with coefficients cf and terminals (d, g, s) in
//                                  solve k; kept slot q has re at K + q * 2 * stride and im one stride further
//
// The device round.  The devices are taken a wave (or half-wave) at a time: lane t computes the current of device
// m0 + t from the kept solutions in LDS and leaves it there with its drain and source equations; then the lane that
// owns equation i walks those entries in ascending order and subtracts / adds into its two registers.  Every entry of
// the right-hand side so sees the devices in ascending order, whatever the kernel shape: the outputs of the two shapes
// are bit-identical.  The matrix is loaded after the right-hand side is known, so the packed shape holds no more live
// registers through a factorisation than the AC kernel does.
//
// A failed solve zeroes itself and every later one.  The ratios read |v_0| and the numerators from their kept slots,
// the last solve's from the solution; a solve that is neither kept nor the last (at most one per chain) has its |v|
// taken right after it, before the next device round reuses the solution's words.
// Included by kernels_disto.hip and kernels_imd.hip only.
#pragma once

#include <hip/hip_runtime.h>

#include "ac_disto.hpp"
#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

// the solve whose |v| must be taken on the way: a numerator that is neither kept nor the last solve, or -1
template <class Chain>
constexpr int chain_passing()
{
    int found = -1, count = 0;
    for (int q = 0; q < Chain::NRATIO; ++q) {
        const int k = Chain::numerator(q);
        if (Chain::slot(k) < 0 && k != Chain::NSOLVE - 1) { found = k; ++count; }
    }
    return count <= 1 ? found : -2;
}

// the current of device m of chunk instance c in solve k from the kept solutions at K
template <class Chain>
__device__ __forceinline__ cpx chain_device_current(const ChainArgs& a, int k, int m, int c, int d, int g, int s,
                                                    const double* K, int stride)
{
    double cf[DISTO_NCOEF];
#pragma unroll
    for (int q = 0; q < DISTO_NCOEF; ++q) cf[q] = a.coef[((size_t)m * DISTO_NCOEF + q) * a.coefStride + a.coefOff + (size_t)c];
    return Chain::current(k, cf, d, g, s, K, stride);
}

// where solve k (zero-based) of unknown p, point f, instance b goes: [F][NSOLVE][N][B] complex pairs, 64-bit
template <class Chain>
__device__ __forceinline__ size_t chain_h_at(const ChainArgs& a, int f, int k, int p, int b)
{
    return ((((size_t)f * Chain::NSOLVE + (size_t)k) * (size_t)a.N + (size_t)p) * (size_t)a.B + (size_t)b) * 2;
}

// the ratios of (point f, instance b) from the kept solutions at K, the last solution at Xr / Xi and the |v| taken on
// the way: one lane
template <class Chain>
__device__ __forceinline__ void chain_store_ratios(const ChainArgs& a, int f, int b, const double* K, int stride,
                                                   const double* Xr, const double* Xi, double vPassing)
{
    const double v0 = disto_abs(disto_u(K + Chain::slot(0) * 2 * stride, K + (Chain::slot(0) * 2 + 1) * stride, a.outP, a.outM));
    double v[Chain::NRATIO];
#pragma unroll
    for (int q = 0; q < Chain::NRATIO; ++q) {
        constexpr int passing = chain_passing<Chain>();
        const int k = Chain::numerator(q), sl = Chain::slot(k);
        v[q] = sl >= 0 ? disto_abs(disto_u(K + sl * 2 * stride, K + (sl * 2 + 1) * stride, a.outP, a.outM))
                       : (k == passing ? vPassing : disto_abs(disto_u(Xr, Xi, a.outP, a.outM)));
    }
#pragma unroll
    for (int q = 0; q < Chain::NRATIO; ++q) a.ratio[((size_t)f * Chain::NRATIO + q) * (size_t)a.B + (size_t)b] = disto_hd(v[q], v0);
}

// ---- wave per system (N <= 63)
// dynamic LDS: the planes, Lr / Li and the solution (acw_carve), then the kept solutions (re, im: N doubles each); the
// last solution stays in the solution.  Between two solves Lr / Li and the real part of the solution (already copied
// or consumed) are free: they take the currents of a round of 64 devices (re, im) and their drain and source equations
// (2 x 64 int32).  So a chain asks for 16 NKEPT N bytes more than the AC kernel: at N = 31, 19 408 B with two kept
// solutions and 20 400 B with four, eight workgroups in the 160 KiB of a compute unit either way, as the AC kernel.
// (With 64 doubles per part, as the solution has them, four kept solutions were 22 512 bytes and seven workgroups:
// three passes over a batch of 4096 instead of two.)
template <class Chain>
inline size_t chain_wave_lds_bytes(int N) { return acw_lds_bytes(N, 1) + sizeof(double) * 2 * Chain::NKEPT * (size_t)N; }

template <class Chain>
__device__ __forceinline__ void chain_wave(const ChainArgs& a)
{
    constexpr int passing = chain_passing<Chain>();
    static_assert(passing >= -1 && Chain::slot(0) >= 0, "one |v| at most is taken on the way, and v_0 is kept");
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
    const double* J2r = Chain::NTONE == 2 && a.j2 ? a.j2 + (size_t)c * 2 * N : J1r;
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w1 = a.omega[f];
        double w2 = 0.0;
        if constexpr (Chain::NTONE == 2) w2 = a.omega2[f];
        bool failed = false;
        double vPassing = 0.0;
#pragma unroll 1
        for (int k = 0; k < Chain::NSOLVE; ++k) {
            double rr = 0.0, ri = 0.0;                      // entry `lane` of the right-hand side
            if (k < Chain::NTONE) {
                const double* J = k == 0 ? J1r : J2r;
                if (lane < N) { rr = J[lane]; ri = J[N + lane]; }
            } else {
                for (int m0 = 0; m0 < M; m0 += 64) {
                    const int mm = m0 + lane;
                    if (mm < M) {
                        const int d = a.devD[mm], g = a.devG[mm], s = a.devS[mm];
                        const cpx I = chain_device_current<Chain>(a, k, mm, c, d, g, s, H, N);
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
            acw_load<false>(N, LD, Gt, Ct, Chain::freq(k, w1, w2), Ar, Ai, lane);
            if (lane < N) { Ar[lane * LD + N] = rr; Ai[lane * LD + N] = ri; }
            wave_sync();

            if (acw_solve(N, 1, LD, Ar, Ai, m.Lr, m.Li, Xr, Xi, eps2, lane)) {
                flags |= CSIM_ST_LU_TINY_PIVOT;
                failed = true;
            }
            if (lane < N) {
                const double yr = failed ? 0.0 : Xr[lane], yi = failed ? 0.0 : Xi[lane];    // an earlier failed solve too
                const int sl = Chain::slot(k);
                double* const Yr = sl >= 0 ? H + sl * 2 * N : Xr;
                double* const Yi = sl >= 0 ? Yr + N : Xi;
                Yr[lane] = yr;
                Yi[lane] = yi;
                if (a.h) {
                    const size_t at = chain_h_at<Chain>(a, f, k, lane, b);
                    a.h[at] = yr;
                    a.h[at + 1] = yi;
                }
            }
            wave_sync();
            if (passing >= 0 && k == passing) {             // it leaves the solution with the next round
                vPassing = disto_abs(disto_u(Xr, Xi, a.outP, a.outM));
                wave_sync();
            }
        }
        if (lane == 0) chain_store_ratios<Chain>(a, f, b, H, N, Xr, Xi, vPassing);
        wave_sync();
    }
    if (lane == 0 && flags) a.status[b] |= flags;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32)
template <class Chain, int NP>
__device__ __forceinline__ void chain_packed(const ChainArgs& a)
{
    constexpr int passing = chain_passing<Chain>();
    static_assert(passing >= -1 && Chain::slot(0) >= 0, "one |v| at most is taken on the way, and v_0 is kept");
    __shared__ double xs[2][2][ACP_LANES];                  // [instance][re, im][position]: the solution
    __shared__ double ks[2][Chain::NKEPT][2][ACP_LANES];    // [instance][kept slot][re, im][equation]
    __shared__ double cur[2][2][ACP_LANES];                 // [instance][re, im][device of the round]
    __shared__ int32_t ends[2][2][ACP_LANES];               // [instance][drain, source][device of the round]
    const int N = a.N, M = a.M;
    const AcpInstance t = acp_instance(a.b0, a.Bc);
    const int h = t.h, r = t.r, cc = t.cc, b = t.b;
    const bool on = t.on;
    const double* Gt = ac_system_at(a.sys, cc, N);
    const double* Ct = Gt + N * N;
    const double* J1r = Ct + N * N;
    const double* J2r = Chain::NTONE == 2 && a.j2 ? a.j2 + (size_t)cc * 2 * N : J1r;
    double* Xr = xs[h][0];
    double* Xi = xs[h][1];
    const double* K = &ks[h][0][0][0];
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w1 = a.omega[f];
        double w2 = 0.0;
        if constexpr (Chain::NTONE == 2) w2 = a.omega2[f];
        bool failed = false;
        double vPassing = 0.0;
#pragma unroll 1
        for (int k = 0; k < Chain::NSOLVE; ++k) {
            double rr = 0.0, ri = 0.0;                      // entry r of the right-hand side
            if (k < Chain::NTONE) {
                const double* J = k == 0 ? J1r : J2r;
                if (r < N) { rr = J[r]; ri = J[N + r]; }
            } else {
                for (int m0 = 0; m0 < M; m0 += ACP_LANES) {
                    const int mm = m0 + r;
                    if (mm < M) {
                        const int d = a.devD[mm], g = a.devG[mm], s = a.devS[mm];
                        const cpx I = chain_device_current<Chain>(a, k, mm, cc, d, g, s, K, ACP_LANES);
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
            const double wk = Chain::freq(k, w1, w2);
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
                const double yr = failed ? 0.0 : Xr[r], yi = failed ? 0.0 : Xi[r];          // an earlier failed solve too
                const int sl = Chain::slot(k);
                if (sl >= 0) {
                    ks[h][sl][0][r] = yr;
                    ks[h][sl][1][r] = yi;
                } else {
                    Xr[r] = yr;
                    Xi[r] = yi;
                }
                if (a.h && on) {
                    const size_t at = chain_h_at<Chain>(a, f, k, r, b);
                    a.h[at] = yr;
                    a.h[at + 1] = yi;
                }
            }
            __syncthreads();
            if (passing >= 0 && k == passing) {             // the solution is overwritten by the next solve
                vPassing = disto_abs(disto_u(Xr, Xi, a.outP, a.outM));
                __syncthreads();
            }
        }
        if (on && r == 0) chain_store_ratios<Chain>(a, f, b, K, ACP_LANES, Xr, Xi, vPassing);
        __syncthreads();
    }
    if (on && r == 0 && flags) a.status[b] |= flags;
}

// ---- launch.  The output pair and the device terminals (hostD, hostG, hostS: the host's copy of the table) index
// LDS: checked here, before any launch.  packedOf(std::integral_constant<int, NP>) gives the packed kernel of NP.
template <class Chain, class PackedOf>
inline hipError_t launchChainSweep(int which, const ChainArgs& a, const int32_t* hostD, const int32_t* hostG,
                                   const int32_t* hostS, hipStream_t stream, void (*wave)(ChainArgs), PackedOf packedOf)
{
    if (a.Bc <= 0 || a.F <= 0) return hipSuccess;
    const int N = a.N;
    if (which != AC_KERNEL_WAVE && which != AC_KERNEL_PACKED) return hipErrorInvalidValue;
    if (!ac_sweep_covers(which, N)) return hipErrorInvalidValue;
    if (a.outP < 0 || a.outP >= N || a.outM < -1 || a.outM >= N || a.M < 0 || !a.ratio) return hipErrorInvalidValue;
    if ((a.omega2 != nullptr) != (Chain::NTONE == 2)) return hipErrorInvalidValue;
    if (a.M > 0 && (!hostD || !hostG || !hostS)) return hipErrorInvalidValue;
    for (int m = 0; m < a.M; ++m)
        if (hostD[m] < -1 || hostD[m] >= N || hostG[m] < -1 || hostG[m] >= N || hostS[m] < -1 || hostS[m] >= N)
            return hipErrorInvalidValue;
    if (which == AC_KERNEL_WAVE) return launchWave(wave, dim3(a.Bc), chain_wave_lds_bytes<Chain>(N), stream, a);
    acp_dispatch(N, [&](auto np) { hipLaunchKernelGGL(packedOf(np), dim3((a.Bc + 1) / 2), dim3(64), 0, stream, a); });
    return hipGetLastError();
}

} // namespace

} // namespace csim
