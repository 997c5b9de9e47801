// kernels_stb.hip -- loop-gain analysis: T of B instances x F frequencies by Middlebrook's double injection at a V source
// in series in the loop, one factorisation with two right-hand sides per point; then phase and gain margins per
// instance (include/csim.h "Loop-gain analysis", arithmetic in ac_stb.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major; its J is not read).  Three kernels:
//
//   stb_sweep_wave_kernel        one wavefront per instance, N <= 63: the matrix and its two right-hand sides in LDS
//                                (odd leading dimension >= N + 2), acw_load / acw_solve of ac_sweep.hpp.
//   stb_sweep_packed_kernel<NP>  N <= 32: 32 lanes per instance, lane r owns row r in registers ar/ai[NP + 2],
//                                acp_column<NP, 2, 0> / acp_back.  G, then C, are staged through an LDS tile with an odd
//                                leading dimension, as the packed S-parameter kernel stages them.
//   stb_margins_kernel           one lane per instance walks the F loop gains of [F][B] (coalesced over the instances),
//                                once, after every chunk of the sweep has run.
//
// Right-hand sides: column 0 the real unit vector at the probe's branch equation, column 1 +1.0 at the equation of its
// + node.  Epilogue: the two solutions sit in LDS; one lane per instance reads vx, vy, ib and stores T.  The solutions
// go to memory only when the caller gives a buffer.  Both sweep kernels apply ac_stb.hpp's primitives in the same
// order: their outputs are bit-identical.
#include <hip/hip_runtime.h>

#include "ac_stb.hpp"
#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

// solution c, unknown i of (frequency f, instance b): [F][2][N][B] complex
__device__ __forceinline__ size_t stb_x_at(const StbArgs& a, int f, int c, int i, int b)
{
    return ((((size_t)f * 2 + (size_t)c) * (size_t)a.N + (size_t)i) * (size_t)a.B + (size_t)b) * 2;
}

// one lane: T of (frequency f, instance b) from the two solutions in LDS (solution c at X[c * ldx ...]); returns flags
__device__ __forceinline__ unsigned stb_store_t(const StbArgs& a, int f, int b, bool failed, const double* Xr,
                                                const double* Xi, int ldx)
{
    unsigned fl = 0u;
    const cpx t = stb_loop_gain({Xr[a.eqP], Xi[a.eqP]}, {Xr[a.eqM], Xi[a.eqM]}, {Xr[ldx + a.eqBr], Xi[ldx + a.eqBr]}, failed, &fl);
    const size_t at = ((size_t)f * (size_t)a.B + (size_t)b) * 2;
    a.t[at] = t.re;
    a.t[at + 1] = t.im;
    return fl;
}

// ---- wave per system (N <= 63)
__global__ void __launch_bounds__(64) stb_sweep_wave_kernel(StbArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int N = a.N;
    const int c0 = blockIdx.x, b = a.b0 + c0;
    const int LD = acw_ld(N, 2);
    const AcwLds m = acw_carve(lds, N, 2, LD);
    double *const Ar = m.Ar, *const Ai = m.Ai, *const Xr = m.Xr, *const Xi = m.Xi;      // solution c at c * 64
    const double* Gt = ac_system_at(a.sys, c0, N);
    const double* Ct = Gt + N * N;
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        acw_load<false>(N, LD, Gt, Ct, w, Ar, Ai, lane);
        if (lane < N) {
            Ar[lane * LD + N] = lane == a.eqBr ? 1.0 : 0.0;
            Ai[lane * LD + N] = 0.0;
            Ar[lane * LD + N + 1] = lane == a.eqP ? 1.0 : 0.0;
            Ai[lane * LD + N + 1] = 0.0;
        }
        wave_sync();

        const bool failed = acw_solve(N, 2, LD, Ar, Ai, m.Lr, m.Li, Xr, Xi, eps2, lane);
        if (a.x && lane < N)
            for (int c = 0; c < 2; ++c) {
                const size_t at = stb_x_at(a, f, c, lane, b);
                a.x[at] = Xr[c * 64 + lane];                 // zeros when the factorisation failed
                a.x[at + 1] = Xi[c * 64 + lane];
            }
        if (lane == 0) flags |= stb_store_t(a, f, b, failed, Xr, Xi, 64);
        wave_sync();
    }
    if (lane == 0 && flags) a.status[b] |= flags;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32)
template <int NP>
__global__ void __launch_bounds__(64) stb_sweep_packed_kernel(StbArgs a)
{
    constexpr int LDT = NP + 1;                             // odd: lane r reading word r * LDT + j is conflict-free
    __shared__ double tile[2][NP * LDT];                    // [instance] staged G, then C, as rows of A
    __shared__ double xs[2][2][2 * ACP_LANES];              // [instance][re, im][solution c at c * 32]
    const int N = a.N;
    const AcpInstance t = acp_instance(a.b0, a.Bc);
    const int h = t.h, r = t.r, cc = t.cc, b = t.b;
    const bool on = t.on;
    const double* Gt = ac_system_at(a.sys, cc, N);
    const double* Ct = Gt + N * N;
    double* T = tile[h];
    double* Xr = xs[h][0];
    double* Xi = xs[h][1];
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;
    // word idx = j * N + i of a column-major plane -> tile row i, column j; idx advances by 32 per step
    const int dj = ACP_LANES / N, di = ACP_LANES % N, j0 = r / N, i0 = r % N;
    auto stage = [&](const double* src) {
        int i = i0, j = j0;
        for (int idx = r; idx < N * N; idx += ACP_LANES) {
            T[i * LDT + j] = src[idx];
            j += dj;
            i += di;
            if (i >= N) { i -= N; ++j; }
        }
    };

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        double ar[NP + 2], ai[NP + 2];
        stage(Gt);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) ar[j] = (r < N && j < N) ? T[r * LDT + j] : 0.0;
        __syncthreads();
        stage(Ct);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) ai[j] = (r < N && j < N) ? w * T[r * LDT + j] : 0.0;
        ar[NP] = (r < N && r == a.eqBr) ? 1.0 : 0.0;
        ai[NP] = 0.0;
        ar[NP + 1] = (r < N && r == a.eqP) ? 1.0 : 0.0;
        ai[NP + 1] = 0.0;
        int pos = r;
        bool failed = false;
        acp_column<NP, 2, 0>(ar, ai, N, pos, failed, eps2, h);
        acp_back<NP, 2, NP - 1>(ar, ai, N, pos, Xr, Xi);
        if (failed) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {                   // as the wave kernel leaves them: zero vectors
                Xr[c * ACP_LANES + r] = 0.0;
                Xi[c * ACP_LANES + r] = 0.0;
            }
        }
        __syncthreads();
        if (a.x && on && r < N)
            for (int c = 0; c < 2; ++c) {
                const size_t at = stb_x_at(a, f, c, r, b);
                a.x[at] = Xr[c * ACP_LANES + r];
                a.x[at + 1] = Xi[c * ACP_LANES + r];
            }
        if (on && r == 0) flags |= stb_store_t(a, f, b, failed, Xr, Xi, ACP_LANES);
        __syncthreads();
    }
    if (on && r == 0 && flags) a.status[b] |= flags;
}

// ---- margins: one lane per instance
__global__ void __launch_bounds__(256) stb_margins_kernel(int F, int B, const double* __restrict__ freqs,
                                                          const double* __restrict__ t, double* __restrict__ margins,
                                                          int32_t* __restrict__ found)
{
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (size_t)B) return;
    const StbMargins r = stb_margins(F, freqs, t + 2 * b, (size_t)B);
    margins[b] = r.pm;
    margins[(size_t)B + b] = r.fc;
    margins[2 * (size_t)B + b] = r.gm;
    margins[3 * (size_t)B + b] = r.f180;
    if (found) found[b] = r.found;
}

} // namespace

hipError_t launchStbSweep(int which, const StbArgs& a, hipStream_t stream)
{
    if (a.Bc <= 0 || a.F <= 0) return hipSuccess;
    const int N = a.N;
    if (which != AC_KERNEL_WAVE && which != AC_KERNEL_PACKED) return hipErrorInvalidValue;
    if (!ac_sweep_covers(which, N)) return hipErrorInvalidValue;
    for (int eq : {a.eqP, a.eqM, a.eqBr})
        if (eq < 0 || eq >= N) return hipErrorInvalidValue;                         // they index LDS
    if (!a.t) return hipErrorInvalidValue;
    if (which == AC_KERNEL_PACKED) {
        acp_dispatch(N, [&](auto np) {
            hipLaunchKernelGGL(stb_sweep_packed_kernel<decltype(np)::value>, dim3((a.Bc + 1) / 2), dim3(64), 0, stream, a);
        });
    } else {
        const size_t lds = acw_lds_bytes(N, 2);
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute((const void*)stb_sweep_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(stb_sweep_wave_kernel, dim3(a.Bc), dim3(64), lds, stream, a);
    }
    return hipGetLastError();
}

hipError_t launchStbMargins(int F, int B, const double* dFreqs, const double* dT, double* dMargins, int32_t* dFound,
                            hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    if (F < 0 || !dMargins || (F > 0 && (!dFreqs || !dT))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stb_margins_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, F, B, dFreqs, dT, dMargins,
                       dFound);
    return hipGetLastError();
}

} // namespace csim
