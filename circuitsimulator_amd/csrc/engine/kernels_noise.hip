// kernels_noise.hip -- small-signal noise analysis: output noise of B instances x F frequencies by one adjoint
// solve each (include/csim.h "Noise analysis", arithmetic in ac_noise.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major).  Three kernels:
//
//   noise_psd_kernel        one thread per (generator, instance), ONCE per instance: current PSD of every resistor
//                           (kT4 / R) and MOSFET channel (kT4 2/3 |gg|, mos_eval at x_op as in the G pass).
//   ac_noise_wave_kernel    one wavefront per instance, N <= 63: A^T in LDS, acw_solve() of ac_sweep.hpp, epilogue.
//   ac_noise_packed_kernel  N <= 32: 32 lanes per instance, lane r owns row r of A^T, acp_column / acp_back.
//   ac_noise_block_kernel   opt-in (ac_kernel=block), N <= 1024: a 256-thread workgroup per instance, A^T in a global
//                           scratch, acb_solve() of ac_block.hpp; the contributions go through LDS, 256 at a time,
//                           and one thread adds them in ascending order.
//
// The transposed load.  Entry (i, j) of A^T is word i * N + j of the column-major G and C.  The wave kernel walks
// those words in order and scatters them into LDS: consecutive lanes read consecutive addresses, nothing to
// stage.  In the packed kernel lane r wants row r, register j: the lanes of one load would be N words apart,
// every lane its own cache line, at every frequency.  So that kernel stages: the 32 lanes of a system copy G,
// then C, in address order into an LDS tile with an odd leading dimension and each lane reads its row back from
// there (a column walk with an odd stride is conflict-free).  In the AC kernels the roles are the other way
// round: there the packed kernel reads column-major directly.
//
// Epilogue: y in LDS; the lanes stride over the generators, the contributions travel to every lane in ascending
// order (readlane / shuffle) and are added in that order; one lane stores the total.  Both kernels apply
// ac_noise.hpp's primitives to every entry in the same order: their outputs are bit-identical.
#include <hip/hip_runtime.h>

#include "ac_noise.hpp"
#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

__global__ void __launch_bounds__(256) noise_psd_kernel(GenPlan pl, const int32_t* __restrict__ srcElem, int S,
                                                        const double* __restrict__ params, int B, int b0, int Bc,
                                                        const double* __restrict__ xop, double kT4,
                                                        double* __restrict__ psd, size_t psdStride, size_t psdOff)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)S * (size_t)Bc) return;
    const int s = (int)(t / (size_t)Bc), c = (int)(t - (size_t)s * (size_t)Bc);
    const size_t b = (size_t)b0 + (size_t)c;
    const int e = srcElem[s];
    const int kind = pl.kind[e], slot = pl.slot[e];
    auto P = [&](int p) { return params[(size_t)(slot + p) * (size_t)B + b]; };
    double v = 0.0;
    if (kind == CSIM_R) {
        const double R = P(0);
        v = (R == 0.0) ? 0.0 : kT4 * (1.0 / R);                              // element.cpp:20-24: no stamp, no noise
    } else if (kind == CSIM_NMOS || kind == CSIM_PMOS) {
        const int32_t* q = pl.eq + 4 * e;
        auto X = [&](int eq) { return eq >= 0 ? xop[(size_t)eq * (size_t)B + b] : 0.0; };
        const MosLin m = mos_eval(kind == CSIM_PMOS, P(0), P(1), P(2), pl.k.mos_off_gds, X(q[0]), X(q[1]), X(q[2]));
        v = kT4 * ((2.0 / 3.0) * fabs(m.gg));
    }
    psd[(size_t)s * psdStride + psdOff + (size_t)c] = v;
}

// generator s of chunk instance c: psd[s * psdStride + psdOff + c]
__device__ __forceinline__ double psd_at(const NoiseArgs& a, int s, int c)
{
    return a.psd[(size_t)s * a.psdStride + a.psdOff + (size_t)c];
}

// the outputs of (frequency f, instance b) that one lane writes
__device__ __forceinline__ void noise_store(const NoiseArgs& a, int f, int b, bool failed, double total,
                                            const double* Xr, const double* Xi)
{
    a.onoise[(size_t)f * (size_t)a.B + (size_t)b] = total;
    if (a.gain && a.inKind != NOISE_IN_NONE) {
        const cpx g = failed ? cpx{0.0, 0.0} : noise_gain(Xr, Xi, a.inKind, a.inA, a.inB);
        const size_t at = ((size_t)f * (size_t)a.B + (size_t)b) * 2;
        a.gain[at] = g.re;
        a.gain[at + 1] = g.im;
    }
}

// ---- wave per system (N <= 63)
__global__ void __launch_bounds__(64) ac_noise_wave_kernel(NoiseArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int N = a.N, S = a.S;
    const int c = blockIdx.x, b = a.b0 + c;
    const int LD = acw_ld(N, 1);
    const AcwLds m = acw_carve(lds, N, 1, LD);
    double *const Ar = m.Ar, *const Ai = m.Ai, *const Xr = m.Xr, *const Xi = m.Xi;
    const double* Gt = ac_system_at(a.sys, c, N);
    const double* Ct = Gt + N * N;
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        acw_load<true>(N, LD, Gt, Ct, w, Ar, Ai, lane);
        for (int i = lane; i < N; i += 64) {
            Ar[i * LD + N] = i == a.outP ? 1.0 : (i == a.outM ? -1.0 : 0.0);
            Ai[i * LD + N] = 0.0;
        }
        wave_sync();

        const bool failed = acw_solve(N, 1, LD, Ar, Ai, m.Lr, m.Li, Xr, Xi, eps2, lane);
        if (failed) flags |= CSIM_ST_LU_TINY_PIVOT;
        if (a.y)
            for (int p = lane; p < N; p += 64) {
                const size_t at = (((size_t)f * (size_t)N + (size_t)p) * (size_t)a.B + (size_t)b) * 2;
                a.y[at] = Xr[p];                             // zeros when the factorisation failed
                a.y[at + 1] = Xi[p];
            }
        double total = 0.0;
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            double cv = 0.0;
            if (s < S) {
                if (!failed) cv = noise_contrib(noise_transfer(Xr, Xi, a.srcA[s], a.srcB[s]), psd_at(a, s, c));
                if (a.contrib) a.contrib[((size_t)f * (size_t)S + (size_t)s) * (size_t)a.B + (size_t)b] = cv;
            }
            const int cnt = min(64, S - s0);
            for (int t = 0; t < cnt; ++t) total = total + read_lane(cv, t);
        }
        if (lane == 0) noise_store(a, f, b, failed, total, Xr, Xi);
        wave_sync();
    }
    if (lane == 0 && flags) a.status[b] |= flags;
}

// ---- 256-thread workgroup per system (N <= 1024)
__global__ void __launch_bounds__(ACB_THREADS) ac_noise_block_kernel(NoiseArgs a)
{
    extern __shared__ double lds[];
    __shared__ double cbuf[ACB_THREADS];
    const int tid = threadIdx.x;
    const int N = a.N, S = a.S;
    const int c = blockIdx.x, b = a.b0 + c;
    const int LD = acw_ld(N, 1);
    const AcbLds m = acb_carve(lds, N, 1);
    double *const Xr = m.Xr, *const Xi = m.Xi;
    double* const Ar = acb_work_at(a.work, c, N, LD);
    double* const Ai = Ar + N * LD;
    const double* Gt = ac_system_at(a.sys, c, N);
    const double* Ct = Gt + N * N;
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        acb_load<true>(N, LD, Gt, Ct, w, Ar, Ai, tid);
        for (int i = tid; i < N; i += ACB_THREADS) {
            Ar[i * LD + N] = i == a.outP ? 1.0 : (i == a.outM ? -1.0 : 0.0);
            Ai[i * LD + N] = 0.0;
        }
        acb_sync();

        const bool failed = acb_solve(N, 1, LD, Ar, Ai, m.Lr, m.Li, m.rows, Xr, Xi, eps2, tid);
        if (failed) flags |= CSIM_ST_LU_TINY_PIVOT;
        if (a.y)
            for (int p = tid; p < N; p += ACB_THREADS) {
                const size_t at = (((size_t)f * (size_t)N + (size_t)p) * (size_t)a.B + (size_t)b) * 2;
                a.y[at] = Xr[p];                             // zeros when the factorisation failed
                a.y[at + 1] = Xi[p];
            }
        double total = 0.0;
        for (int s0 = 0; s0 < S; s0 += ACB_THREADS) {
            const int s = s0 + tid;
            double cv = 0.0;
            if (s < S) {
                if (!failed) cv = noise_contrib(noise_transfer(Xr, Xi, a.srcA[s], a.srcB[s]), psd_at(a, s, c));
                if (a.contrib) a.contrib[((size_t)f * (size_t)S + (size_t)s) * (size_t)a.B + (size_t)b] = cv;
            }
            cbuf[tid] = cv;
            __syncthreads();
            if (tid == 0) {
                const int cnt = min(ACB_THREADS, S - s0);
                for (int t = 0; t < cnt; ++t) total = total + cbuf[t];
            }
            __syncthreads();
        }
        if (tid == 0) noise_store(a, f, b, failed, total, Xr, Xi);
        __syncthreads();
    }
    if (tid == 0 && flags) a.status[b] |= flags;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32)
template <int NP>
__global__ void __launch_bounds__(64) ac_noise_packed_kernel(NoiseArgs a)
{
    constexpr int LDT = NP + 1;                             // odd: lane r reading word r * LDT + j is conflict-free
    __shared__ double tile[2][NP * LDT];                    // [instance] staged G, then C, as rows of A^T
    __shared__ double xs[2][2][ACP_LANES];                  // [instance][re, im][position]
    const int N = a.N, S = a.S;
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
    // word idx = i * N + j of a column-major plane -> tile row i, column j; idx advances by 32 per step
    const int di = ACP_LANES / N, dj = ACP_LANES % N, i0 = r / N, j0 = r % N;
    auto stage = [&](const double* src) {
        int i = i0, j = j0;
        for (int idx = r; idx < N * N; idx += ACP_LANES) {
            T[i * LDT + j] = src[idx];
            i += di;
            j += dj;
            if (j >= N) { j -= N; ++i; }
        }
    };

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        double ar[NP + 1], ai[NP + 1];
        stage(Gt);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) ar[j] = (r < N && j < N) ? T[r * LDT + j] : 0.0;
        __syncthreads();
        stage(Ct);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) ai[j] = (r < N && j < N) ? w * T[r * LDT + j] : 0.0;
        ar[NP] = r == a.outP ? 1.0 : (r == a.outM ? -1.0 : 0.0);
        ai[NP] = 0.0;
        int pos = r;
        bool failed = false;
        acp_column<NP, 1, 0>(ar, ai, N, pos, failed, eps2, h);
        acp_back<NP, 1, NP - 1>(ar, ai, N, pos, Xr, Xi);
        if (failed) {
            flags |= CSIM_ST_LU_TINY_PIVOT;
            Xr[r] = 0.0;                                    // as the wave kernel leaves it: the zero vector
            Xi[r] = 0.0;
        }
        __syncthreads();
        if (a.y && on)
            for (int p = r; p < N; p += ACP_LANES) {
                const size_t at = (((size_t)f * (size_t)N + (size_t)p) * (size_t)a.B + (size_t)b) * 2;
                a.y[at] = Xr[p];
                a.y[at + 1] = Xi[p];
            }
        double total = 0.0;
        for (int s0 = 0; s0 < S; s0 += ACP_LANES) {
            const int s = s0 + r;
            double cv = 0.0;
            if (s < S) {
                if (!failed) cv = noise_contrib(noise_transfer(Xr, Xi, a.srcA[s], a.srcB[s]), psd_at(a, s, cc));
                if (a.contrib && on) a.contrib[((size_t)f * (size_t)S + (size_t)s) * (size_t)a.B + (size_t)b] = cv;
            }
            const int cnt = min(ACP_LANES, S - s0);
            for (int t = 0; t < cnt; ++t) total = total + __shfl(cv, t, ACP_LANES);
        }
        if (on && r == 0) noise_store(a, f, b, failed, total, Xr, Xi);
        __syncthreads();
    }
    if (on && r == 0 && flags) a.status[b] |= flags;
}

} // namespace

hipError_t launchNoisePsd(const GenPlan& pl, const int32_t* dSrcElem, int S, const double* dParams, int B, int b0, int Bc,
                          const double* dXop, double kT4, double* dPsd, size_t psdStride, size_t psdOff, hipStream_t stream)
{
    if (Bc <= 0 || S <= 0) return hipSuccess;
    const size_t total = (size_t)S * (size_t)Bc;
    hipLaunchKernelGGL(noise_psd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, pl, dSrcElem, S, dParams,
                       B, b0, Bc, dXop, kT4, dPsd, psdStride, psdOff);
    return hipGetLastError();
}

hipError_t launchNoiseSweep(int which, const NoiseArgs& a, hipStream_t stream)
{
    if (a.Bc <= 0 || a.F <= 0) return hipSuccess;
    const int N = a.N;
    if (!ac_sweep_covers(which, N)) return hipErrorInvalidValue;
    if (a.outP < 0 || a.outP >= N || a.outM < -1 || a.outM >= N || a.S < 0) return hipErrorInvalidValue;
    if (which == AC_KERNEL_BLOCK) {
        if (!a.work) return hipErrorInvalidValue;
        hipLaunchKernelGGL(ac_noise_block_kernel, dim3(a.Bc), dim3(ACB_THREADS), acb_lds_bytes(N, 1), stream, a);
    } else if (which == AC_KERNEL_PACKED) {
        acp_dispatch(N, [&](auto np) {
            hipLaunchKernelGGL(ac_noise_packed_kernel<decltype(np)::value>, dim3((a.Bc + 1) / 2), dim3(64), 0, stream, a);
        });
    } else {
        const size_t lds = acw_lds_bytes(N, 1);
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute((const void*)ac_noise_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(ac_noise_wave_kernel, dim3(a.Bc), dim3(64), lds, stream, a);
    }
    return hipGetLastError();
}

} // namespace csim
