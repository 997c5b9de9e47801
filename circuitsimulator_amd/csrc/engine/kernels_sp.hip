// kernels_sp.hip -- S-parameter analysis: Y and S of B instances x F frequencies by one factorisation with one
// right-hand side per port (include/csim.h "S-parameter analysis", arithmetic in ac_port.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major; its J is not read).  Two kernels:
//
//   sp_sweep_wave_kernel            one wavefront per instance, N <= 63: the matrix and its K right-hand sides in LDS
//                                   (odd leading dimension >= N + K), acw_solve() of ac_sweep.hpp.
//   sp_sweep_packed_kernel<NP, KP>  N <= 32: 32 lanes per instance, lane r owns row r in registers ar/ai[NP + KP],
//                                   acp_column / acp_back.  K is rounded up to KP in {2, 4}; a padded
//                                   zero column changes no other column and is never stored.  G, then C, are staged
//                                   through an LDS tile with an odd leading dimension (the tile of the packed noise
//                                   kernel, here filled column by column): NP loads in flight instead of 2 NP.
//
// Right-hand sides: with ports (P = K > 0) the real unit vectors at the ports' branch equations; without (P = 0, the
// engine-free test entry) K arbitrary complex columns per instance.
//
// Epilogue (P > 0): the K solutions sit in LDS; one lane per instance gathers Y from the P branch equations and runs
// ac_port.hpp's P x P solve for S on LDS work planes; P * P lanes store Y and S.  Both kernels apply ac_port.hpp's
// primitives to every entry in the same order: their outputs are bit-identical.
#include <hip/hip_runtime.h>

#include "ac_port.hpp"
#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

constexpr int PP = SP_MAX_PORTS * SP_MAX_PORTS;

// LDS of one instance's epilogue: Y, S, the augmented M | 2 I and its solution
struct SpEpi {
    double yr[PP], yi[PP], sr[PP], si[PP], mr[2 * PP], mi[2 * PP], tr[PP], ti[PP];
    double sz[SP_MAX_PORTS];
    int32_t eq[SP_MAX_PORTS];
};

// kernel arguments -> LDS, with constant indices (an argument array indexed at run time would live in scratch)
__device__ __forceinline__ void sp_ports_to_lds(const SpArgs& a, SpEpi& e, int r)
{
    if (r == 0) { e.eq[0] = a.portEq[0]; e.sz[0] = a.sz[0]; }
    if (r == 1) { e.eq[1] = a.portEq[1]; e.sz[1] = a.sz[1]; }
    if (r == 2) { e.eq[2] = a.portEq[2]; e.sz[2] = a.sz[2]; }
    if (r == 3) { e.eq[3] = a.portEq[3]; e.sz[3] = a.sz[3]; }
}

// one lane: Y from the solutions (solution j at X[j * ldx ...]), then S; returns the flag of the P x P solve
__device__ __forceinline__ unsigned sp_epilogue(const SpArgs& a, SpEpi& e, bool failed, const double* Xr, const double* Xi,
                                                int ldx)
{
    const int P = a.P;
    sp_read_y(P, e.eq, failed, Xr, Xi, ldx, e.yr, e.yi);
    if (!a.s) return 0u;
    if (failed) {
        for (int t = 0; t < P * P; ++t) { e.sr[t] = 0.0; e.si[t] = 0.0; }
        return 0u;
    }
    return sp_s_from_y(P, e.yr, e.yi, e.sz, a.eps, e.mr, e.mi, e.tr, e.ti, e.sr, e.si);
}

// entry t = i * P + j of Y and S of (frequency f, instance b): [F][P][P][B] complex
__device__ __forceinline__ void sp_store(const SpArgs& a, const SpEpi& e, int f, int b, int t)
{
    const size_t at = (((size_t)f * (size_t)(a.P * a.P) + (size_t)t) * (size_t)a.B + (size_t)b) * 2;
    a.y[at] = e.yr[t];
    a.y[at + 1] = e.yi[t];
    if (a.s) {
        a.s[at] = e.sr[t];
        a.s[at + 1] = e.si[t];
    }
}

// solution c, unknown i of (frequency f, instance b): [F][K][N][B] complex
__device__ __forceinline__ size_t sp_x_at(const SpArgs& a, int f, int c, int i, int b)
{
    return ((((size_t)f * (size_t)a.K + (size_t)c) * (size_t)a.N + (size_t)i) * (size_t)a.B + (size_t)b) * 2;
}

// ---- wave per system (N <= 63)
__global__ void __launch_bounds__(64) sp_sweep_wave_kernel(SpArgs a)
{
    extern __shared__ double lds[];
    __shared__ SpEpi epi;
    const int lane = threadIdx.x;
    const int N = a.N, K = a.K, P = a.P;
    const int c0 = blockIdx.x, b = a.b0 + c0;
    const int LD = acw_ld(N, K);
    const AcwLds m = acw_carve(lds, N, K, LD);
    double *const Ar = m.Ar, *const Ai = m.Ai, *const Xr = m.Xr, *const Xi = m.Xi;      // solution c at c * 64
    const double* Gt = ac_system_at(a.sys, c0, N);
    const double* Ct = Gt + N * N;
    const double* rhs = a.rhs ? a.rhs + (size_t)c0 * (size_t)(2 * K * N) : nullptr;
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;
    sp_ports_to_lds(a, epi, lane);
    wave_sync();

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        acw_load<false>(N, LD, Gt, Ct, w, Ar, Ai, lane);
        for (int e = lane; e < N * K; e += 64) {
            const int c = e / N, i = e - c * N;
            Ar[i * LD + N + c] = P > 0 ? (i == epi.eq[c] ? 1.0 : 0.0) : rhs[2 * e];
            Ai[i * LD + N + c] = P > 0 ? 0.0 : rhs[2 * e + 1];
        }
        wave_sync();

        const bool failed = acw_solve(N, K, LD, Ar, Ai, m.Lr, m.Li, Xr, Xi, eps2, lane);
        if (failed) flags |= CSIM_ST_LU_TINY_PIVOT;
        if (a.x)
            for (int e = lane; e < N * K; e += 64) {
                const int c = e / N, i = e - c * N;
                const size_t at = sp_x_at(a, f, c, i, b);
                a.x[at] = Xr[c * 64 + i];                    // zeros when the factorisation failed
                a.x[at + 1] = Xi[c * 64 + i];
            }
        if (P > 0) {
            if (lane == 0) flags |= sp_epilogue(a, epi, failed, Xr, Xi, 64);
            wave_sync();
            if (lane < P * P) sp_store(a, epi, f, b, lane);
        }
        wave_sync();
    }
    if (lane == 0 && flags) a.status[b] |= flags;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32), KP >= K right-hand-side registers
template <int NP, int KP>
__global__ void __launch_bounds__(64) sp_sweep_packed_kernel(SpArgs a)
{
    constexpr int LDT = NP + 1;                             // odd: lane r reading word r * LDT + j is conflict-free
    __shared__ double tile[2][NP * LDT];                    // [instance] staged G, then C, as rows of A
    __shared__ double xs[2][2][KP * ACP_LANES];             // [instance][re, im][solution c at c * 32]
    __shared__ SpEpi epis[2];
    const int N = a.N, K = a.K, P = a.P;
    const AcpInstance t = acp_instance(a.b0, a.Bc);
    const int h = t.h, r = t.r, cc = t.cc, b = t.b;
    const bool on = t.on;
    const double* Gt = ac_system_at(a.sys, cc, N);
    const double* Ct = Gt + N * N;
    const double* rhs = a.rhs ? a.rhs + (size_t)cc * (size_t)(2 * K * N) : nullptr;
    double* T = tile[h];
    double* Xr = xs[h][0];
    double* Xi = xs[h][1];
    SpEpi& epi = epis[h];
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;
    sp_ports_to_lds(a, epi, r);
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
    __syncthreads();

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        double ar[NP + KP], ai[NP + KP];
        stage(Gt);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) ar[j] = (r < N && j < N) ? T[r * LDT + j] : 0.0;
        __syncthreads();
        stage(Ct);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) ai[j] = (r < N && j < N) ? w * T[r * LDT + j] : 0.0;
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            const bool in = c < K && r < N;
            if (P > 0) {
                ar[NP + c] = (in && r == epi.eq[c]) ? 1.0 : 0.0;
                ai[NP + c] = 0.0;
            } else {
                ar[NP + c] = in ? rhs[2 * (c * N + r)] : 0.0;
                ai[NP + c] = in ? rhs[2 * (c * N + r) + 1] : 0.0;
            }
        }
        int pos = r;
        bool failed = false;
        acp_column<NP, KP, 0>(ar, ai, N, pos, failed, eps2, h);
        acp_back<NP, KP, NP - 1>(ar, ai, N, pos, Xr, Xi);
        if (failed) {
            flags |= CSIM_ST_LU_TINY_PIVOT;
#pragma unroll
            for (int c = 0; c < KP; ++c) {                  // as the wave kernel leaves them: zero vectors
                Xr[c * ACP_LANES + r] = 0.0;
                Xi[c * ACP_LANES + r] = 0.0;
            }
        }
        __syncthreads();
        if (a.x && on && r < N)
            for (int c = 0; c < K; ++c) {
                const size_t at = sp_x_at(a, f, c, r, b);
                a.x[at] = Xr[c * ACP_LANES + r];
                a.x[at + 1] = Xi[c * ACP_LANES + r];
            }
        if (P > 0) {
            if (r == 0) flags |= sp_epilogue(a, epi, failed, Xr, Xi, ACP_LANES);
            __syncthreads();
            if (on && r < P * P) sp_store(a, epi, f, b, r);
        }
        __syncthreads();
    }
    if (on && r == 0 && flags) a.status[b] |= flags;
}

} // namespace

hipError_t launchSpSweep(int which, const SpArgs& a, hipStream_t stream)
{
    if (a.Bc <= 0 || a.F <= 0) return hipSuccess;
    const int N = a.N;
    if (!ac_sweep_covers(which, N)) return hipErrorInvalidValue;
    if (a.K < 1 || a.K > SP_MAX_PORTS || (a.P != 0 && a.P != a.K)) return hipErrorInvalidValue;
    for (int p = 0; p < a.P; ++p)
        if (a.portEq[p] < 0 || a.portEq[p] >= N) return hipErrorInvalidValue;       // they index LDS
    if (a.P == 0 ? (!a.rhs || !a.x) : !a.y) return hipErrorInvalidValue;
    if (which == AC_KERNEL_PACKED) {
        acp_dispatch(N, [&](auto np) {
            constexpr int NP = decltype(np)::value;
            const dim3 grid((a.Bc + 1) / 2);
            if (a.K <= 2) hipLaunchKernelGGL((sp_sweep_packed_kernel<NP, 2>), grid, dim3(64), 0, stream, a);
            else hipLaunchKernelGGL((sp_sweep_packed_kernel<NP, 4>), grid, dim3(64), 0, stream, a);
        });
    } else {
        const size_t lds = acw_lds_bytes(N, a.K);
        if (lds + sizeof(SpEpi) > 64 * 1024)
            (void)hipFuncSetAttribute((const void*)sp_sweep_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(sp_sweep_wave_kernel, dim3(a.Bc), dim3(64), lds, stream, a);
    }
    return hipGetLastError();
}

} // namespace csim
