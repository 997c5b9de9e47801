// kernels_ac.hip -- small-signal AC analysis: (G(x_op) + jwC) v = J for B instances x F frequencies.
//
// AC is the small-signal limit of the engine's own backward-Euler transient (include/csim.h "AC analysis").
// Three kernels:
//
//   ac_assemble_kernel   one wavefront per instance, ONCE per instance: the transient plan's gather
//                        (device_common.hpp assemble(), linear in the term vector) run with two term vectors.
//                        G pass: 1/R, incidence ones, tran_gmin, the MOSFET gd/gg/gs at x_op, companion terms
//                        zero.  C pass: only C, L, Cj0/2, Cj0 in the companion slots (C/dt, L/dt, ... with dt = 1).
//                        The RHS columns of the two passes carry the AC excitation (re, im) in the source
//                        slots.  Same sparsity, signs and accumulation order as the transient.  Output per
//                        instance: G and C column-major [N][N], then J re [N], J im [N].
//   ac_sweep_wave_kernel one wavefront per instance, N <= 63: for every frequency the augmented complex
//                        matrix in LDS (re / im planes, odd leading dimension), pivot by max-reduction and
//                        ballot, rows swapped in LDS, elimination spread over the trailing sub-matrix.
//   ac_sweep_packed_kernel  N <= 32: 32 lanes per instance, two instances per wavefront.  Lane r owns one row;
//                        column j is register j (re and im: 2 (NP + 1) doubles, NP = N rounded up to 8).
//                        Rows are exchanged logically: every lane carries the row position it holds; the pivot
//                        row (a run-time lane) reaches the others by a bpermute per register.
//
//   ac_assemble_big_kernel / ac_sweep_block_kernel  the opt-in block shape (ac_kernel=block), 1 <= N <= 1024: the
//                        assembly scatters every structural non-zero straight to its column-major word (no dense
//                        N x LD stage in LDS, impossible from N ~ 140), and one 256-thread workgroup per instance
//                        solves on planes in a global scratch (ac_block.hpp).
//
// All sweep kernels apply ac_lu.hpp's primitives to every entry in the same order: their outputs are
// bit-identical (tests/test_ac_gpu.py and tests/test_ac_block_gpu.py force each through the engine option ac_kernel).
#include <hip/hip_runtime.h>

#include "ac_lu.hpp"
#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

// G pass (companion terms zero) or C pass (only the companion slots, as C, L, Cj0/2, Cj0) of the
// transient's term vector; the source slots carry src[e] (re or im part of the AC excitation)
template <bool CPASS>
__device__ void ac_terms(const GenPlan& pl, const double* Pv, const double* x, const double* src, double* T, int lane)
{
    for (int e = lane; e < pl.nElem; e += 64) {
        const int kind = pl.kind[e], s = pl.slot[e], tb = pl.termBase[e];
        if (kind == CSIM_R) {
            const double R = Pv[s];
            T[tb + T_R_G] = CPASS ? 0.0 : ((R == 0.0) ? 0.0 : 1.0 / R);     // element.cpp:20-24
        } else if (kind == CSIM_C) {
            const double C = Pv[s];
            T[tb + T_C_GC] = (CPASS && C > 0.0) ? C : 0.0;                  // tanalisis.cpp:65-67
            T[tb + T_C_IH] = 0.0;
        } else if (kind == CSIM_L) {
            const double L = Pv[s];
            const bool on = L > 0.0;                                         // tanalisis.cpp:296
            T[tb + T_L_REQ] = (CPASS && on) ? L : 0.0;
            T[tb + T_L_VH] = 0.0;
            T[tb + T_L_ONE] = (!CPASS && on) ? 1.0 : 0.0;
        } else if (kind == CSIM_V || kind == CSIM_I) {
            T[tb + T_SRC_VAL] = src[e];
        } else if (kind == CSIM_NMOS || kind == CSIM_PMOS) {
            for (int t = 0; t <= T_M_IHDB; ++t) T[tb + t] = 0.0;
            if (CPASS) {
                const double Cj0 = Pv[s + 3];
                const double Ch = 0.5 * Cj0;                                 // tanalisis.cpp:337-341
                T[tb + T_M_GCH] = Ch > 0.0 ? Ch : 0.0;
                T[tb + T_M_GCF] = Cj0 > 0.0 ? Cj0 : 0.0;
            } else {
                const int32_t* q = pl.eq + 4 * e;
                const MosLin m = mos_eval(kind == CSIM_PMOS, Pv[s + 0], Pv[s + 1], Pv[s + 2], pl.k.mos_off_gds,
                                          volt_of(x, q[0]), volt_of(x, q[1]), volt_of(x, q[2]));
                T[tb + T_M_GD] = m.gd;
                T[tb + T_M_GG] = m.gg;
                T[tb + T_M_GS] = m.gs;
            }
        }
    }
    if (lane == 0) {
        T[pl.termOne] = CPASS ? 0.0 : 1.0;
        T[pl.termGmin] = CPASS ? 0.0 : pl.k.tran_gmin;                      // tanalisis.cpp:356
    }
    wave_sync();
}

// dense matrix of the LDS system -> column-major [N][N] + its RHS column
__device__ void ac_store(const double* Gm, int N, int LD, double* mat, double* rhs, int lane)
{
    for (int idx = lane; idx < N * N; idx += 64) {
        const int j = idx / N, i = idx - j * N;
        mat[idx] = Gm[i * LD + j];
    }
    for (int i = lane; i < N; i += 64) rhs[i] = Gm[i * LD + N];
    wave_sync();
}

__global__ void __launch_bounds__(64) ac_assemble_kernel(GenPlan pl, const double* __restrict__ acRe,
                                                         const double* __restrict__ acIm, const double* __restrict__ params,
                                                         int B, int b0, const double* __restrict__ xop, double* __restrict__ sys)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, b = b0 + c;
    const int N = pl.N, LD = pl.LD;
    double* T = lds;
    double* Pv = T + pl.nTerms;
    double* x = Pv + pl.P;
    double* Gm = x + N;
    for (int p = lane; p < pl.P; p += 64) Pv[p] = params[(size_t)p * B + b];
    for (int i = lane; i < N; i += 64) x[i] = xop[(size_t)i * B + b];
    wave_sync();
    double* out = sys + (size_t)c * (2 * N * N + 2 * N);
    ac_terms<false>(pl, Pv, x, acRe, T, lane);
    assemble(pl, T, Gm, lane);
    ac_store(Gm, N, LD, out, out + 2 * N * N, lane);
    ac_terms<true>(pl, Pv, x, acIm, T, lane);
    assemble(pl, T, Gm, lane);
    ac_store(Gm, N, LD, out + N * N, out + 2 * N * N + N, lane);
}

// The assembly without the dense LDS stage: T, Pv and x in LDS (they fit whenever the engine was created), the
// instance's 2 N^2 + 2 N doubles zero-filled, then every structural non-zero accumulated in gCon order as assemble()
// does and stored to its column-major word, the right-hand side rows from iPtr / iRow.  One accumulation and one
// store per entry: the system is bit for bit ac_assemble_kernel's.
__device__ void ac_scatter(const GenPlan& pl, const double* T, double* mat, double* rhs, int lane)
{
    const int N = pl.N, LD = pl.LD;
    for (int n = lane; n < pl.nnzG; n += 64) {
        double acc = 0.0;
        for (int c = pl.gPtr[n]; c < pl.gPtr[n + 1]; ++c) {
            const int con = pl.gCon[c];
            const double v = T[con >> 1];
            acc = (con & 1) ? acc - v : acc + v;
        }
        const int pos = pl.gPos[n], i = pos / LD, j = pos - i * LD;
        mat[(size_t)j * N + i] = acc;
    }
    for (int n = lane; n < pl.nnzI; n += 64) {
        double acc = 0.0;
        for (int c = pl.iPtr[n]; c < pl.iPtr[n + 1]; ++c) {
            const int con = pl.iCon[c];
            const double v = T[con >> 1];
            acc = (con & 1) ? acc - v : acc + v;
        }
        rhs[pl.iRow[n]] = acc;
    }
    wave_sync();
}

__global__ void __launch_bounds__(64) ac_assemble_big_kernel(GenPlan pl, const double* __restrict__ acRe,
                                                             const double* __restrict__ acIm, const double* __restrict__ params,
                                                             int B, int b0, const double* __restrict__ xop, double* __restrict__ sys)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, b = b0 + c;
    const int N = pl.N;
    double* T = lds;
    double* Pv = T + pl.nTerms;
    double* x = Pv + pl.P;
    for (int p = lane; p < pl.P; p += 64) Pv[p] = params[(size_t)p * B + b];
    for (int i = lane; i < N; i += 64) x[i] = xop[(size_t)i * B + b];
    const size_t per = (size_t)2 * N * N + (size_t)2 * N;
    double* out = sys + (size_t)c * per;
    for (size_t i = lane; i < per; i += 64) out[i] = 0.0;
    __threadfence_block();
    wave_sync();
    ac_terms<false>(pl, Pv, x, acRe, T, lane);
    ac_scatter(pl, T, out, out + (size_t)2 * N * N, lane);
    ac_terms<true>(pl, Pv, x, acIm, T, lane);
    ac_scatter(pl, T, out + (size_t)N * N, out + (size_t)2 * N * N + N, lane);
}

// output offset of (frequency f, probe p, instance b), complex pairs: 64-bit
__device__ __forceinline__ size_t ac_out_at(int f, int p, int nProbe, int B, int b)
{
    return (((size_t)f * (size_t)nProbe + (size_t)p) * (size_t)B + (size_t)b) * 2;
}

// ---- wave per system (N <= 63)
__global__ void __launch_bounds__(64) ac_sweep_wave_kernel(int N, const double* __restrict__ sys, const double* __restrict__ omega,
                                                           int F, const int32_t* __restrict__ probe, int nProbe, int B, int b0,
                                                           double eps, double* __restrict__ out, uint32_t* __restrict__ status)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, b = b0 + c;
    const int LD = acw_ld(N, 1);
    const AcwLds m = acw_carve(lds, N, 1, LD);
    double *const Ar = m.Ar, *const Ai = m.Ai, *const Xr = m.Xr, *const Xi = m.Xi;
    const double* Gt = ac_system_at(sys, c, N);
    const double* Ct = Gt + N * N;
    const double* Jr = Ct + N * N;
    const double* Ji = Jr + N;
    const double eps2 = eps * eps;
    unsigned flags = 0u;

    for (int f = 0; f < F; ++f) {
        const double w = omega[f];
        acw_load<false>(N, LD, Gt, Ct, w, Ar, Ai, lane);
        for (int i = lane; i < N; i += 64) { Ar[i * LD + N] = Jr[i]; Ai[i * LD + N] = Ji[i]; }
        wave_sync();

        if (acw_solve(N, 1, LD, Ar, Ai, m.Lr, m.Li, Xr, Xi, eps2, lane)) flags |= CSIM_ST_LU_TINY_PIVOT;
        for (int p = lane; p < nProbe; p += 64) {
            const int eq = probe ? probe[p] : p;
            const size_t at = ac_out_at(f, p, nProbe, B, b);
            out[at] = Xr[eq];
            out[at + 1] = Xi[eq];
        }
        wave_sync();
    }
    if (lane == 0 && flags) status[b] |= flags;
}

// ---- 256-thread workgroup per system (N <= 1024): the planes in the instance's slice of a global scratch
__global__ void __launch_bounds__(ACB_THREADS) ac_sweep_block_kernel(int N, const double* __restrict__ sys,
                                                                     const double* __restrict__ omega, int F,
                                                                     const int32_t* __restrict__ probe, int nProbe, int B, int b0,
                                                                     double eps, double* __restrict__ out,
                                                                     uint32_t* __restrict__ status, double* work)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x;
    const int c = blockIdx.x, b = b0 + c;
    const int LD = acw_ld(N, 1);
    const AcbLds m = acb_carve(lds, N, 1);
    double* const Ar = acb_work_at(work, c, N, LD);
    double* const Ai = Ar + N * LD;
    const double* Gt = ac_system_at(sys, c, N);
    const double* Ct = Gt + N * N;
    const double* Jr = Ct + N * N;
    const double* Ji = Jr + N;
    const double eps2 = eps * eps;
    unsigned flags = 0u;

    for (int f = 0; f < F; ++f) {
        const double w = omega[f];
        acb_load<false>(N, LD, Gt, Ct, w, Ar, Ai, tid);
        for (int i = tid; i < N; i += ACB_THREADS) { Ar[i * LD + N] = Jr[i]; Ai[i * LD + N] = Ji[i]; }
        acb_sync();

        if (acb_solve(N, 1, LD, Ar, Ai, m.Lr, m.Li, m.rows, m.Xr, m.Xi, eps2, tid)) flags |= CSIM_ST_LU_TINY_PIVOT;
        for (int p = tid; p < nProbe; p += ACB_THREADS) {
            const int eq = probe ? probe[p] : p;
            const size_t at = ac_out_at(f, p, nProbe, B, b);
            out[at] = m.Xr[eq];
            out[at + 1] = m.Xi[eq];
        }
        __syncthreads();
    }
    if (tid == 0 && flags) status[b] |= flags;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32): acp_column / acp_back of ac_sweep.hpp, one RHS

template <int NP>
__global__ void __launch_bounds__(64) ac_sweep_packed_kernel(int N, const double* __restrict__ sys, const double* __restrict__ omega,
                                                             int F, const int32_t* __restrict__ probe, int nProbe, int B, int b0,
                                                             int Bc, double eps, double* __restrict__ out,
                                                             uint32_t* __restrict__ status)
{
    __shared__ double xs[2][2][ACP_LANES];                  // [instance][re, im][position]
    const AcpInstance t = acp_instance(b0, Bc);
    const int h = t.h, r = t.r, b = t.b;
    const bool on = t.on;
    const double* Gt = ac_system_at(sys, t.cc, N);
    const double* Ct = Gt + N * N;
    const double* Jr = Ct + N * N;
    const double* Ji = Jr + N;
    double* Xr = xs[h][0];
    double* Xi = xs[h][1];
    const double eps2 = eps * eps;
    unsigned flags = 0u;

    for (int f = 0; f < F; ++f) {
        const double w = omega[f];
        double ar[NP + 1], ai[NP + 1];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const bool in = r < N && j < N;
            ar[j] = in ? Gt[j * N + r] : 0.0;
            ai[j] = in ? w * Ct[j * N + r] : 0.0;
        }
        ar[NP] = r < N ? Jr[r] : 0.0;
        ai[NP] = r < N ? Ji[r] : 0.0;
        int pos = r;
        bool failed = false;
        acp_column<NP, 1, 0>(ar, ai, N, pos, failed, eps2, h);
        acp_back<NP, 1, NP - 1>(ar, ai, N, pos, Xr, Xi);
        if (failed) flags |= CSIM_ST_LU_TINY_PIVOT;
        for (int p = r; p < nProbe; p += ACP_LANES) {
            const int eq = probe ? probe[p] : p;
            if (on) {
                const size_t at = ac_out_at(f, p, nProbe, B, b);
                out[at] = failed ? 0.0 : Xr[eq];
                out[at + 1] = failed ? 0.0 : Xi[eq];
            }
        }
        __syncthreads();
    }
    if (on && r == 0 && flags) status[b] |= flags;
}

} // namespace

size_t acSystemDoubles(int N) { return (size_t)2 * N * N + (size_t)2 * N; }
size_t acBlockWorkDoubles(int N) { return (size_t)2 * N * (size_t)acw_ld(N, 1); }

hipError_t launchAcAssemble(const GenPlan& pl, const double* dAcRe, const double* dAcIm, const double* dParams, int B,
                            int b0, int Bc, const double* dXop, double* dSys, hipStream_t stream, int which)
{
    if (Bc <= 0) return hipSuccess;
    if (which == AC_KERNEL_BLOCK) {
        const size_t lds = sizeof(double) * ((size_t)pl.nTerms + pl.P + pl.N);
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute((const void*)ac_assemble_big_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(ac_assemble_big_kernel, dim3(Bc), dim3(64), lds, stream, pl, dAcRe, dAcIm, dParams, B, b0, dXop, dSys);
        return hipGetLastError();
    }
    const size_t lds = sizeof(double) * ((size_t)pl.nTerms + pl.P + pl.N + (size_t)pl.N * pl.LD);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)ac_assemble_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(ac_assemble_kernel, dim3(Bc), dim3(64), lds, stream, pl, dAcRe, dAcIm, dParams, B, b0, dXop, dSys);
    return hipGetLastError();
}

hipError_t launchAcSweep(int which, const AcArgs& a, hipStream_t stream)
{
    if (a.Bc <= 0 || a.F <= 0) return hipSuccess;
    if (!ac_sweep_covers(which, a.N)) return hipErrorInvalidValue;
    if (which == AC_KERNEL_BLOCK) {
        if (!a.work) return hipErrorInvalidValue;
        hipLaunchKernelGGL(ac_sweep_block_kernel, dim3(a.Bc), dim3(ACB_THREADS), acb_lds_bytes(a.N, 1), stream, a.N, a.sys, a.omega,
                           a.F, a.probe, a.nProbe, a.B, a.b0, a.eps, a.out, a.status, a.work);
    } else if (which == AC_KERNEL_PACKED) {
        acp_dispatch(a.N, [&](auto np) {
            hipLaunchKernelGGL(ac_sweep_packed_kernel<decltype(np)::value>, dim3((a.Bc + 1) / 2), dim3(64), 0, stream, a.N, a.sys,
                               a.omega, a.F, a.probe, a.nProbe, a.B, a.b0, a.Bc, a.eps, a.out, a.status);
        });
    } else {
        const size_t lds = acw_lds_bytes(a.N, 1);
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute((const void*)ac_sweep_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(ac_sweep_wave_kernel, dim3(a.Bc), dim3(64), lds, stream, a.N, a.sys, a.omega, a.F, a.probe, a.nProbe,
                           a.B, a.b0, a.eps, a.out, a.status);
    }
    return hipGetLastError();
}

} // namespace csim
