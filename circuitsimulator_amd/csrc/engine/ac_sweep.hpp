// ac_sweep.hpp -- what the sweep kernels of the AC, noise, S-parameter, two-port noise, distortion, intermodulation and
// loop-gain analyses (kernels_ac.hip, kernels_noise.hip, kernels_sp.hip, kernels_spnoise.hip, kernels_disto.hip,
// kernels_imd.hip, kernels_stb.hip) share: the
// factorisation and back substitution with K right-hand sides -- ac_lu.hpp's primitives applied in the order of
// ac_lu_solve_multi(), by one wavefront on a system in LDS, or by 32 lanes on a system in registers -- and the
// scaffolding around it (LDS carve-up, the G + jwC load, instance indexing, launch dispatch).  AC, noise, distortion
// and intermodulation are K = 1, loop gain is K = 2.  Included by those seven files only (by the distortion and
// intermodulation ones through ac_chain.hpp, which holds their two kernel bodies).
// A third shape, one 256-thread workgroup per system for N <= 1024 (AC and noise only), is ac_block.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "ac_block.hpp"
#include "ac_lu.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

// ---- wave per system (N <= 63): the augmented matrix in LDS (re / im planes, row i at i * LD, right-hand side c in
// column N + c, LD >= N + K), pivot by max-reduction and ballot, rows swapped in LDS, elimination spread over the
// trailing sub-matrix.  The right-hand sides never take part in the pivot search.
// Lr, Li: 64 doubles each (multipliers of the current column, then products of the back substitution).
// Solution c goes to Xr/Xi[c * 64 + 0 .. N-1], zeros when the factorisation fails; returns whether it failed.
__device__ __forceinline__ bool acw_solve(int N, int K, int LD, double* Ar, double* Ai, double* Lr, double* Li, double* Xr,
                                          double* Xi, double eps2, int lane)
{
    bool failed = false;
    const int W = N + K;
    for (int k = 0; k < N; ++k) {
        const bool cand = lane >= k && lane < N;
        const double v = cand ? cpx_abs2({Ar[lane * LD + k], Ai[lane * LD + k]}) : -1.0;
        const double dv = read_lane(v, k);
        int piv = k;
        double maxv = dv;
        if (dv == dv) {                  // a NaN diagonal keeps the pivot
            maxv = wave_max(v);          // v_max_f64 drops NaN candidates, as "v > maxv" never takes them
            piv = __ffsll((long long)__ballot(cand && v == maxv)) - 1;
        }
        if (maxv < eps2) { failed = true; break; }
        if (piv != k) {
            for (int j = k + lane; j < W; j += 64) {
                double t = Ar[k * LD + j]; Ar[k * LD + j] = Ar[piv * LD + j]; Ar[piv * LD + j] = t;
                t = Ai[k * LD + j]; Ai[k * LD + j] = Ai[piv * LD + j]; Ai[piv * LD + j] = t;
            }
            wave_sync();
        }
        const cpx p = {Ar[k * LD + k], Ai[k * LD + k]};
        if (lane > k && lane < N) {
            const cpx l = cpx_div({Ar[lane * LD + k], Ai[lane * LD + k]}, p);
            Lr[lane] = l.re;
            Li[lane] = l.im;
        }
        wave_sync();
        const int cols = W - k - 1, total = (N - k - 1) * cols;
        for (int e = lane; e < total; e += 64) {
            const int di = e / cols;
            const int i = k + 1 + di, j = k + 1 + (e - di * cols);
            const cpx l = {Lr[i], Li[i]};
            if (cpx_is_zero(l)) continue;
            const cpx r = cpx_elim({Ar[i * LD + j], Ai[i * LD + j]}, l, {Ar[k * LD + j], Ai[k * LD + j]});
            Ar[i * LD + j] = r.re;
            Ai[i * LD + j] = r.im;
        }
        wave_sync();
    }

    if (failed) {
        for (int c = 0; c < K; ++c)
            if (lane < N) { Xr[c * 64 + lane] = 0.0; Xi[c * 64 + lane] = 0.0; }
    } else {
        for (int c = 0; c < K; ++c) {
            double* xr = Xr + c * 64;
            double* xi = Xi + c * 64;
            for (int i = N - 1; i >= 0; --i) {
                if (lane > i && lane < N) {              // products U(i,j) x(j), then their ordered sum
                    const cpx pr = cpx_mul({Ar[i * LD + lane], Ai[i * LD + lane]}, {xr[lane], xi[lane]});
                    Lr[lane] = pr.re;
                    Li[lane] = pr.im;
                }
                wave_sync();
                cpx s = {Ar[i * LD + N + c], Ai[i * LD + N + c]};
                for (int j = i + 1; j < N; ++j) s = cpx_sub(s, {Lr[j], Li[j]});
                const cpx xv = cpx_div(s, {Ar[i * LD + i], Ai[i * LD + i]});
                wave_sync();
                if (lane == 0) { xr[i] = xv.re; xi[i] = xv.im; }
                wave_sync();
            }
        }
    }
    wave_sync();
    return failed;
}

// the system of chunk instance c as ac_assemble_kernel leaves it: G, C column-major [N][N], then J re, J im
__device__ __forceinline__ const double* ac_system_at(const double* sys, int c, int N)
{
    return sys + (size_t)c * (2 * N * N + 2 * N);
}

// the wave kernels' dynamic LDS: the two planes, Lr / Li, then K solutions of 64 doubles per part
__host__ __device__ inline int acw_ld(int N, int K) { return (N + K) | 1; }     // odd, >= N + K; K = 1: plan.hpp ldFor()
inline size_t acw_lds_bytes(int N, int K)
{
    return sizeof(double) * (2 * (size_t)N * (size_t)acw_ld(N, K) + 2 * 64 + 2 * (size_t)K * 64);
}
struct AcwLds { double *Ar, *Ai, *Lr, *Li, *Xr, *Xi; };
__device__ __forceinline__ AcwLds acw_carve(double* lds, int N, int K, int LD)
{
    AcwLds m;
    m.Ar = lds;
    m.Ai = m.Ar + N * LD;
    m.Lr = m.Ai + N * LD;
    m.Li = m.Lr + 64;
    m.Xr = m.Li + 64;
    m.Xi = m.Xr + K * 64;
    return m;
}

// A = G + jwC into the LDS planes, or A^T (word q * N + m of a column-major plane is A(m,q) = A^T(q,m)): the lanes
// walk the words in address order.  The caller fills the right-hand sides and synchronises.
template <bool TRANSPOSED>
__device__ __forceinline__ void acw_load(int N, int LD, const double* Gt, const double* Ct, double w, double* Ar, double* Ai,
                                         int lane)
{
    for (int idx = lane; idx < N * N; idx += 64) {
        const int q = idx / N, m = idx - q * N;
        const int i = TRANSPOSED ? q : m, j = TRANSPOSED ? m : q;
        Ar[i * LD + j] = Gt[idx];
        Ai[i * LD + j] = w * Ct[idx];
    }
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32), two systems per wavefront
constexpr int ACP_LANES = 32;

// half h of the wavefront, lane r of it, chunk instance c; the second half of the last block may be empty (on false):
// it computes on instance cc = 0 and stores nothing
struct AcpInstance { int h, r, cc, b; bool on; };
__device__ __forceinline__ AcpInstance acp_instance(int b0, int Bc)
{
    AcpInstance t;
    t.h = threadIdx.x / ACP_LANES;
    t.r = threadIdx.x % ACP_LANES;
    const int c = blockIdx.x * 2 + t.h;
    t.on = c < Bc;
    t.cc = t.on ? c : 0;
    t.b = b0 + t.cc;
    return t;
}

__device__ __forceinline__ unsigned half_ballot(bool pred, int h)
{
    return (unsigned)((__ballot(pred) >> (h * ACP_LANES)) & 0xFFFFFFFFull);
}
__device__ __forceinline__ double half_max(double v)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, ACP_LANES));
    return v;
}
__device__ __forceinline__ int half_min(int v)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, ACP_LANES));
    return v;
}

// column K of the elimination: pivot search over the positions K..N-1, logical exchange of positions K and
// the pivot's, pivot row to every lane, rows below apply their multiplier.  Lane r holds one row: column j in
// register j, right-hand side c in register NP + c (KP of them).
template <int NP, int KP, int K>
__device__ __forceinline__ void acp_column(double (&ar)[NP + KP], double (&ai)[NP + KP], int N, int& pos, bool& failed,
                                           double eps2, int h)
{
    if constexpr (K < NP) {
        if (K < N) {
            const bool cand = pos >= K && pos < N;
            const double v = cand ? cpx_abs2({ar[K], ai[K]}) : -1.0;
            const int dl = __ffs((int)half_ballot(pos == K, h)) - 1;
            const double dv = __shfl(v, dl, ACP_LANES);
            const double m = half_max(v);
            const int first = half_min((cand && v == m) ? pos : 1 << 20);
            const bool nanDiag = dv != dv;                   // a NaN diagonal keeps the pivot
            const int pivPos = nanDiag ? K : first;
            const double maxv = nanDiag ? dv : m;
            if (maxv < eps2) failed = true;
            const int pl = __ffs((int)half_ballot(pos == pivPos, h)) - 1;
            if (pos == pivPos) pos = K;
            else if (pos == K) pos = pivPos;
            const cpx p = {__shfl(ar[K], pl, ACP_LANES), __shfl(ai[K], pl, ACP_LANES)};
            cpx l = {0.0, 0.0};
            if (pos > K && pos < N) l = cpx_div({ar[K], ai[K]}, p);
            const bool upd = !cpx_is_zero(l);
#pragma unroll
            for (int j = K + 1; j < NP + KP; ++j) {
                const cpx u = {__shfl(ar[j], pl, ACP_LANES), __shfl(ai[j], pl, ACP_LANES)};
                if (upd) {
                    const cpx r = cpx_elim({ar[j], ai[j]}, l, u);
                    ar[j] = r.re;
                    ai[j] = r.im;
                }
            }
        }
        acp_column<NP, KP, K + 1>(ar, ai, N, pos, failed, eps2, h);
    }
}

// row I of the back substitution of all KP columns (independent of each other): every lane sums on its own row, the
// lane holding position I stores x(I) of solution c at X[c * ACP_LANES + I]
template <int NP, int KP, int I>
__device__ __forceinline__ void acp_back(const double (&ar)[NP + KP], const double (&ai)[NP + KP], int N, int pos,
                                         double* Xr, double* Xi)
{
    if constexpr (I >= 0) {
        if (I < N) {
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                cpx s = {ar[NP + c], ai[NP + c]};
#pragma unroll
                for (int j = I + 1; j < NP; ++j)
                    if (j < N) s = cpx_sub(s, cpx_mul({ar[j], ai[j]}, {Xr[c * ACP_LANES + j], Xi[c * ACP_LANES + j]}));
                const cpx xv = cpx_div(s, {ar[I], ai[I]});
                if (pos == I) { Xr[c * ACP_LANES + I] = xv.re; Xi[c * ACP_LANES + I] = xv.im; }
            }
            __syncthreads();
        }
        acp_back<NP, KP, I - 1>(ar, ai, N, pos, Xr, Xi);
    }
}

// ---- launch: the sizes the kernel shapes cover, and the packed kernel's NP = N rounded up to 8
inline bool ac_sweep_covers(int which, int N)
{
    if (which == AC_KERNEL_BLOCK) return N >= 1 && N <= ACB_MAX_N;
    return N >= 1 && N <= 63 && !(which == AC_KERNEL_PACKED && N > 32);
}

// A = G + jwC (or A^T) into the block shape's planes, the workgroup walking the words in address order
template <bool TRANSPOSED>
__device__ __forceinline__ void acb_load(int N, int LD, const double* Gt, const double* Ct, double w, double* Ar, double* Ai,
                                         int tid)
{
    for (int idx = tid; idx < N * N; idx += ACB_THREADS) {
        const int q = idx / N, m = idx - q * N;
        const int i = TRANSPOSED ? q : m, j = TRANSPOSED ? m : q;
        Ar[i * LD + j] = Gt[idx];
        Ai[i * LD + j] = w * Ct[idx];
    }
}

// the planes of chunk instance c in the block shape's scratch: acBlockWorkDoubles(N) doubles per instance
__device__ __forceinline__ double* acb_work_at(double* work, int c, int N, int LD) { return work + (size_t)c * 2 * N * LD; }

// launch(std::integral_constant<int, NP>)
template <class Launch>
inline void acp_dispatch(int N, Launch&& launch)
{
    if (N <= 8) launch(std::integral_constant<int, 8>{});
    else if (N <= 16) launch(std::integral_constant<int, 16>{});
    else if (N <= 24) launch(std::integral_constant<int, 24>{});
    else launch(std::integral_constant<int, 32>{});
}

} // namespace

} // namespace csim
