// ac_sweep.hpp -- the factorisation and back substitution shared by the sweep kernels of the AC analysis
// (kernels_ac.hip) and of the noise analysis (kernels_noise.hip): ac_lu.hpp's primitives applied in its order,
// by one wavefront on a system in LDS, or by 32 lanes on a system in registers.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "ac_lu.hpp"
#include "device_common.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

// ---- wave per system (N <= 63): the augmented matrix in LDS (re / im planes, row i at i * LD, RHS in column N),
// pivot by max-reduction and ballot, rows swapped in LDS, elimination spread over the trailing sub-matrix.
// Lr, Li: 64 doubles each (multipliers of the current column, then products of the back substitution).
// X gets the solution, or zeros when the factorisation fails; returns whether it failed.
// Twin: acw_solve_multi() below repeats the pivot search, exchange and elimination over N + K columns -- a change to
// either belongs in both (bitwise guards: tests/test_ac_kernels_gpu.py here, tests/test_sp_kernels_gpu.py there, and
// K = 1 of the one against the other).
__device__ __forceinline__ bool acw_solve(int N, int LD, double* Ar, double* Ai, double* Lr, double* Li, double* Xr,
                                          double* Xi, double eps2, int lane)
{
    bool failed = false;
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
            for (int j = k + lane; j <= N; j += 64) {
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
        const int cols = N - k, total = (N - k - 1) * cols;
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
        if (lane < N) { Xr[lane] = 0.0; Xi[lane] = 0.0; }
    } else {
        for (int i = N - 1; i >= 0; --i) {
            if (lane > i && lane < N) {              // products U(i,j) x(j), then their ordered sum
                const cpx pr = cpx_mul({Ar[i * LD + lane], Ai[i * LD + lane]}, {Xr[lane], Xi[lane]});
                Lr[lane] = pr.re;
                Li[lane] = pr.im;
            }
            wave_sync();
            cpx s = {Ar[i * LD + N], Ai[i * LD + N]};
            for (int j = i + 1; j < N; ++j) s = cpx_sub(s, {Lr[j], Li[j]});
            const cpx xv = cpx_div(s, {Ar[i * LD + i], Ai[i * LD + i]});
            wave_sync();
            if (lane == 0) { Xr[i] = xv.re; Xi[i] = xv.im; }
            wave_sync();
        }
    }
    wave_sync();
    return failed;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32)
constexpr int ACP_LANES = 32;

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
// the pivot's, pivot row to every lane, rows below apply their multiplier.
// Twins: acp_column_multi / acp_back_multi below (KP right-hand-side registers) -- a change to either belongs in both.
template <int NP, int K>
__device__ __forceinline__ void acp_column(double (&ar)[NP + 1], double (&ai)[NP + 1], int N, int& pos, bool& failed,
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
            for (int j = K + 1; j <= NP; ++j) {
                const cpx u = {__shfl(ar[j], pl, ACP_LANES), __shfl(ai[j], pl, ACP_LANES)};
                if (upd) {
                    const cpx r = cpx_elim({ar[j], ai[j]}, l, u);
                    ar[j] = r.re;
                    ai[j] = r.im;
                }
            }
        }
        acp_column<NP, K + 1>(ar, ai, N, pos, failed, eps2, h);
    }
}

// row I of the back substitution: every lane sums on its own row, the lane holding position I stores x(I)
template <int NP, int I>
__device__ __forceinline__ void acp_back(const double (&ar)[NP + 1], const double (&ai)[NP + 1], int N, int pos,
                                         double* Xr, double* Xi)
{
    if constexpr (I >= 0) {
        if (I < N) {
            cpx s = {ar[NP], ai[NP]};
#pragma unroll
            for (int j = I + 1; j < NP; ++j)
                if (j < N) s = cpx_sub(s, cpx_mul({ar[j], ai[j]}, {Xr[j], Xi[j]}));
            const cpx xv = cpx_div(s, {ar[I], ai[I]});
            if (pos == I) { Xr[I] = xv.re; Xi[I] = xv.im; }
            __syncthreads();
        }
        acp_back<NP, I - 1>(ar, ai, N, pos, Xr, Xi);
    }
}

// ---- the same two solves carried to K right-hand sides (ac_port.hpp ac_lu_solve_multi): columns N .. N+K-1 of the
// wave kernel's LDS matrix, registers NP .. NP+KP-1 of the packed kernel's rows.  Every entry gets the operations
// of the single-RHS solve in its order; the right-hand sides never take part in the pivot search.

// X: solution c at Xr/Xi[c * 64 + 0 .. N-1], zeros when the factorisation fails; LD >= N + K
__device__ __forceinline__ bool acw_solve_multi(int N, int K, int LD, double* Ar, double* Ai, double* Lr, double* Li,
                                                double* Xr, double* Xi, double eps2, int lane)
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
            maxv = wave_max(v);
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

// acp_column with KP right-hand-side registers NP .. NP+KP-1
template <int NP, int KP, int K>
__device__ __forceinline__ void acp_column_multi(double (&ar)[NP + KP], double (&ai)[NP + KP], int N, int& pos,
                                                 bool& failed, double eps2, int h)
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
        acp_column_multi<NP, KP, K + 1>(ar, ai, N, pos, failed, eps2, h);
    }
}

// row I of the back substitution of all KP columns (independent of each other): solution c at X[c * ACP_LANES ...]
template <int NP, int KP, int I>
__device__ __forceinline__ void acp_back_multi(const double (&ar)[NP + KP], const double (&ai)[NP + KP], int N, int pos,
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
        acp_back_multi<NP, KP, I - 1>(ar, ai, N, pos, Xr, Xi);
    }
}

} // namespace

} // namespace csim
