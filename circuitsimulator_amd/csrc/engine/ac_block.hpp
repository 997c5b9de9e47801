// ac_block.hpp -- the third shape of the complex solve of ac_sweep.hpp: one 256-thread workgroup per system, for
// 1 <= N <= 1024.  The wave shape ties a row to a lane and the packed shape keeps a row in registers, so both end at
// 63 unknowns; here rows and columns are spread over the workgroup and nothing but the N-long vectors lives in LDS.
// ac_lu.hpp's primitives are applied to every entry in the order of ac_lu_solve_multi(): the result is bit-identical
// to the host statement and to the other two shapes.  Included by ac_sweep.hpp only.
#pragma once

#include <hip/hip_runtime.h>

#include "ac_lu.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

constexpr int ACB_THREADS = 256;
constexpr int ACB_MAX_N = 1024;

// the block kernels' dynamic LDS: Lr / Li (N each), K solutions of N doubles per part, the compacted row list (N ints)
inline size_t acb_lds_bytes(int N, int K)
{
    return sizeof(double) * (2 * (size_t)N + 2 * (size_t)K * (size_t)N) + sizeof(int32_t) * (size_t)N;
}
struct AcbLds { double *Lr, *Li, *Xr, *Xi; int32_t* rows; };
__device__ __forceinline__ AcbLds acb_carve(double* lds, int N, int K)
{
    AcbLds m;
    m.Lr = lds;
    m.Li = m.Lr + N;
    m.Xr = m.Li + N;
    m.Xi = m.Xr + K * N;
    m.rows = reinterpret_cast<int32_t*>(m.Xi + K * N);
    return m;
}

// a phase that wrote the planes (they may live in global memory) before one that reads them
__device__ __forceinline__ void acb_sync()
{
    __threadfence_block();
    __syncthreads();
}

// The augmented matrix as re / im planes behind plain pointers (global scratch or LDS), row i at i * LD, right-hand
// side c in column N + c, LD >= N + K.  Rows are swapped physically.  Lr, Li: N doubles each (multipliers of the
// current column, then products of the back substitution); rows: N ints (the rows of the column whose multiplier is
// not zero).  Solution c goes to Xr/Xi[c * N + 0 .. N-1], zeros when the factorisation fails; returns whether it
// failed (the same answer in every thread).  The caller has synchronised after filling the planes.
__device__ __forceinline__ bool acb_solve(int N, int K, int LD, double* Ar, double* Ai, double* Lr, double* Li, int32_t* rows,
                                          double* Xr, double* Xi, double eps2, int tid)
{
    __shared__ double redV[ACB_THREADS / 64];
    __shared__ int redI[ACB_THREADS / 64];
    __shared__ int nRows;
    const int lane = tid & 63, wave = tid >> 6;
    const int W = N + K;
    bool failed = false;

    for (int k = 0; k < N; ++k) {
        // ---- pivot: every thread keeps (max, first index) of its rows, walked ascending with a strict '>' (a NaN is
        // never taken); the reduction prefers the larger value, then the smaller index
        double bv = -1.0;
        int bi = 0x7fffffff;
        for (int i = k + tid; i < N; i += ACB_THREADS) {
            const double v = cpx_abs2({Ar[i * LD + k], Ai[i * LD + k]});
            if (v > bv) { bv = v; bi = i; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(bv, m);
            const int oi = __shfl_xor(bi, m);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { redV[wave] = bv; redI[wave] = bi; }
        if (tid == 0) nRows = 0;
        __syncthreads();
        // the decision, from LDS and the diagonal alone: the same in every thread (barriers follow it)
        const double dv = cpx_abs2({Ar[k * LD + k], Ai[k * LD + k]});
        double maxv = dv;
        int piv = k;
        if (dv == dv) {                                     // a NaN diagonal keeps the pivot
            maxv = redV[0];
            piv = redI[0];
#pragma unroll
            for (int w = 1; w < ACB_THREADS / 64; ++w)
                if (redV[w] > maxv || (redV[w] == maxv && redI[w] < piv)) { maxv = redV[w]; piv = redI[w]; }
        }
        if (maxv < eps2) { failed = true; break; }
        if (piv != k) {
            for (int j = k + tid; j < W; j += ACB_THREADS) {
                double t = Ar[k * LD + j]; Ar[k * LD + j] = Ar[piv * LD + j]; Ar[piv * LD + j] = t;
                t = Ai[k * LD + j]; Ai[k * LD + j] = Ai[piv * LD + j]; Ai[piv * LD + j] = t;
            }
            acb_sync();
        }
        // ---- multipliers, and the list of rows that have one: MNA columns hold a handful
        const cpx p = {Ar[k * LD + k], Ai[k * LD + k]};
        for (int i = k + 1 + tid; i < N; i += ACB_THREADS) {
            const cpx l = cpx_div({Ar[i * LD + k], Ai[i * LD + k]}, p);
            if (cpx_is_zero(l)) continue;
            Lr[i] = l.re;
            Li[i] = l.im;
            rows[atomicAdd(&nRows, 1)] = i;                 // any order: the updates of two entries are independent
        }
        __syncthreads();
        // ---- elimination over (those rows) x (every trailing column, zeros of the pivot row included: a - l * 0
        // may change the sign of a zero)
        const int cols = W - k - 1, total = nRows * cols;
        for (int e = tid; e < total; e += ACB_THREADS) {
            const int r = e / cols;
            const int i = rows[r], j = k + 1 + (e - r * cols);
            const cpx v = cpx_elim({Ar[i * LD + j], Ai[i * LD + j]}, {Lr[i], Li[i]}, {Ar[k * LD + j], Ai[k * LD + j]});
            Ar[i * LD + j] = v.re;
            Ai[i * LD + j] = v.im;
        }
        acb_sync();
    }

    if (failed) {
        for (int e = tid; e < K * N; e += ACB_THREADS) { Xr[e] = 0.0; Xi[e] = 0.0; }
    } else {
        for (int c = 0; c < K; ++c) {
            double* xr = Xr + c * N;
            double* xi = Xi + c * N;
            for (int i = N - 1; i >= 0; --i) {
                for (int j = i + 1 + tid; j < N; j += ACB_THREADS) {     // products U(i,j) x(j), then their ordered sum
                    const cpx pr = cpx_mul({Ar[i * LD + j], Ai[i * LD + j]}, {xr[j], xi[j]});
                    Lr[j] = pr.re;
                    Li[j] = pr.im;
                }
                __syncthreads();
                if (tid == 0) {
                    cpx s = {Ar[i * LD + N + c], Ai[i * LD + N + c]};
                    int j = i + 1;
                    for (; j + 4 <= N; j += 4) {                         // four loads in flight, one chain
                        const cpx p0 = {Lr[j], Li[j]}, p1 = {Lr[j + 1], Li[j + 1]}, p2 = {Lr[j + 2], Li[j + 2]},
                                  p3 = {Lr[j + 3], Li[j + 3]};
                        s = cpx_sub(cpx_sub(cpx_sub(cpx_sub(s, p0), p1), p2), p3);
                    }
                    for (; j < N; ++j) s = cpx_sub(s, {Lr[j], Li[j]});
                    const cpx xv = cpx_div(s, {Ar[i * LD + i], Ai[i * LD + i]});
                    xr[i] = xv.re;
                    xi[i] = xv.im;
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    return failed;
}

} // namespace

} // namespace csim
