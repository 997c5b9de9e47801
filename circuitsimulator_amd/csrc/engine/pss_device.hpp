// pss_device.hpp -- the one home of what the period kernels of the periodic steady state (kernels_pss.hip), the
// periodic AC analysis (kernels_pac.hip) and the periodic noise analysis (kernels_pnoise.hip) have in common: the
// per-instance prologue (period_load), the start decision of the analyses that follow a W_K launch
// (period_start_status), Hm = d(right-hand side)/d(x_prev) (period_hm, from pss_rhs and pss_terms_history), the
// backward-Euler step with its Newton loop (period_newton_step) and the sparse-row product with Hm
// (period_hm_product).  Every kernel that integrates the orbit calls period_newton_step, so the orbit is one piece of
// code and the same bits in all of them.
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "pac.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

// the right-hand side alone, as assemble() forms it: out[0 .. N-1]
__device__ __forceinline__ void pss_rhs(const GenPlan& pl, const double* T, double* out, int lane)
{
    if (lane < pl.N) out[lane] = 0.0;
    wave_sync();
    for (int n = lane; n < pl.nnzI; n += 64) {
        double acc = 0.0;
        for (int c = pl.iPtr[n]; c < pl.iPtr[n + 1]; ++c) {
            const int con = pl.iCon[c];
            const double v = T[con >> 1];
            acc = (con & 1) ? acc - v : acc + v;
        }
        out[pl.iRow[n]] = acc;
    }
    wave_sync();
}

// the history terms at xp with every source at zero
__device__ __forceinline__ void pss_terms_history(const GenPlan& pl, const double* Pv, double* T, const double* xp, int lane)
{
    terms_step_tran(pl, Pv, T, xp, 0.0, lane);
    wave_sync();
    for (int e = lane; e < pl.nElem; e += 64) {
        const int kind = pl.kind[e];
        if (kind == CSIM_V || kind == CSIM_I) T[pl.termBase[e] + T_SRC_VAL] = 0.0;
    }
    wave_sync();
}

// The parameters of instance b, the terms at zero, the state vectors at the lane's start values xs0 and xp0 (where the
// four kernels differ), the launch's constant terms and the transient gmin.  The state vectors are written here, after
// the parameter loads, and not by the caller before the call: with the stores first k_pnoise_period came out with
// 55 more scalar-spill reloads and ran 0.5 % slower.
__device__ __forceinline__ void period_load(const GenPlan& pl, const double* params, int B, int b, double dt, double* Pv,
                                            double* T, double* xs, double xs0, double* xp, double xp0, int lane)
{
    for (int p = lane; p < pl.P; p += 64) Pv[p] = params[(int64_t)p * B + b];
    for (int t = lane; t < pl.nTerms; t += 64) T[t] = 0.0;
    if (lane < pl.N) { xs[lane] = xs0; xp[lane] = xp0; }
    wave_sync();
    terms_const<true>(pl, Pv, T, dt, lane);
    if (lane == 0) T[pl.termGmin] = pl.k.tran_gmin;
    wave_sync();
}

// An instance stops before it starts: a start vector, an earlier analysis (status word in) or the W_K launch (status
// word ws) that was not finite or singular.  Adds what the instance inherits to st; true = stop.
__device__ __forceinline__ bool period_start_status(unsigned in, unsigned ws, double xin, int N, int lane, unsigned& st)
{
    st |= ws & (CSIM_ST_TRAN_NONFINITE | CSIM_ST_TRAN_NONCONV | CSIM_ST_LU_TINY_PIVOT | CSIM_ST_LU_ZERO_DIAG);
    if (ws & CSIM_ST_PSS_SINGULAR) st |= CSIM_ST_PAC_SINGULAR;
    if (!wave_all_finite(xin, N, lane)) st |= CSIM_ST_TRAN_NONFINITE;
    return ((in | st) & CSIM_ST_TRAN_NONFINITE) || (in & CSIM_ST_PSS_SINGULAR) || (st & CSIM_ST_PAC_SINGULAR);
}

// Hm = d(right-hand side)/d(x_prev): the history currents are linear and source-free in xp, and no MOS term has been
// written yet, so column l is rhs(e_l) - rhs(0) with both exact.  Entry (i, l) goes to Hm[i * rowStride + l * colStride]:
// (N, 1) stores Hm row-major, (1, N) its transpose.  xp comes in all zero and leaves all zero.
__device__ __forceinline__ void period_hm(const GenPlan& pl, const double* Pv, double* T, double* xp, double* sc, double* Hm,
                                          int rowStride, int colStride, int lane)
{
    const int N = pl.N;
    pss_terms_history(pl, Pv, T, xp, lane);
    pss_rhs(pl, T, sc, lane);
    const double base = (lane < N) ? sc[lane] : 0.0;
    for (int l = 0; l < N; ++l) {
        if (lane == l) xp[l] = 1.0;
        wave_sync();
        pss_terms_history(pl, Pv, T, xp, lane);
        pss_rhs(pl, T, sc, lane);
        if (lane < N) Hm[lane * rowStride + l * colStride] = sc[lane] - base;
        if (lane == l) xp[l] = 0.0;
        wave_sync();
    }
}

// Backward-Euler step s from xp: k_tran_general's body without its logs, counts and hand-backs -- the same device
// functions in the same order, so the trajectory is that kernel's bit for bit.  Leaves the converged iterate in xs and
// in xp.  A solve that is not finite sets CSIM_ST_TRAN_NONFINITE and returns false: the instance stops.
__device__ __forceinline__ bool period_newton_step(const GenPlan& pl, const double* Pv, double* T, double* Gm, double* xs,
                                                   double* xp, double* sc, long long s, double dt, int lane, unsigned& st)
{
    const int N = pl.N;
    const csim_consts& K = pl.k;
    terms_step_tran(pl, Pv, T, xp, tran_time(s, dt), lane);
    wave_sync();
    for (int iter = 0; iter < K.tran_max_iters; ++iter) {
        terms_iter_mos(pl, Pv, T, xs, lane);
        wave_sync();
        assemble(pl, T, Gm, lane);
        const double xr = lu_solve_wave(Gm, N, pl.LD, K.lu_eps, lane, st);
        if (!wave_all_finite(xr, N, lane)) {
            st |= CSIM_ST_TRAN_NONFINITE;
            return false;
        }
        const double xo = (lane < N) ? xs[lane] : 0.0;
        const double xn = xo + K.tran_alpha * (xr - xo);
        const double err = norm_in_order(xn - xo, sc, N, lane);
        if (lane < N) xs[lane] = xn;
        wave_sync();
        if (err < K.tran_tol) break;
        if (iter == K.tran_max_iters - 1) st |= CSIM_ST_TRAN_NONCONV;
    }
    if (lane < N) xp[lane] = xs[lane];
    wave_sync();
    return true;
}

// dst(i, :) = sum over the non-zero H(i, l), l ascending, of H(i, l) src(l, :) for the N rows of H (N x N, row-major):
// lane j owns column j of the `width` columns, product and sum rounded separately (pac_hm_add)
__device__ __forceinline__ void period_hm_product(const double* H, int N, const double* src, int srcStride, double* dst,
                                                  int dstStride, int width, int lane)
{
    for (int i = 0; i < N; ++i) {
        const double hv = (lane < N) ? H[i * N + lane] : 0.0;
        unsigned long long todo = __ballot(hv != 0.0);
        double acc = 0.0;
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const double h = read_lane(hv, l);
            if (lane < width) acc = pac_hm_add(acc, h, src[l * srcStride + lane]);
        }
        if (lane < width) dst[i * dstStride + lane] = acc;
    }
    wave_sync();
}

} // namespace

} // namespace csim
