// kernels_pac.hip -- periodic AC analysis: the backward-Euler transient linearised around a periodic orbit
// (include/csim.h "Periodic AC analysis", arithmetic in pac.hpp, budget and measurements in DESIGN.md 8i).
//
//   k_pac_period    one wavefront = one workgroup = one instance, N <= 63, Fc <= 32 frequencies.  K backward-Euler steps
//                   from x0, each one period_newton_step (pss_device.hpp), the step k_pss_period takes, so the orbit is
//                   that kernel's bit for bit; after every converged step Q = Hm P_{k-1}, P = z Q + u per frequency, J_k
//                   at the converged iterate, P <- J_k^-1 P.  The first launch starts at p_0 = 0 and leaves r_K; the
//                   second starts at the p_0 the close kernel solved for and adds the sideband sums, kept in LDS and
//                   stored once.
//   k_period_close  one wavefront per (instance, frequency): (I - z_K W_K) p_0 = r_K through acw_solve, the project's
//                   one complex LU.  The periodic noise analysis closes its adjoint recursion with the same kernel and
//                   W_K read transposed (PeriodCloseArgs::transposeW): one uniform branch where the matrix is filled.
//
// The P plane is N x 2 Fc real: frequency f has its real part in column 2 f and its imaginary part in column 2 f + 1, and
// lane j owns column j as lu_solve_multi_wave wants.  LDS of the period kernel: the general kernel's carve-up, Hm
// (N x N), P (N x 2 Fc), u (2 N), the sums (2 (2 M + 1) nProbe Fc); Q goes to the matrix area, dead between a step's
// last solve and the assembly of J_k, when its rows fit (2 Fc <= LD), else to a plane of its own.
#include <hip/hip_runtime.h>

#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"
#include "pac.hpp"
#include "pnoise.hpp"
#include "pss_device.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

struct PacLds { int Hm, Pm, ur, ui, Qm, sums, total; };      // offsets in doubles
__host__ __device__ inline PacLds pacLds(int N, int LD, int nTerms, int P, int Fc, int M, int nProbe)
{
    const int R = 2 * Fc;
    PacLds l;
    l.Hm = ldsLayout(N, LD, nTerms, P).total;
    l.Pm = l.Hm + N * N;
    l.ur = l.Pm + N * R;
    l.ui = l.ur + N;
    const int own = l.ui + N;
    l.Qm = R <= LD ? 0 : own;                               // 0: the matrix area
    l.sums = R <= LD ? own : own + N * R;
    l.total = l.sums + 2 * (2 * M + 1) * nProbe * Fc;
    return l;
}

// word of sideband sum idx = (mi * nProbe + q) * Fc + f of instance b in out [F][2 M + 1][nProbe][B] complex
__device__ __forceinline__ size_t pac_out_at(const PacArgs& a, int idx, int b)
{
    const int per = a.nProbe * a.Fc;
    const int mi = idx / per, rem = idx - mi * per;
    const int q = rem / a.Fc, f = rem - q * a.Fc;
    return 2 * ((((size_t)(a.fFirst + f) * (size_t)(2 * a.M + 1) + (size_t)mi) * (size_t)a.nProbe + (size_t)q) * (size_t)a.B + (size_t)b);
}

__device__ __forceinline__ void pac_set_sources(const GenPlan& pl, double* T, const double* src, int lane)
{
    for (int e = lane; e < pl.nElem; e += 64) {
        const int kind = pl.kind[e];
        if (kind == CSIM_V || kind == CSIM_I) T[pl.termBase[e] + T_SRC_VAL] = src[e];
    }
    wave_sync();
}

} // namespace

__global__ void __launch_bounds__(64)
k_pac_period(GenPlan pl, PacArgs a)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, b = a.b0 + c, B = a.B;
    const int N = pl.N, LD = pl.LD, R = 2 * a.Fc;
    const LdsLayout L = ldsLayout(N, LD, pl.nTerms, pl.P);
    const PacLds PL = pacLds(N, LD, pl.nTerms, pl.P, a.Fc, a.M, a.nProbe);
    double* Gm = sm + L.G;
    double* T = sm + L.T;
    double* Pv = sm + L.P;
    double* xs = sm + L.xs;
    double* xp = sm + L.xp;
    double* sc = sm + L.sc;
    double* Hm = sm + PL.Hm;
    double* Pm = sm + PL.Pm;
    double* ur = sm + PL.ur;
    double* ui = sm + PL.ui;
    double* Qm = sm + PL.Qm;
    const int nAcc = (2 * a.M + 1) * a.nProbe * a.Fc;
    double* sre = sm + PL.sums;
    double* sim = sre + nAcc;
    const csim_consts& K = pl.k;
    const bool second = a.out != nullptr;

    auto zeros_out = [&]() {
        for (int idx = lane; idx < nAcc; idx += 64) {
            const size_t at = pac_out_at(a, idx, b);
            a.out[at] = 0.0;
            a.out[at + 1] = 0.0;
        }
    };

    // an instance stops before it starts: a start vector, an earlier analysis or the W_K launch that was not finite or
    // singular.  The first launch decides and says so in stop[c]; the close kernel may add to it.
    unsigned st = 0;
    bool stop = a.stop[c] != 0;
    const double xin = (lane < N) ? a.x0[(int64_t)lane * B + b] : 0.0;
    if (!second) stop = period_start_status(a.status[b], a.wStatus[b], xin, N, lane, st);
    if (stop) {
        if (second) zeros_out();
        else if (lane == 0) { a.stop[c] = 1; a.status[b] |= st; }
        return;
    }

    period_load(pl, a.params, B, b, a.dt, Pv, T, xs, xin, xp, 0.0, lane);
    period_hm(pl, Pv, T, xp, sc, Hm, N, 1, lane);
    // u: the right-hand side with the AC excitation in the source slots and every history zero, as the AC analysis has it
    pss_terms_history(pl, Pv, T, xp, lane);
    pac_set_sources(pl, T, a.acRe, lane);
    pss_rhs(pl, T, sc, lane);
    if (lane < N) ur[lane] = sc[lane];
    wave_sync();
    pac_set_sources(pl, T, a.acIm, lane);
    pss_rhs(pl, T, sc, lane);
    if (lane < N) ui[lane] = sc[lane];
    wave_sync();

    const int fq = lane >> 1;                                           // this lane's frequency and part (lane < R)
    const bool imPart = (lane & 1) != 0;
    const double zr = (lane < R) ? a.zr[fq] : 0.0, zi = (lane < R) ? a.zi[fq] : 0.0;
    const double* p0 = a.p0 ? a.p0 + (size_t)c * (size_t)(N * R) : nullptr;
    for (int i = 0; i < N; ++i)
        if (lane < R) Pm[i * R + lane] = p0 ? p0[i * R + lane] : 0.0;
    for (int idx = lane; idx < nAcc; idx += 64) { sre[idx] = 0.0; sim[idx] = 0.0; }
    if (lane < N) xp[lane] = xin;                                       // histories come from the previous state
    wave_sync();

    bool aborted = false;
    for (long long s = 1; s <= a.K && !aborted; ++s) {
        // ---- the step, k_pss_period's
        if (!period_newton_step(pl, Pv, T, Gm, xs, xp, sc, s, a.dt, lane, st)) { aborted = true; break; }

        // ---- Q = Hm P_{k-1}, walking the non-zeros of Hm's row; P = z Q + u per frequency
        period_hm_product(Hm, N, Pm, R, Qm, R, R, lane);
        for (int i = 0; i < N; ++i)
            if (lane < R) {
                double re, im;
                pac_step_rhs(zr, zi, Qm[i * R + 2 * fq], Qm[i * R + 2 * fq + 1], ur[i], ui[i], &re, &im);
                Pm[i * R + lane] = imPart ? im : re;
            }
        wave_sync();

        // ---- J_k at the converged iterate, P <- J_k^-1 P
        terms_iter_mos(pl, Pv, T, xs, lane);
        wave_sync();
        assemble(pl, T, Gm, lane);
        if (!lu_solve_multi_wave(Gm, N, LD, Pm, R, R, K.lu_eps, lane)) {
            st |= CSIM_ST_PAC_SINGULAR | CSIM_ST_LU_TINY_PIVOT;
            aborted = true;
            break;
        }

        // ---- sideband sums (pac.hpp), k ascending; sum idx is always this lane's
        if (second)
            for (int idx = lane; idx < nAcc; idx += 64) {
                const int per = a.nProbe * a.Fc;
                const int mi = idx / per, rem = idx - mi * per;
                const int q = rem / a.Fc, f = rem - q * a.Fc;
                const int eq = a.probeEq ? a.probeEq[q] : q;
                const int j = pac_tw_index(mi - a.M, s, a.K);
                double re = sre[idx], im = sim[idx];
                pac_sum_add(Pm[eq * R + 2 * f], Pm[eq * R + 2 * f + 1], a.twc[j], a.tws[j], &re, &im);
                sre[idx] = re;
                sim[idx] = im;
            }
    }

    if (!second) {
        if (lane == 0) {
            a.status[b] |= st;
            if (aborted) a.stop[c] = 1;
        }
        if (!aborted) {
            double* pK = a.pK + (size_t)c * (size_t)(N * R);
            for (int i = 0; i < N; ++i)
                if (lane < R) pK[i * R + lane] = Pm[i * R + lane];
        }
        return;
    }
    if (aborted) { zeros_out(); return; }
    for (int idx = lane; idx < nAcc; idx += 64) {
        double re = sre[idx], im = sim[idx];
        pac_sum_finish(a.K, &re, &im);
        const size_t at = pac_out_at(a, idx, b);
        a.out[at] = re;
        a.out[at + 1] = im;
    }
}

// the closure of both analyses that carry a recursion round the orbit: v <- (I - z_K W_K)^-1 v, or with W_K^T
__global__ void __launch_bounds__(64)
k_period_close(int N, double eps, PeriodCloseArgs a)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, f = blockIdx.y, b = a.b0 + c;
    if (a.stop[c]) return;
    const int R = 2 * a.Fc;
    const int LD = acw_ld(N, 1);
    const AcwLds m = acw_carve(sm, N, 1, LD);
    const double* W = a.W + (size_t)c * (size_t)(N * N);
    double* v = a.v + (size_t)c * (size_t)(N * R);
    const double zKr = a.zKr[f], zKi = a.zKi[f];
    for (int idx = lane; idx < N * N; idx += 64) {
        const int i = idx / N, j = idx - i * N;
        double re, im;
        if (a.transposeW) pnoise_close_entry(i, j, N, W, zKr, zKi, &re, &im);
        else pac_close_entry(i, j, W[idx], zKr, zKi, &re, &im);
        m.Ar[i * LD + j] = re;
        m.Ai[i * LD + j] = im;
    }
    if (lane < N) {
        m.Ar[lane * LD + N] = v[lane * R + 2 * f];
        m.Ai[lane * LD + N] = v[lane * R + 2 * f + 1];
    }
    wave_sync();
    const bool failed = acw_solve(N, 1, LD, m.Ar, m.Ai, m.Lr, m.Li, m.Xr, m.Xi, eps * eps, lane);
    if (failed) {
        if (lane == 0) {
            a.stop[c] = 1;
            atomicOr(&a.status[b], CSIM_ST_PAC_SINGULAR | CSIM_ST_LU_TINY_PIVOT);
        }
        return;
    }
    if (lane < N) {
        v[lane * R + 2 * f] = m.Xr[lane];
        v[lane * R + 2 * f + 1] = m.Xi[lane];
    }
}

size_t pacLdsBytes(const GenPlan& pl, int Fc, int M, int nProbe)
{
    return sizeof(double) * (size_t)pacLds(pl.N, pl.LD, pl.nTerms, pl.P, Fc, M, nProbe).total;
}

int pacMaxFc(const GenPlan& pl, int M, int nProbe)
{
    for (int Fc = PAC_MAX_FC; Fc >= 1; --Fc)
        if (pacLdsBytes(pl, Fc, M, nProbe) <= PAC_LDS_LIMIT) return Fc;
    return 0;
}

hipError_t launchPacPeriod(const GenPlan& pl, const PacArgs& a, hipStream_t stream)
{
    if (pl.N < 1 || pl.N > 63 || a.Fc < 1 || a.Fc > PAC_MAX_FC || a.M < 0 || a.nProbe < 0) return hipErrorInvalidValue;
    const size_t lds = pacLdsBytes(pl, a.Fc, a.M, a.nProbe);
    if (lds > PAC_LDS_LIMIT) return hipErrorInvalidValue;
    return launchWave(k_pac_period, dim3(a.Bc), lds, stream, pl, a);
}

hipError_t launchPeriodClose(const GenPlan& pl, const PeriodCloseArgs& a, hipStream_t stream)
{
    if (pl.N < 1 || pl.N > 63 || a.Fc < 1 || a.Fc > PAC_MAX_FC) return hipErrorInvalidValue;
    return launchWave(k_period_close, dim3(a.Bc, a.Fc), acw_lds_bytes(pl.N, 1), stream, pl.N, pl.k.lu_eps, a);
}

} // namespace csim
