// kernels_pss.hip -- periodic steady state by shooting Newton (include/csim.h "Periodic steady state", arithmetic
// in pss.hpp, budget and measurements in DESIGN.md 8h).
//
//   k_pss_period   one wavefront = one workgroup = one instance, N <= 63.  K backward-Euler steps from x0, each one
//                  period_newton_step (pss_device.hpp: k_tran_general's body, so the trajectory is that kernel's bit
//                  for bit, and the one step the periodic AC and noise kernels take too); after every converged step
//                  the sensitivity W_k = J_k^-1 (Hm W_{k-1}) and the DFT sums of the probes.  Leaves x_K, W_K and the
//                  harmonics of this period.
//   k_pss_update   one wavefront per instance: r = x_K - x0, the closure test, (I - W_K) d = r through lu_solve_wave,
//                  x0 += d; counts the instances that go on.
//
// LDS of the period kernel: the general kernel's carve-up (matrix N x LD, terms, parameters, two state vectors), then
// W (N x N) and Hm (N x N).  The product Hm W_{k-1} is formed in the matrix area, which is dead between a step's last
// solve and the sensitivity assembly, and copied over W, so no third N x N plane is needed: 97 KB at N = 63, 24 KB at
// N = 31.  One wave does both phases: lane j owns column j of the matrix and of W, the elimination walks the non-zero
// multipliers only, and nothing but wave_sync orders the two phases.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "kernels.hpp"
#include "pss.hpp"
#include "pss_device.hpp"

namespace csim {

namespace {

__device__ __forceinline__ size_t pss_harm_at(const PssArgs& a, int idx, int b) { return 2 * ((size_t)idx * (size_t)a.B + (size_t)b); }

} // namespace

__global__ void __launch_bounds__(64)
k_pss_period(GenPlan pl, PssArgs a)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, b = a.b0 + c, B = a.B;
    if (a.done[b]) return;
    const int N = pl.N, LD = pl.LD;
    const LdsLayout L = ldsLayout(N, LD, pl.nTerms, pl.P);
    double* Gm = sm + L.G;
    double* T = sm + L.T;
    double* Pv = sm + L.P;
    double* xs = sm + L.xs;
    double* xp = sm + L.xp;
    double* sc = sm + L.sc;
    double* Wm = sm + L.total;
    double* Hm = Wm + N * N;
    const csim_consts& K = pl.k;

    unsigned st = a.status[b] & CSIM_ST_TRAN_NONFINITE;
    const double xin = (lane < N) ? a.x0[(int64_t)lane * B + b] : 0.0;
    if (!wave_all_finite(xin, N, lane)) st |= CSIM_ST_TRAN_NONFINITE;    // a start vector that is not finite stops its instance
    const int nAcc = (a.H + 1) * a.nProbe;
    for (int idx = lane; idx < nAcc; idx += 64) {                       // the sums start at zero; a stopped instance reports zeros
        const size_t at = pss_harm_at(a, idx, b);
        a.harm[at] = 0.0;
        a.harm[at + 1] = 0.0;
    }
    if (st & CSIM_ST_TRAN_NONFINITE) {
        if (lane == 0) a.status[b] |= st;
        return;                                                         // the update kernel closes the instance
    }

    period_load(pl, a.params, B, b, a.dt, Pv, T, xs, xin, xp, 0.0, lane);
    period_hm(pl, Pv, T, xp, sc, Hm, N, 1, lane);
    for (int i = 0; i < N; ++i)
        if (lane < N) Wm[i * N + lane] = (i == lane) ? 1.0 : 0.0;     // W_0 = I
    if (lane < N) xp[lane] = xin;                                       // histories come from the previous state
    wave_sync();

    bool aborted = false;
    for (long long s = 1; s <= a.K && !aborted; ++s) {
        // ---- the step
        if (!period_newton_step(pl, Pv, T, Gm, xs, xp, sc, s, a.dt, lane, st)) { aborted = true; break; }

        // ---- sensitivity: Hm W_{k-1} into the matrix area (dead here), over W, then J_k at the converged iterate
        period_hm_product(Hm, N, Wm, N, Gm, LD, N, lane);
        for (int i = 0; i < N; ++i)
            if (lane < N) Wm[i * N + lane] = Gm[i * LD + lane];
        wave_sync();
        terms_iter_mos(pl, Pv, T, xs, lane);
        wave_sync();
        assemble(pl, T, Gm, lane);
        if (!lu_solve_multi_wave(Gm, N, LD, Wm, N, N, K.lu_eps, lane)) {
            st |= CSIM_ST_PSS_SINGULAR | CSIM_ST_LU_TINY_PIVOT;
            aborted = true;
            break;
        }

        // ---- DFT sums of the probes (pss.hpp), k ascending
        for (int idx = lane; idx < nAcc; idx += 64) {
            const int m = idx / a.nProbe, q = idx - m * a.nProbe;
            const int eq = a.probeEq ? a.probeEq[q] : q;
            const int j = pss_tw_index(m, s, a.K);
            const size_t at = pss_harm_at(a, idx, b);
            double re = a.harm[at], im = a.harm[at + 1];
            pss_dft_add(xs[eq], a.twc[j], a.tws[j], &re, &im);
            a.harm[at] = re;
            a.harm[at + 1] = im;
        }
    }

    for (int idx = lane; idx < nAcc; idx += 64) {
        const size_t at = pss_harm_at(a, idx, b);
        double re = a.harm[at], im = a.harm[at + 1];
        pss_dft_finish(idx / a.nProbe, a.K, &re, &im);
        a.harm[at] = re;
        a.harm[at + 1] = im;
    }
    if (lane < N) a.xK[(int64_t)lane * B + b] = xs[lane];
    double* Wout = a.W + (size_t)c * (size_t)(N * N);
    for (int i = lane; i < N * N; i += 64) Wout[i] = Wm[i];
    if (lane == 0) a.status[b] |= st;
}

__global__ void __launch_bounds__(64)
k_pss_update(int N, int LD, double eps, PssArgs a)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, b = a.b0 + c, B = a.B;
    if (a.done[b]) return;
    const int rounds = a.rounds[b] + 1;
    const unsigned st = a.status[b];
    auto close = [&](unsigned add) {
        if (lane == 0) {
            a.done[b] = 1;
            a.rounds[b] = rounds;
            if (add) a.status[b] = st | add;
        }
    };
    if (st & (CSIM_ST_TRAN_NONFINITE | CSIM_ST_PSS_SINGULAR)) { close(0u); return; }

    double* Gm = sm;
    double* sc = sm + N * LD;
    const double x0 = (lane < N) ? a.x0[(int64_t)lane * B + b] : 0.0;
    const double r = (lane < N) ? pss_residual(a.xK[(int64_t)lane * B + b], x0) : 0.0;
    if (lane < N) sc[lane] = r;
    wave_sync();
    const double nrm = pss_norm_inf(sc, N);
    if (pss_closed(nrm, a.tol)) { close(0u); return; }
    if (rounds >= a.maxRounds) { close(CSIM_ST_PSS_NONCONV); return; }     // x0 stays: the harmonics belong to it

    const double* Win = a.W + (size_t)c * (size_t)(N * N);
    for (int i = 0; i < N; ++i)
        if (lane < N) Gm[i * LD + lane] = pss_shoot_entry(i, lane, Win[i * N + lane]);
    if (lane < N) Gm[lane * LD + N] = r;
    wave_sync();
    unsigned fl = 0;
    const double d = lu_solve_wave(Gm, N, LD, eps, lane, fl);
    if (fl & CSIM_ST_LU_TINY_PIVOT) { close(CSIM_ST_PSS_SINGULAR | fl); return; }
    if (lane < N) a.x0[(int64_t)lane * B + b] = pss_update(x0, d);
    if (lane == 0) {
        a.rounds[b] = rounds;
        if (fl) a.status[b] = st | fl;
        atomicAdd(a.unfinished, 1);
    }
}

size_t pssLdsBytes(const GenPlan& pl)
{
    return sizeof(double) * ((size_t)ldsLayout(pl.N, pl.LD, pl.nTerms, pl.P).total + 2 * (size_t)pl.N * (size_t)pl.N);
}

hipError_t launchPssPeriod(const GenPlan& pl, const PssArgs& a, hipStream_t stream)
{
    if (pl.N < 1 || pl.N > 63) return hipErrorInvalidValue;
    return launchWave(k_pss_period, dim3(a.Bc), pssLdsBytes(pl), stream, pl, a);
}

hipError_t launchPssRound(const GenPlan& pl, const PssArgs& a, hipStream_t stream)
{
    hipError_t e = launchPssPeriod(pl, a, stream);
    if (e != hipSuccess) return e;
    const size_t ldsU = sizeof(double) * ((size_t)pl.N * pl.LD + (size_t)pl.N);
    hipLaunchKernelGGL(k_pss_update, dim3(a.Bc), dim3(64), ldsU, stream, pl.N, pl.LD, pl.k.lu_eps, a);
    return hipGetLastError();
}

} // namespace csim
