// kernels_pnoise.hip -- periodic noise analysis: the adjoint of the periodic AC recursion, backwards over a stored orbit
// (include/csim.h "Periodic noise analysis", arithmetic in pnoise.hpp, budget and measurements in DESIGN.md 8j).
//
//   k_pnoise_orbit   one wavefront = one workgroup = one instance, N <= 63.  K backward-Euler steps from x0, each one
//                    period_newton_step (pss_device.hpp), the step k_pss_period and k_pac_period take, so the orbit is
//                    theirs bit for bit; every converged x_k goes to the orbit store [c][k][N].
//   k_pnoise_period  one wavefront per instance, Fc <= 32 output frequencies.  k = K .. 1: x_k from the store, one MOSFET
//                    pass and one assembly of J_k, transposed (no Newton iterations), the right-hand side z g_k + d, the
//                    real LU on 2 Fc columns, the generators' sigma from the same MOSFET pass, the transfer sums (second
//                    pass only, kept in LDS and stored once), g_{k-1} = Hm^T q_k.  The first launch starts at g_K = 0
//                    and leaves r; the second starts at the g_K the close kernel solved for.
//
// The close kernel, (I - z_K W_K^T) g_K = r per (instance, frequency), is k_period_close (kernels_pac.hip) with W read
// transposed.
//
// The g and q planes are N x 2 Fc real: frequency f has its real part in column 2 f and its imaginary part in column
// 2 f + 1, and lane j owns column j as lu_solve_multi_wave wants.  LDS of the period kernel: the general kernel's
// carve-up, Hm (N x N, stored transposed so that the product walks a row), g and q (N x 2 Fc each), per generator its
// sigma and its two equations, and the sums, 2 (S + 1) (2 M + 1) Fc: sum (m, s, f) at (m (S + 1) + s) Fc + f.
#include <hip/hip_runtime.h>

#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"
#include "pnoise.hpp"
#include "pss_device.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

struct PnoiseLds { int Hm, Gp, Qp, sig, term, sums, total; };      // offsets in doubles
__host__ __device__ inline PnoiseLds pnoiseLds(int N, int LD, int nTerms, int P, int Fc, int M, int S)
{
    const int R = 2 * Fc, nGen = S + 1;
    PnoiseLds l;
    l.Hm = ldsLayout(N, LD, nTerms, P).total;
    l.Gp = l.Hm + N * N;
    l.Qp = l.Gp + N * R;
    l.sig = l.Qp + N * R;
    l.term = l.sig + nGen;                                  // 2 nGen int32
    l.sums = l.term + nGen;
    l.total = l.sums + 2 * (2 * M + 1) * nGen * Fc;
    return l;
}

// the matrix part of assemble(), every entry at its transposed place; the right-hand side column is not formed
__device__ __forceinline__ void assemble_transposed(const GenPlan& pl, const double* T, double* Gm, int lane)
{
    const int total = pl.N * pl.LD;
    for (int i = lane; i < total; i += 64) Gm[i] = 0.0;
    wave_sync();
    for (int n = lane; n < pl.nnzG; n += 64) {
        double acc = 0.0;
        for (int c = pl.gPtr[n]; c < pl.gPtr[n + 1]; ++c) {
            const int con = pl.gCon[c];
            const double v = T[con >> 1];
            acc = (con & 1) ? acc - v : acc + v;
        }
        const int pos = pl.gPos[n];
        const int r = pos / pl.LD, col = pos - r * pl.LD;
        Gm[col * pl.LD + r] = acc;
    }
    wave_sync();
}

} // namespace

__global__ void __launch_bounds__(64)
k_pnoise_orbit(GenPlan pl, PnoiseArgs a)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, b = a.b0 + c, B = a.B;
    const int N = pl.N, LD = pl.LD;
    const LdsLayout L = ldsLayout(N, LD, pl.nTerms, pl.P);
    double* Gm = sm + L.G;
    double* T = sm + L.T;
    double* Pv = sm + L.P;
    double* xs = sm + L.xs;
    double* xp = sm + L.xp;
    double* sc = sm + L.sc;

    unsigned st = 0;
    const double xin = (lane < N) ? a.x0[(int64_t)lane * B + b] : 0.0;
    if (period_start_status(a.status[b], a.wStatus[b], xin, N, lane, st)) {
        if (lane == 0) { a.orbitStop[c] = 1; a.status[b] |= st; }
        return;
    }

    period_load(pl, a.params, B, b, a.dt, Pv, T, xs, xin, xp, xin, lane);   // histories come from the previous state

    double* orbit = a.orbit + (size_t)c * (size_t)a.K * (size_t)N;
    bool aborted = false;
    for (long long s = 1; s <= a.K && !aborted; ++s) {
        // ---- the step, k_pss_period's; every converged state goes to the store
        if (!period_newton_step(pl, Pv, T, Gm, xs, xp, sc, s, a.dt, lane, st)) { aborted = true; break; }
        if (lane < N) orbit[(size_t)(s - 1) * (size_t)N + lane] = xs[lane];
    }
    if (lane == 0) {
        a.status[b] |= st;
        a.orbitStop[c] = aborted ? 1 : 0;
    }
}

__global__ void __launch_bounds__(64)
k_pnoise_period(GenPlan pl, PnoiseArgs a)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, b = a.b0 + c, B = a.B;
    const int N = pl.N, LD = pl.LD, Fc = a.Fc, R = 2 * Fc, S = a.S, nSb = 2 * a.M + 1;
    const LdsLayout L = ldsLayout(N, LD, pl.nTerms, pl.P);
    const PnoiseLds PL = pnoiseLds(N, LD, pl.nTerms, pl.P, Fc, a.M, S);
    double* Gm = sm + L.G;
    double* T = sm + L.T;
    double* Pv = sm + L.P;
    double* xs = sm + L.xs;
    double* xp = sm + L.xp;
    double* sc = sm + L.sc;
    double* HmT = sm + PL.Hm;                                           // HmT[i * N + l] = Hm(l, i)
    double* Gp = sm + PL.Gp;
    double* Qp = sm + PL.Qp;
    double* sig = sm + PL.sig;
    int32_t* term = reinterpret_cast<int32_t*>(sm + PL.term);          // generator s: equations term[2 s], term[2 s + 1]
    const int nGen = S + 1, nPair = nGen * Fc, nAcc = nSb * nPair;
    double* sre = sm + PL.sums;
    double* sim = sre + nAcc;
    const csim_consts& K = pl.k;
    const bool second = a.g0 != nullptr;

    auto zeros_out = [&]() {
        for (int f = lane; f < Fc; f += 64) a.onoise[(size_t)(a.fFirst + f) * (size_t)B + (size_t)b] = 0.0;
        for (int idx = lane; idx < nSb * Fc; idx += 64) {
            const int mi = idx / Fc, f = idx - mi * Fc;
            const size_t at = ((size_t)(a.fFirst + f) * (size_t)nSb + (size_t)mi) * (size_t)B + (size_t)b;
            if (a.side) a.side[at] = 0.0;
            if (a.gain) { a.gain[2 * at] = 0.0; a.gain[2 * at + 1] = 0.0; }
        }
        if (a.contrib)
            for (int idx = lane; idx < S * Fc; idx += 64) {
                const int s = idx / Fc, f = idx - s * Fc;
                a.contrib[((size_t)(a.fFirst + f) * (size_t)S + (size_t)s) * (size_t)B + (size_t)b] = 0.0;
            }
    };

    // an instance the orbit kernel, the first pass or the close kernel stopped
    if (a.orbitStop[c] != 0 || a.stop[c] != 0) {
        if (second) zeros_out();
        else if (lane == 0) a.stop[c] = 1;
        return;
    }

    unsigned st = 0;
    period_load(pl, a.params, B, b, a.dt, Pv, T, xs, 0.0, xp, 0.0, lane);
    period_hm(pl, Pv, T, xp, sc, HmT, 1, N, lane);                      // column l of Hm becomes row l of HmT
    for (int g = lane; g < nGen; g += 64) {
        term[2 * g] = g < S ? a.srcA[g] : a.inA;
        term[2 * g + 1] = g < S ? a.srcB[g] : a.inB;
    }
    const int fq = lane >> 1;                                           // this lane's frequency and part (lane < R)
    const bool imPart = (lane & 1) != 0;
    const double zr = (lane < R) ? a.zr[fq] : 0.0, zi = (lane < R) ? a.zi[fq] : 0.0;
    const double* g0 = second ? a.g0 + (size_t)c * (size_t)(N * R) : nullptr;
    for (int i = 0; i < N; ++i)
        if (lane < R) Gp[i * R + lane] = g0 ? g0[i * R + lane] : 0.0;
    for (int idx = lane; idx < nAcc; idx += 64) { sre[idx] = 0.0; sim[idx] = 0.0; }
    wave_sync();

    const double* orbit = a.orbit + (size_t)c * (size_t)a.K * (size_t)N;
    bool aborted = false;
    for (long long s = a.K; s >= 1; --s) {
        // ---- J_k^T at the stored state
        if (lane < N) xs[lane] = orbit[(size_t)(s - 1) * (size_t)N + lane];
        wave_sync();
        terms_iter_mos(pl, Pv, T, xs, lane);
        wave_sync();
        assemble_transposed(pl, T, Gm, lane);

        // ---- q = J_k^-T (z g + d)
        for (int i = 0; i < N; ++i)
            if (lane < R) {
                const double d = i == a.outP ? 1.0 : (i == a.outM ? -1.0 : 0.0);
                double re, im;
                pnoise_step_rhs(zr, zi, Gp[i * R + 2 * fq], Gp[i * R + 2 * fq + 1], d, &re, &im);
                Qp[i * R + lane] = imPart ? im : re;
            }
        wave_sync();
        if (!lu_solve_multi_wave(Gm, N, LD, Qp, R, R, K.lu_eps, lane)) {
            st |= CSIM_ST_PAC_SINGULAR | CSIM_ST_LU_TINY_PIVOT;
            aborted = true;
            break;
        }

        // ---- the generators at x_k and the transfer sums (pnoise.hpp), k descending; sum idx is always this lane's
        if (second) {
            for (int g = lane; g < nGen; g += 64) {
                double v = 1.0;                                         // the input source
                if (g < S) {
                    const int e = a.srcElem[g];
                    const int kind = pl.kind[e];
                    double psd = 0.0;
                    if (kind == CSIM_R) psd = pnoise_psd_r(a.kT4, Pv[pl.slot[e]]);
                    else if (kind == CSIM_NMOS || kind == CSIM_PMOS) psd = pnoise_psd_mos(a.kT4, T[pl.termBase[e] + T_M_GG]);
                    v = pnoise_sigma(psd);
                }
                sig[g] = v;
            }
            wave_sync();
            for (int idx = lane; idx < nPair; idx += 64) {
                const int g = idx / Fc, f = idx - g * Fc;
                double dr, di;
                pnoise_diff(Qp, R, f, term[2 * g], term[2 * g + 1], &dr, &di);
                const double sg = sig[g];
                for (int mi = 0; mi < nSb; ++mi) {
                    const int j = pac_tw_index(mi - a.M, s, a.K);
                    double re = sre[mi * nPair + idx], im = sim[mi * nPair + idx];
                    pnoise_sum_add(sg, dr, di, a.twc[j], a.tws[j], &re, &im);
                    sre[mi * nPair + idx] = re;
                    sim[mi * nPair + idx] = im;
                }
            }
        }

        // ---- g = Hm^T q, walking the non-zeros of Hm's column
        period_hm_product(HmT, N, Qp, R, Gp, R, R, lane);
    }

    if (lane == 0) {
        a.status[b] |= st;
        if (aborted) a.stop[c] = 1;
    }
    if (!second) {
        if (!aborted) {
            double* gK = a.gK + (size_t)c * (size_t)(N * R);
            for (int i = 0; i < N; ++i)
                if (lane < R) gK[i * R + lane] = Gp[i * R + lane];
        }
        return;
    }
    if (aborted) { zeros_out(); return; }

    for (int idx = lane; idx < nAcc; idx += 64) {
        double re = sre[idx], im = sim[idx];
        pac_sum_finish(a.K, &re, &im);
        sre[idx] = re;
        sim[idx] = im;
    }
    wave_sync();
    // lane f adds up frequency f: contributions over the sidebands, the sidebands over the generators, the total
    if (lane < Fc) {
        const int f = lane;
        const size_t fb = (size_t)(a.fFirst + f);
        double total = 0.0;
        for (int s = 0; s < S; ++s) {
            double cs = 0.0;
            for (int mi = 0; mi < nSb; ++mi) {
                const int at = (mi * nGen + s) * Fc + f;
                cs = cs + pnoise_abs2(sre[at], sim[at]);
            }
            if (a.contrib) a.contrib[(fb * (size_t)S + (size_t)s) * (size_t)B + (size_t)b] = cs;
            total = total + cs;
        }
        a.onoise[fb * (size_t)B + (size_t)b] = total;
        for (int mi = 0; mi < nSb; ++mi) {
            const size_t at = (fb * (size_t)nSb + (size_t)mi) * (size_t)B + (size_t)b;
            if (a.side) {
                double sd = 0.0;
                for (int s = 0; s < S; ++s) {
                    const int w = (mi * nGen + s) * Fc + f;
                    sd = sd + pnoise_abs2(sre[w], sim[w]);
                }
                a.side[at] = sd;
            }
            if (a.gain) {
                const int w = (mi * nGen + S) * Fc + f;
                a.gain[2 * at] = sre[w];
                a.gain[2 * at + 1] = sim[w];
            }
        }
    }
}

size_t pnoiseLdsBytes(const GenPlan& pl, int Fc, int M, int S)
{
    return sizeof(double) * (size_t)pnoiseLds(pl.N, pl.LD, pl.nTerms, pl.P, Fc, M, S).total;
}

int pnoiseMaxFc(const GenPlan& pl, int M, int S)
{
    for (int Fc = PAC_MAX_FC; Fc >= 1; --Fc)
        if (pnoiseLdsBytes(pl, Fc, M, S) <= PAC_LDS_LIMIT) return Fc;
    return 0;
}

hipError_t launchPnoiseOrbit(const GenPlan& pl, const PnoiseArgs& a, hipStream_t stream)
{
    if (pl.N < 1 || pl.N > 63 || a.K < 1 || !a.orbit) return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * (size_t)ldsLayout(pl.N, pl.LD, pl.nTerms, pl.P).total;
    if (lds > PAC_LDS_LIMIT) return hipErrorInvalidValue;
    return launchWave(k_pnoise_orbit, dim3(a.Bc), lds, stream, pl, a);
}

hipError_t launchPnoisePeriod(const GenPlan& pl, const PnoiseArgs& a, hipStream_t stream)
{
    if (pl.N < 1 || pl.N > 63 || a.Fc < 1 || a.Fc > PAC_MAX_FC || a.M < 0 || a.S < 0 || a.K < 1) return hipErrorInvalidValue;
    if (a.outP < 0 || a.outP >= pl.N || a.outM < -1 || a.outM >= pl.N || a.inA >= pl.N || a.inB >= pl.N) return hipErrorInvalidValue;
    const size_t lds = pnoiseLdsBytes(pl, a.Fc, a.M, a.S);
    if (lds > PAC_LDS_LIMIT) return hipErrorInvalidValue;
    return launchWave(k_pnoise_period, dim3(a.Bc), lds, stream, pl, a);
}

} // namespace csim
