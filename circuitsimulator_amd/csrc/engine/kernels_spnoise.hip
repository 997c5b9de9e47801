// kernels_spnoise.hip -- two-port noise analysis: Y, the port noise-current correlation matrix Cy and (two ports) NF,
// Fmin, Rn, Yopt of B instances x F frequencies by one factorisation of A^T with one adjoint right-hand side per port
// (include/csim.h "Two-port noise analysis", arithmetic in ac_port_noise.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major; its J is not read); the
// generators' PSDs are those noise_psd_kernel leaves.  Two kernels, the shapes of kernels_noise.hip carrying the
// right-hand sides of kernels_sp.hip:
//
//   spn_sweep_wave_kernel<KP>        one wavefront per instance, N <= 63: A^T and its P right-hand sides in LDS
//                                    (acw_load<true>, odd leading dimension >= N + P), acw_solve() of ac_sweep.hpp.
//   spn_sweep_packed_kernel<NP, KP>  N <= 32: 32 lanes per instance, lane r owns row r of A^T in registers
//                                    ar/ai[NP + KP], acp_column / acp_back; G, then C, staged in address order through
//                                    the noise kernel's LDS tile.  P is rounded up to KP in {2, 4}; a padded zero
//                                    column changes no other column and is never read.
//
// Epilogue, the same in both: the P solutions sit in LDS; the lanes stride over the generators in chunks of the lane
// count, each forms its generator's P transfers and the P (P + 1) / 2 correlation products; the products travel to
// every lane in ascending generator order (readlane / shuffle) and are added in that order.  One lane per instance
// writes Y and Cy to LDS and runs the two-port arithmetic; P * P lanes store Y and Cy.  Every register array is
// indexed with constants (loops over KP, unrolled).  Both kernels apply ac_port_noise.hpp's primitives to every entry
// in the same order: their outputs are bit-identical.
#include <hip/hip_runtime.h>

#include "ac_port_noise.hpp"
#include "ac_sweep.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

constexpr int PP = SP_MAX_PORTS * SP_MAX_PORTS;

// LDS of one instance's epilogue
struct SpnEpi {
    double yr[PP], yi[PP], cr[PP], ci[PP];
    int32_t eq[SP_MAX_PORTS];
};

// kernel arguments -> LDS, with constant indices (an argument array indexed at run time would live in scratch)
__device__ __forceinline__ void spn_ports_to_lds(const SpNoiseArgs& a, SpnEpi& e, int r)
{
    if (r == 0) e.eq[0] = a.portEq[0];
    if (r == 1) e.eq[1] = a.portEq[1];
    if (r == 2) e.eq[2] = a.portEq[2];
    if (r == 3) e.eq[3] = a.portEq[3];
}

// Sums over the generators of the correlation products of the pairs (i, j), i <= j < P: lane `lane` of LANES takes
// generator s0 + lane of every chunk, bcast(v, t) hands lane t's value to every lane.  X: solution i at X[i * ldx ...].
template <int KP, int LANES, class Bcast>
__device__ __forceinline__ void spn_correlate(const SpNoiseArgs& a, bool failed, const double* Xr, const double* Xi, int ldx,
                                              int lane, int c, Bcast bcast, double (&sumRe)[KP * (KP + 1) / 2],
                                              double (&sumIm)[KP * (KP + 1) / 2])
{
    constexpr int NPAIR = KP * (KP + 1) / 2;
    const int P = a.P, S = a.S;
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) { sumRe[p] = 0.0; sumIm[p] = 0.0; }
    for (int s0 = 0; s0 < S; s0 += LANES) {
        const int s = s0 + lane;
        double qr[NPAIR], qi[NPAIR];
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) { qr[p] = 0.0; qi[p] = 0.0; }
        if (s < S && !failed) {
            const int sa = a.srcA[s], sb = a.srcB[s];
            const double psd = a.psd[(size_t)s * a.psdStride + a.psdOff + (size_t)c];
            cpx t[KP];
#pragma unroll
            for (int i = 0; i < KP; ++i)
                t[i] = i < P ? noise_transfer(Xr + i * ldx, Xi + i * ldx, sa, sb) : cpx{0.0, 0.0};
#pragma unroll
            for (int i = 0; i < KP; ++i) {
#pragma unroll
                for (int j = i; j < KP; ++j) {
                    if (j < P) {
                        const cpx q = spn_corr(t[i], t[j], psd);
                        qr[spn_pair(KP, i, j)] = q.re;
                        if (i != j) qi[spn_pair(KP, i, j)] = q.im;
                    }
                }
            }
        }
        const int cnt = min(LANES, S - s0);
        for (int g = 0; g < cnt; ++g) {
#pragma unroll
            for (int i = 0; i < KP; ++i) {
#pragma unroll
                for (int j = i; j < KP; ++j) {
                    if (j < P) {
                        const int p = spn_pair(KP, i, j);
                        sumRe[p] = sumRe[p] + bcast(qr[p], g);
                        if (i != j) sumIm[p] = sumIm[p] + bcast(qi[p], g);
                    }
                }
            }
        }
    }
}

// one lane: Y and Cy to LDS, then the noise parameters of (frequency f, instance b)
template <int KP>
__device__ __forceinline__ void spn_finish(const SpNoiseArgs& a, SpnEpi& e, bool failed, const double* Xr, const double* Xi,
                                           int ldx, const double (&sumRe)[KP * (KP + 1) / 2],
                                           const double (&sumIm)[KP * (KP + 1) / 2], int f, int b)
{
    const int P = a.P;
    spn_read_y(P, e.eq, failed, Xr, Xi, ldx, e.yr, e.yi);
    spn_fill_cy<KP>(P, failed, sumRe, sumIm, e.cr, e.ci);
    if (P != 2 || !(a.nf || a.fmin || a.rn || a.yopt)) return;
    const TwoPortNoise o = failed ? spn_failed()
                                  : spn_two_port({e.yr[0], e.yi[0]}, {e.yr[2], e.yi[2]}, e.cr[0], e.cr[3], {e.cr[1], e.ci[1]},
                                                 a.kT40, a.gs);
    const size_t at = (size_t)f * (size_t)a.B + (size_t)b;
    if (a.nf) a.nf[at] = o.nf;
    if (a.fmin) a.fmin[at] = o.fmin;
    if (a.rn) a.rn[at] = o.rn;
    if (a.yopt) {
        a.yopt[2 * at] = o.yoptRe;
        a.yopt[2 * at + 1] = o.yoptIm;
    }
}

// entry t = i * P + j of Y and Cy of (frequency f, instance b): [F][P][P][B] complex
__device__ __forceinline__ void spn_store(const SpNoiseArgs& a, const SpnEpi& e, int f, int b, int t)
{
    const size_t at = (((size_t)f * (size_t)(a.P * a.P) + (size_t)t) * (size_t)a.B + (size_t)b) * 2;
    a.cy[at] = e.cr[t];
    a.cy[at + 1] = e.ci[t];
    if (a.y) {
        a.y[at] = e.yr[t];
        a.y[at + 1] = e.yi[t];
    }
}

// adjoint solution c, unknown i of (frequency f, instance b): [F][P][N][B] complex
__device__ __forceinline__ size_t spn_x_at(const SpNoiseArgs& a, int f, int c, int i, int b)
{
    return ((((size_t)f * (size_t)a.P + (size_t)c) * (size_t)a.N + (size_t)i) * (size_t)a.B + (size_t)b) * 2;
}

// ---- wave per system (N <= 63)
template <int KP>
__global__ void __launch_bounds__(64) spn_sweep_wave_kernel(SpNoiseArgs a)
{
    extern __shared__ double lds[];
    __shared__ SpnEpi epi;
    const int lane = threadIdx.x;
    const int N = a.N, P = a.P;
    const int c0 = blockIdx.x, b = a.b0 + c0;
    const int LD = acw_ld(N, P);
    const AcwLds m = acw_carve(lds, N, P, LD);
    double *const Ar = m.Ar, *const Ai = m.Ai, *const Xr = m.Xr, *const Xi = m.Xi;      // solution c at c * 64
    const double* Gt = ac_system_at(a.sys, c0, N);
    const double* Ct = Gt + N * N;
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;
    spn_ports_to_lds(a, epi, lane);
    wave_sync();

    for (int f = 0; f < a.F; ++f) {
        const double w = a.omega[f];
        acw_load<true>(N, LD, Gt, Ct, w, Ar, Ai, lane);
        for (int e = lane; e < N * P; e += 64) {
            const int c = e / N, i = e - c * N;
            Ar[i * LD + N + c] = i == epi.eq[c] ? 1.0 : 0.0;
            Ai[i * LD + N + c] = 0.0;
        }
        wave_sync();

        const bool failed = acw_solve(N, P, LD, Ar, Ai, m.Lr, m.Li, Xr, Xi, eps2, lane);
        if (failed) flags |= CSIM_ST_LU_TINY_PIVOT;
        if (a.x)
            for (int e = lane; e < N * P; e += 64) {
                const int c = e / N, i = e - c * N;
                const size_t at = spn_x_at(a, f, c, i, b);
                a.x[at] = Xr[c * 64 + i];                    // zeros when the factorisation failed
                a.x[at + 1] = Xi[c * 64 + i];
            }
        double sumRe[KP * (KP + 1) / 2], sumIm[KP * (KP + 1) / 2];
        spn_correlate<KP, 64>(a, failed, Xr, Xi, 64, lane, c0, [](double v, int g) { return read_lane(v, g); }, sumRe,
                              sumIm);
        if (lane == 0) spn_finish<KP>(a, epi, failed, Xr, Xi, 64, sumRe, sumIm, f, b);
        wave_sync();
        if (lane < P * P) spn_store(a, epi, f, b, lane);
        wave_sync();
    }
    if (lane == 0 && flags) a.status[b] |= flags;
}

// ---- register-resident, 32 lanes per system (N <= NP <= 32), KP >= P right-hand-side registers
template <int NP, int KP>
__global__ void __launch_bounds__(64) spn_sweep_packed_kernel(SpNoiseArgs a)
{
    constexpr int LDT = NP + 1;                             // odd: lane r reading word r * LDT + j is conflict-free
    __shared__ double tile[2][NP * LDT];                    // [instance] staged G, then C, as rows of A^T
    __shared__ double xs[2][2][KP * ACP_LANES];             // [instance][re, im][solution c at c * 32]
    __shared__ SpnEpi epis[2];
    const int N = a.N, P = a.P;
    const AcpInstance t = acp_instance(a.b0, a.Bc);
    const int h = t.h, r = t.r, cc = t.cc, b = t.b;
    const bool on = t.on;
    const double* Gt = ac_system_at(a.sys, cc, N);
    const double* Ct = Gt + N * N;
    double* T = tile[h];
    double* Xr = xs[h][0];
    double* Xi = xs[h][1];
    SpnEpi& epi = epis[h];
    const double eps2 = a.eps * a.eps;
    unsigned flags = 0u;
    spn_ports_to_lds(a, epi, r);
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
            ar[NP + c] = (c < P && r < N && r == epi.eq[c]) ? 1.0 : 0.0;
            ai[NP + c] = 0.0;
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
            for (int c = 0; c < P; ++c) {
                const size_t at = spn_x_at(a, f, c, r, b);
                a.x[at] = Xr[c * ACP_LANES + r];
                a.x[at + 1] = Xi[c * ACP_LANES + r];
            }
        double sumRe[KP * (KP + 1) / 2], sumIm[KP * (KP + 1) / 2];
        spn_correlate<KP, ACP_LANES>(a, failed, Xr, Xi, ACP_LANES, r, cc,
                                     [](double v, int g) { return __shfl(v, g, ACP_LANES); }, sumRe, sumIm);
        if (on && r == 0) spn_finish<KP>(a, epi, failed, Xr, Xi, ACP_LANES, sumRe, sumIm, f, b);
        __syncthreads();
        if (on && r < P * P) spn_store(a, epi, f, b, r);
        __syncthreads();
    }
    if (on && r == 0 && flags) a.status[b] |= flags;
}

} // namespace

hipError_t launchSpNoiseSweep(int which, const SpNoiseArgs& a, hipStream_t stream)
{
    if (a.Bc <= 0 || a.F <= 0) return hipSuccess;
    const int N = a.N;
    if (!ac_sweep_covers(which, N)) return hipErrorInvalidValue;
    if (a.P < 1 || a.P > SP_MAX_PORTS || a.S < 0 || !a.cy) return hipErrorInvalidValue;
    for (int p = 0; p < a.P; ++p)
        if (a.portEq[p] < 0 || a.portEq[p] >= N) return hipErrorInvalidValue;       // they index LDS
    if (a.P != 2 && (a.nf || a.fmin || a.rn || a.yopt)) return hipErrorInvalidValue;
    if (which == AC_KERNEL_PACKED) {
        acp_dispatch(N, [&](auto np) {
            constexpr int NP = decltype(np)::value;
            const dim3 grid((a.Bc + 1) / 2);
            if (a.P <= 2) hipLaunchKernelGGL((spn_sweep_packed_kernel<NP, 2>), grid, dim3(64), 0, stream, a);
            else hipLaunchKernelGGL((spn_sweep_packed_kernel<NP, 4>), grid, dim3(64), 0, stream, a);
        });
    } else {
        const size_t lds = acw_lds_bytes(N, a.P);
        if (lds + sizeof(SpnEpi) > 160 * 1024) return hipErrorInvalidValue;
        const void* fn = a.P <= 2 ? (const void*)spn_sweep_wave_kernel<2> : (const void*)spn_sweep_wave_kernel<4>;
        if (lds + sizeof(SpnEpi) > 64 * 1024)
            (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (a.P <= 2) hipLaunchKernelGGL(spn_sweep_wave_kernel<2>, dim3(a.Bc), dim3(64), lds, stream, a);
        else hipLaunchKernelGGL(spn_sweep_wave_kernel<4>, dim3(a.Bc), dim3(64), lds, stream, a);
    }
    return hipGetLastError();
}

} // namespace csim
