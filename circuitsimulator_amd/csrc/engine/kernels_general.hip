// kernels_general.hip -- wave-per-instance kernels (gfx950): DC operating
// point (K2), backward-Euler transient (K1) and the stand-alone batched LU.
//
// One 64-lane wavefront = one workgroup = one circuit instance; the dense
// augmented system sits in LDS and is solved in place (device_common.hpp).
// These kernels take any circuit with N <= 63 unknowns and make every pivot
// decision at run time, exactly as the reference does; they are the planner
// and the fallback of the circuit-specialised lane-per-instance kernels.
//
// Iteration control restated from the reference:
//   k_dc_general    dcSolveLU dispatch          src/dcanalysis.cpp:242-262
//                   dcSolveDirectLU             src/dcanalysis.cpp:46-68
//                   dcSolveNewtonLU             src/dcanalysis.cpp:95-163
//                   ConvController::update      src/dcanalysis.cpp:268-307
//   k_tran_general  runTransientAnalysisBackwardEuler  src/tanalisis.cpp:238-420
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "general_shapes.hpp"

namespace csim {

// ------------------------------------------------------------------ DC (K2)
__global__ void __launch_bounds__(64)
k_dc_general(GenPlan pl, GenDcArgs a)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int b = blockIdx.x, B = a.B;
    if (a.only && !a.only[b]) return;       // fallback / planner launches touch the flagged instances only
    int32_t* myPivLog = (a.pivLog && b == a.pivInstance) ? a.pivLog : nullptr;
    const int N = pl.N, LD = pl.LD;
    const LdsLayout L = ldsLayout(N, LD, pl.nTerms, pl.P);
    double* Gm = sm + L.G;
    double* T = sm + L.T;
    double* Pv = sm + L.P;
    double* xs = sm + L.xs;
    double* sc = sm + L.sc;
    const csim_consts& K = pl.k;

    for (int p = lane; p < pl.P; p += 64) Pv[p] = a.params[(int64_t)p * B + b];
    for (int t = lane; t < pl.nTerms; t += 64) T[t] = 0.0;
    if (lane < N) xs[lane] = 0.0;
    wave_sync();
    terms_const<false>(pl, Pv, T, 0.0, lane);
    wave_sync();

    unsigned st = 0;
    int itTotal = 0;

    if (!pl.hasNonlinear) {
        // linear circuit: one solve at x = 0, full sources, NO gmin (dcanalysis.cpp:46-68)
        terms_step_dc(pl, Pv, T, 1.0, lane);
        if (lane == 0) T[pl.termGmin] = 0.0;
        wave_sync();
        assemble(pl, T, Gm, lane);
        const double xr = lu_solve_wave(Gm, N, LD, K.lu_eps, lane, st, myPivLog);
        if (lane < N) xs[lane] = xr;
        itTotal = 1;
    } else {
        for (int step = 1; step <= K.dc_ramp_steps; ++step) {
            const double scale = (double)step / K.dc_ramp_steps;        // :113
            double gmin = base_gmin(K, scale);                          // :116
            double prevErr = INFINITY;                                  // :117
            terms_step_dc(pl, Pv, T, scale, lane);
            wave_sync();
            for (int iter = 0; iter < K.dc_max_iters; ++iter) {
                terms_iter_mos(pl, Pv, T, xs, lane);
                if (lane == 0) T[pl.termGmin] = gmin;
                wave_sync();
                assemble(pl, T, Gm, lane);
                const double xr = lu_solve_wave(Gm, N, LD, K.lu_eps, lane, st, myPivLog, nullptr);   // :134
                ++itTotal;
                if (!wave_all_finite(xr, N, lane)) {                    // :135-138
                    gmin = fmin(gmin * K.gmin_nonfinite_mul, K.gmin_nonfinite_cap);
                    st |= CSIM_ST_DC_NONFINITE;
                    continue;
                }
                // ConvController::update
                const double xo = (lane < N) ? xs[lane] : 0.0;
                const double xn = xo + dc_alpha(K) * (xr - xo);         // :275
                const double err = norm_in_order(xn - xo, sc, N, lane); // :276
                const double gnext = conv_gmin_next(K, iter, err, prevErr, gmin, base_gmin(K, scale));
                if (lane < N) xs[lane] = xn;                            // :145
                wave_sync();
                gmin = gnext;
                prevErr = err;
                if (err < K.dc_tol) break;                              // :150
                if (iter == K.dc_max_iters - 1) st |= CSIM_ST_DC_NONCONV;   // :153-158
            }
        }
    }
    wave_sync();
    if (lane < N) a.x[(int64_t)lane * B + b] = xs[lane];
    if (lane == 0) {
        a.iters[b] = itTotal;
        a.status[b] = (a.only && !a.pivLog) ? (st | CSIM_ST_SCHED_FALLBACK_DC) : st;
    }
}

// ------------------------------------------------------------ transient (K1)
__global__ void __launch_bounds__(64)
k_tran_general(GenPlan pl, GenTranArgs a)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int b = blockIdx.x, B = a.B;
    if (a.only && !a.only[b]) return;       // planner launches touch the chosen instance only
    const StepWindow w = step_window(a.done, b, a.nSteps, a.maxSteps);
    if (a.done && w.d0 >= a.nSteps) return;
    int32_t* myPivLog = (a.pivLog && b == a.pivInstance) ? a.pivLog : nullptr;
    const int N = pl.N, LD = pl.LD;
    const LdsLayout L = ldsLayout(N, LD, pl.nTerms, pl.P);
    double* Gm = sm + L.G;
    double* T = sm + L.T;
    double* Pv = sm + L.P;
    double* xs = sm + L.xs;
    double* xp = sm + L.xp;
    double* sc = sm + L.sc;
    int32_t* curPiv = (a.done && a.knownAlts) ? reinterpret_cast<int32_t*>(sm + L.piv) : nullptr;
    const csim_consts& K = pl.k;

    for (int p = lane; p < pl.P; p += 64) Pv[p] = a.params[(int64_t)p * B + b];
    for (int t = lane; t < pl.nTerms; t += 64) T[t] = 0.0;
    if (lane < N) {
        const double v = a.x[(int64_t)lane * B + b];
        xs[lane] = v;
        xp[lane] = v;                       // histories come from the previous state (:139-180)
    }
    wave_sync();
    terms_const<true>(pl, Pv, T, a.dt, lane);
    if (lane == 0) T[pl.termGmin] = K.tran_gmin;
    wave_sync();

    if (a.stepFirst == 0 && w.d0 == 0 && a.wave)    // t = 0 row (:250)
        store_probe_row(a.wave, 0, a.probeEq, a.nProbe, B, b, xs, lane, 64);

    unsigned st = (a.status[b] & CSIM_ST_TRAN_NONFINITE);
    if (a.done) st |= CSIM_ST_SCHED_FALLBACK;
    long long itTotal = 0;
    bool aborted = (st & CSIM_ST_TRAN_NONFINITE) != 0;                 // an instance the reference would have thrown on stays stopped

    const int slowIters = slowStepIters(K.tran_tol, K.tran_alpha, K.tran_max_iters);
    long long sLast = w.d0;
    for (long long s = w.d0 + 1; s <= w.sEnd && !aborted; ++s) {
        sLast = s;
        bool stepKnown = curPiv != nullptr;     // every factorisation of this step on a known sequence?
        bool stepConverged = false;             // a slow step (plan.hpp slowStepIters) is not handed back either
        const long long gstep = a.stepFirst + s;
        terms_step_tran(pl, Pv, T, xp, tran_time(gstep, a.dt), lane);
        wave_sync();
        int it = 0;
        for (int iter = 0; iter < K.tran_max_iters; ++iter) {
            terms_iter_mos(pl, Pv, T, xs, lane);
            wave_sync();
            assemble(pl, T, Gm, lane);                                  // :259-356
            const double xr = lu_solve_wave(Gm, N, LD, K.lu_eps, lane, st, myPivLog, curPiv);   // :359
            if (stepKnown) stepKnown = sequence_is_known(curPiv, a.knownAlts, a.nKnown, N, lane);
            ++it;
            if (!wave_all_finite(xr, N, lane)) {                        // :360-362
                st |= CSIM_ST_TRAN_NONFINITE;
                aborted = true;
                break;
            }
            const double xo = (lane < N) ? xs[lane] : 0.0;
            const double xn = xo + K.tran_alpha * (xr - xo);            // :365
            const double err = norm_in_order(xn - xo, sc, N, lane);     // :366
            if (lane < N) xs[lane] = xn;                                // :367
            wave_sync();
            if (err < K.tran_tol) { stepConverged = it <= slowIters; break; }   // :369-371
            if (iter == K.tran_max_iters - 1) st |= CSIM_ST_TRAN_NONCONV;   // :372-376
        }
        itTotal += it;
        if (a.stepIters && lane == 0) a.stepIters[(s - 1) * (int64_t)B + b] = it;
        if (aborted) break;
        if (lane < N) xp[lane] = xs[lane];                              // :381-417
        wave_sync();
        if (a.wave && (gstep % a.outStride) == 0)                       // :419
            store_probe_row(a.wave, gstep / a.outStride, a.probeEq, a.nProbe, B, b, xs, lane, 64);
        if (stepKnown && stepConverged) break;  // back on a recorded schedule and converging: hand the instance back
    }

    if (lane < N) a.x[(int64_t)lane * B + b] = xs[lane];
    if (lane == 0) {
        a.iters[b] += itTotal;
        a.status[b] |= st;
        step_window_close(a.done, b, a.nSteps, aborted, sLast);
    }
}

// ------------------------------------------------------ stand-alone LU solve
// Solver::solveLinearSystemLU for B systems (include/solver.hpp:83-131)
__global__ void __launch_bounds__(64)
k_lu_solve(int n, int LD, int B, const double* __restrict__ A, const double* __restrict__ rhs,
           double* __restrict__ x, uint32_t* __restrict__ flags, double eps)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const double* Ab = A + (int64_t)b * n * n;
    for (int i = lane; i < n * n; i += 64) sm[(i / n) * LD + (i % n)] = Ab[i];
    if (lane < n) sm[lane * LD + n] = rhs[(int64_t)b * n + lane];
    wave_sync();
    unsigned st = 0;
    const double xv = lu_solve_wave(sm, n, LD, eps, lane, st);
    if (lane < n) x[(int64_t)b * n + lane] = xv;
    if (flags && lane == 0) flags[b] = st;
}

// Solver::luDecompose for B matrices (include/solver.hpp:30-80)
__global__ void __launch_bounds__(64)
k_lu_factor(int n, int LD, int B, const double* __restrict__ A, double* __restrict__ LU,
            int32_t* __restrict__ perm, uint32_t* __restrict__ flags, double eps)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const double* Ab = A + (int64_t)b * n * n;
    for (int i = lane; i < n * n; i += 64) sm[(i / n) * LD + (i % n)] = Ab[i];
    wave_sync();
    int pv = 0;
    const bool ok = lu_factor_wave(sm, n, LD, eps, lane, pv);
    wave_sync();
    for (int i = lane; i < n * n; i += 64) LU[(int64_t)b * n * n + i] = sm[(i / n) * LD + (i % n)];
    if (lane < n) perm[(int64_t)b * n + lane] = pv;
    if (flags && lane == 0) flags[b] = ok ? 0u : CSIM_ST_LU_TINY_PIVOT;
}

// ------------------------------------------------------------------ launchers
hipError_t launchLuFactor(int n, int B, const double* dA, double* dLU, int32_t* dPerm, uint32_t* dFlags,
                          double eps, hipStream_t stream)
{
    const int LD = ldFor(n);
    const size_t lds = sizeof(double) * (size_t)n * (size_t)LD;
    hipLaunchKernelGGL(k_lu_factor, dim3(B), dim3(64), lds, stream, n, LD, B, dA, dLU, dPerm, dFlags, eps);
    return hipGetLastError();
}

// the one place that chooses the shape of a general launch (kernels.hpp)
enum class GenShape { Packed, Wave, Big };
static GenShape shapeFor(const GenPlan& pl, const int32_t* pivLog)
{
    if (!pivLog && packedLanesFor(pl) == 16) return GenShape::Packed;   // the planner keeps the wave per instance
    return pl.N <= 63 ? GenShape::Wave : GenShape::Big;
}

hipError_t launchDcGeneral(const GenPlan& pl, const GenDcArgs& a, hipStream_t stream)
{
    const GenShape shape = shapeFor(pl, a.pivLog);
    if (shape == GenShape::Packed) return launchDcPacked(pl, a, stream);
    if (shape == GenShape::Big) return launchDcBig(pl, a, stream);
    const size_t lds = sizeof(double) * (size_t)ldsLayout(pl.N, pl.LD, pl.nTerms, pl.P).total;
    hipLaunchKernelGGL(k_dc_general, dim3(a.B), dim3(64), lds, stream, pl, a);
    return hipGetLastError();
}

hipError_t launchTranGeneral(const GenPlan& pl, const GenTranArgs& a, hipStream_t stream)
{
    const GenShape shape = shapeFor(pl, a.pivLog);
    if (shape == GenShape::Packed) return launchTranPacked(pl, a, stream);
    if (shape == GenShape::Big) return launchTranBig(pl, a, stream);
    const size_t lds = sizeof(double) * (size_t)ldsLayout(pl.N, pl.LD, pl.nTerms, pl.P).total;
    hipLaunchKernelGGL(k_tran_general, dim3(a.B), dim3(64), lds, stream, pl, a);
    return hipGetLastError();
}

hipError_t launchLuSolve(int n, int B, const double* dA, const double* dRhs, double* dX,
                         uint32_t* dFlags, double eps, hipStream_t stream)
{
    if (n <= 32) return launchLuSolvePacked(n, B, dA, dRhs, dX, dFlags, eps, stream);     // four systems per wave, in registers
    const int LD = ldFor(n);
    const size_t lds = sizeof(double) * (size_t)n * (size_t)LD;
    hipLaunchKernelGGL(k_lu_solve, dim3(B), dim3(64), lds, stream, n, LD, B, dA, dRhs, dX, dFlags, eps);
    return hipGetLastError();
}

} // namespace csim
