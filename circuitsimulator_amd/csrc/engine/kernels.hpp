// kernels.hpp -- host-callable launchers of the HIP kernels (library-private), and the launch idiom of the
// wave-per-workgroup kernels whose dynamic LDS may pass 64 KB (launchWave).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"

namespace csim {

// One 64-lane wavefront per workgroup with ldsBytes of dynamic LDS: above 64 KB the kernel's limit is raised first.
template <class... Params, class... Args>
inline hipError_t launchWave(void (*kernel)(Params...), dim3 grid, size_t ldsBytes, hipStream_t stream, const Args&... args)
{
    if (ldsBytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(64), ldsBytes, stream, args...);
    return hipGetLastError();
}

// The general DC and transient kernels (run-time pivoting, bit-faithful): one record and one launcher per analysis.
// The launcher chooses the shape: four instances per wavefront with the matrix in registers (kernels_packed.hip)
// when no pivot log is asked for and packedLanesFor(pl) == 16, a wavefront per instance with the matrix in LDS up
// to 63 unknowns (kernels_general.hip), the bit-guided global-memory storage beyond that (kernels_big.hip).
// Absent parts stay null or zero.
struct GenDcArgs {
    const double* params;               // [P][B]
    int B;
    double* x;                          // [N][B] operating points
    int32_t* iters;                     // [B] NR passes
    uint32_t* status;                   // [B]
    const uint8_t* only;                // [B] or null: the instances to run (fallback and planner launches)
    int32_t* pivLog;                    // planner log of instance pivInstance (device_common.hpp PIVLOG_*) or null
    int pivInstance;
    double* scratch;                    // N > 63: bigScratchBytesPerInstance(pl) zeroed bytes per instance
};
struct GenTranArgs {
    const double* params;               // [P][B]
    int B;
    double dt;
    long long stepFirst, nSteps;        // steps stepFirst + 1 .. stepFirst + nSteps
    const int32_t* probeEq;             // [nProbe] equations
    int nProbe, outStride;
    double* wave;                       // [rows][nProbe][B] or null
    double* x;                          // [N][B] state, in and out
    long long* iters;                   // [B], added to
    uint32_t* status;                   // [B], OR-ed
    int32_t* stepIters;                 // [nSteps][B] or null
    const uint8_t* only;                // [B] or null: the instances to run (planner launches)
    int32_t* pivLog;                    // planner log of instance pivInstance or null
    int pivInstance;
    int32_t* done;                      // [B] hybrid stepping: steps of this launch completed, or null
    int maxSteps;                       // at most this many further steps per instance (done != null)
    const int32_t* knownAlts;           // [nKnown][N] recorded pivot sequences: hand an instance back once a whole
    int nKnown;                         // step ran on them (N <= 63), or null
    double* scratch;                    // N > 63, as GenDcArgs
};
hipError_t launchDcGeneral(const GenPlan& pl, const GenDcArgs& a, hipStream_t stream);
hipError_t launchTranGeneral(const GenPlan& pl, const GenTranArgs& a, hipStream_t stream);
int packedLanesFor(const GenPlan& pl);  // 16, or 64: N > 32 or four instances with the staged plan do not fit the LDS
size_t bigScratchBytesPerInstance(const GenPlan& pl);
int bigMaxUnknowns();
bool bigSupports(int N, int nTerms, int P);

// stand-alone batched LU (kernels_general.hip; n <= 32: four systems per wavefront, kernels_packed_lu.hip)
hipError_t launchLuSolve(int n, int B, const double* dA, const double* dRhs, double* dX,
                         uint32_t* dFlags, double eps, hipStream_t stream);
hipError_t launchLuFactor(int n, int B, const double* dA, double* dLU, int32_t* dPerm, uint32_t* dFlags,
                          double eps, hipStream_t stream);
hipError_t launchLuSolvePacked(int n, int B, const double* dA, const double* dRhs, double* dX, uint32_t* dFlags, double eps,
                               hipStream_t stream);

// dense stand-alone LU for 64 <= n <= 1024, one workgroup per system, in place (kernels_dense.hip)
hipError_t launchLuSolveDense(int n, int B, double* dWork, const double* dRhs, double* dX, uint32_t* dFlags,
                              double eps, hipStream_t stream);
hipError_t launchLuFactorDense(int n, int B, double* dLU, int32_t* dPerm, uint32_t* dFlags, double eps,
                               hipStream_t stream);

// Gauss-Seidel solver and the DC operating point built on it (kernels_gs.hip)
hipError_t launchGsSolve(int n, int B, const double* dAt /*[n*n][B]*/, const double* dRhs /*[n][B]*/,
                         const double* dX0 /*[n][B] or null*/, int maxIters, double tol, double* dX /*[n][B]*/,
                         double* dXold /*[n][B] scratch*/, int32_t* dSweeps, hipStream_t stream);
hipError_t launchDcGs(const GenPlan& pl, const int32_t* dRowPtr, const int32_t* dRowCol, const double* dParams, int B,
                      double* dX, int32_t* dIters, uint32_t* dStatus, hipStream_t stream);

// near-threshold verification of the fast generated kernels (kernels_verify.hip)
hipError_t launchNearPrep(int B, int N, long long nSteps, const int32_t* dNearStep, const double* dNearX, double* dVerX,
                          int32_t* dVerDone, long long* dVerIters, uint32_t* dVerStatus, unsigned char* dVerFallback,
                          hipStream_t stream);
hipError_t launchNearResolve(int B, int N, int32_t* dNearStep, const int32_t* dNearIt, const long long* dNearItAfter,
                             const double* dNearX, const int32_t* dVerDone, const long long* dVerIters, double* dX,
                             int32_t* dDone, long long* dIters, unsigned char* dFallback, int32_t* dFlags,
                             bool forceMismatch, hipStream_t stream);

// Monte-Carlo parameter table (mc.hip)
hipError_t launchMcParams(int P, int B, long long bFirst, uint64_t seed, double sigma,
                          const int32_t* dKind, const double* dNominal, const double* dMu,
                          const double* dCox, const double* dW, const double* dL,
                          double* dParams, hipStream_t stream);

// AC small-signal analysis (kernels_ac.hip).  System of one instance (acSystemDoubles(N) doubles): G and C
// column-major [N][N], J re [N], J im [N].  Instances b0 .. b0+Bc-1 of a batch of B; dSys holds Bc systems.
// AC_KERNEL_BLOCK is opt-in: one 256-thread workgroup per system, N <= 1024, AC and noise only; its matrix lives in a
// scratch of acBlockWorkDoubles(N) doubles per chunk instance (dWork).  The value 3 stays an invalid selector.
enum { AC_KERNEL_AUTO = 0, AC_KERNEL_WAVE = 1, AC_KERNEL_PACKED = 2, AC_KERNEL_BLOCK = 4 };
size_t acSystemDoubles(int N);
size_t acBlockWorkDoubles(int N);
// which == AC_KERNEL_BLOCK: the assembly that scatters straight to global memory (any N the engine accepts)
hipError_t launchAcAssemble(const GenPlan& pl, const double* dAcRe, const double* dAcIm, const double* dParams, int B,
                            int b0, int Bc, const double* dXop, double* dSys, hipStream_t stream,
                            int which = AC_KERNEL_AUTO);
// the sweep on the systems launchAcAssemble leaves (host side only: the kernels take these one by one)
struct AcArgs {
    int N, F, B, b0, Bc;
    int nProbe;
    double eps;
    const double* sys;
    const double* omega;
    const int32_t* probe;               // [nProbe] equations, or null = every unknown (nProbe = N)
    double* out;                        // [F][nProbe][B] complex (re, im)
    uint32_t* status;                   // [B], OR-ed
    double* work;                       // AC_KERNEL_BLOCK: acBlockWorkDoubles(N) doubles per chunk instance
};
hipError_t launchAcSweep(int which, const AcArgs& a, hipStream_t stream);

// Noise analysis (kernels_noise.hip) on the systems launchAcAssemble leaves.  Generator s of chunk instance c has
// its PSD at psd[s * psdStride + psdOff + c].  Equation indices are checked by the callers: they index LDS.
struct NoiseArgs {
    int N, F, S, B, b0, Bc;
    int outP, outM;                     // d = +1 at outP, -1 at outM (-1: ground)
    int inKind, inA, inB;               // ac_noise.hpp NOISE_IN_*
    double eps;
    const double* sys;
    const double* omega;
    const int32_t *srcA, *srcB;         // [S] generator terminals (equations, -1 ground)
    const double* psd;
    size_t psdStride, psdOff;
    double* onoise;                     // [F][B]
    double* gain;                       // [F][B] complex or null
    double* contrib;                    // [F][S][B] or null
    double* y;                          // [F][N][B] complex or null: the adjoint solution
    uint32_t* status;                   // [B], OR-ed
    double* work;                       // AC_KERNEL_BLOCK: acBlockWorkDoubles(N) doubles per chunk instance
};
hipError_t launchNoisePsd(const GenPlan& pl, const int32_t* dSrcElem, int S, const double* dParams, int B, int b0, int Bc,
                          const double* dXop, double kT4, double* dPsd, size_t psdStride, size_t psdOff, hipStream_t stream);
hipError_t launchNoiseSweep(int which, const NoiseArgs& a, hipStream_t stream);

// S-parameter analysis (kernels_sp.hip) on the systems launchAcAssemble leaves: one factorisation with K right-hand
// sides per (instance, frequency).  P = K > 0: unit right-hand sides at portEq, Y (and S) formed on the device.
// P = 0: the right-hand sides are given and only the solutions are stored (the engine-free test entry).
struct SpArgs {
    int N, K, P, F, B, b0, Bc;
    int32_t portEq[4];                  // branch equations of the ports; checked by the launcher: they index LDS
    double sz[4];                       // sqrt(Z0) of the ports
    double eps;
    const double* sys;
    const double* omega;
    const double* rhs;                  // [Bc][K][N] complex (P == 0)
    double* x;                          // [F][K][N][B] complex or null (required when P == 0)
    double* y;                          // [F][P][P][B] complex (P > 0)
    double* s;                          // [F][P][P][B] complex or null
    uint32_t* status;                   // [B], OR-ed
};
hipError_t launchSpSweep(int which, const SpArgs& a, hipStream_t stream);

// Two-port noise analysis (kernels_spnoise.hip) on the systems launchAcAssemble leaves: one factorisation of A^T with
// one adjoint right-hand side per port and (instance, frequency), Y and Cy from its solutions.  Generators and their
// PSDs as NoiseArgs.  Port equations are checked by the launcher, generator terminals by the callers: they index LDS.
struct SpNoiseArgs {
    int N, P, F, S, B, b0, Bc;
    int32_t portEq[4];                  // branch equations of the ports
    double eps;
    double kT40, gs;                    // 4 k 290 and 1 / Z0 of port 1 (noise parameters, P == 2)
    const double* sys;
    const double* omega;
    const int32_t *srcA, *srcB;         // [S] generator terminals (equations, -1 ground)
    const double* psd;
    size_t psdStride, psdOff;
    double* y;                          // [F][P][P][B] complex or null
    double* cy;                         // [F][P][P][B] complex
    double *nf, *fmin, *rn;             // [F][B] or null (P == 2)
    double* yopt;                       // [F][B] complex or null (P == 2)
    double* x;                          // [F][P][N][B] complex or null: the adjoint solutions
    uint32_t* status;                   // [B], OR-ed
};
hipError_t launchSpNoiseSweep(int which, const SpNoiseArgs& a, hipStream_t stream);

// Distortion (kernels_disto.hip) and intermodulation analysis (kernels_imd.hip) on the systems launchAcAssemble leaves:
// a chain of dependent factorisations per (instance, point), each after the first ones with a right-hand side of MOSFET
// mixing currents of earlier solutions (ac_chain.hpp).  Distortion: three, at w, 2 w and 3 w (ac_disto.hpp), one tone.
// Intermodulation: six, at w1, w2, w1 + w2, w1 - w2, 2 w1 and 2 w1 - w2 (ac_imd.hpp), two tones.  Coefficient k of
// device m of chunk instance c is at coef[(m * 7 + k) * coefStride + coefOff + c].  The output pair and the device
// terminals (hostD, hostG, hostS: the host's copy of the table) are checked by the launchers: they index LDS.  Wave and
// packed shapes only.
struct ChainArgs {
    int N, F, M, B, b0, Bc;
    int outP, outM;                     // v = x[outP] - x[outM] (-1: ground)
    double eps;
    const double* sys;
    const double* omega;                // [F] the tone, or the first of two
    const double* omega2;               // [F] second tone; one tone: null, never read
    const double* j2;                   // two tones: [Bc][2 N] (re [N], im [N]) excitation of the second, or null: that of the first
    const int32_t *devD, *devG, *devS;  // [M] drain, gate, source equations (-1 ground)
    const double* coef;
    size_t coefStride, coefOff;
    double* h;                          // [F][solves][N][B] complex or null: x1, x2, x3, or x0 .. x5
    double* ratio;                      // [F][2][B]: HD2, HD3, or [F][3][B]: IM2+, IM2-, IM3
    uint32_t* status;                   // [B], OR-ed
};
hipError_t launchDistoCoef(const GenPlan& pl, const int32_t* dDevElem, int M, const double* dParams, int B, int b0, int Bc,
                           const double* dXop, double* dCoef, size_t coefStride, size_t coefOff, hipStream_t stream);
hipError_t launchDistoSweep(int which, const ChainArgs& a, const int32_t* hostD, const int32_t* hostG, const int32_t* hostS,
                            hipStream_t stream);
hipError_t launchImdSweep(int which, const ChainArgs& a, const int32_t* hostD, const int32_t* hostG, const int32_t* hostS,
                          hipStream_t stream);

// Loop-gain analysis (kernels_stb.hip) on the systems launchAcAssemble leaves (their J is not read): one factorisation
// with two right-hand sides per (instance, frequency), T formed on the device.  The probe's equations are checked by
// the launcher: they index LDS.  Wave and packed shapes only.
struct StbArgs {
    int N, F, B, b0, Bc;
    int eqP, eqM, eqBr;                 // the probe: + node (drives), - node (receives), branch equation
    double eps;
    const double* sys;
    const double* omega;
    double* t;                          // [F][B] complex: the loop gain
    double* x;                          // [F][2][N][B] complex or null: the two solutions
    uint32_t* status;                   // [B], OR-ed
};
hipError_t launchStbSweep(int which, const StbArgs& a, hipStream_t stream);
// the margins of B instances from t [F][B] complex at freqs [F] (Hz, on the device): margins [4][B] = PM, fc, GM, f180;
// found [B] or null
hipError_t launchStbMargins(int F, int B, const double* dFreqs, const double* dT, double* dMargins, int32_t* dFound,
                            hipStream_t stream);

// Pole analysis (kernels_pz.hip) on the systems launchAcAssemble leaves (their J is not read): per instance the
// eigenvalues of -(G + sigma0 C)^-1 C, the cut at wmax, the ordered poles and their summary.  One wave per instance,
// N <= 63 (checked by the launcher: N sizes the LDS).
struct PzArgs {
    int N, B, b0, Bc;
    double eps, sigma0, wmax;
    const double* sys;
    double* poles;                      // [N][B] complex: slot k of instance b
    int32_t* nPoles;                    // [B]
    int32_t* nRhp;                      // [B]
    double* maxRe;                      // [B]
    uint32_t* status;                   // [B], OR-ed
};
size_t pzLdsBytes(int N);
hipError_t launchPz(const PzArgs& a, hipStream_t stream);

// Periodic steady state (kernels_pss.hip): one shooting round of chunk instances b0 .. b0+Bc-1 of a batch of B -- the
// period kernel (K steps of the general transient from x0, the sensitivity W_K, the harmonics of the probes), then the
// update kernel (closure test, x0 += (I - W_K)^-1 (x_K - x0)).  Probe equations are checked by the caller: they index LDS.
struct PssArgs {
    const double* params;               // [P][B]
    int B, b0, Bc;
    double dt;
    int K, H;                           // steps per period, highest harmonic
    const int32_t* probeEq;             // [nProbe] equations, or null = every unknown (nProbe = N)
    int nProbe;
    const double *twc, *tws;            // [K] cos and sin of 2 pi j / K
    double tol;
    int maxRounds;
    double* x0;                         // [N][B] in: start of the round, out: updated
    double* xK;                         // [N][B] scratch: the state after the period
    double* harm;                       // [H+1][nProbe][B] complex: the harmonics of this round's period
    double* W;                          // [Bc][N][N] scratch: W_K
    int32_t* rounds;                    // [B] rounds used
    uint32_t* status;                   // [B], OR-ed
    int32_t* done;                      // [B] 0 while an instance is still shooting
    int32_t* unfinished;                // one counter: instances that go on to another round, added to
};
hipError_t launchPssRound(const GenPlan& pl, const PssArgs& a, hipStream_t stream);
// the period kernel alone (no update): x_K and W_K of the period that starts at x0; H = 0 and nProbe = 0 store no harmonics
hipError_t launchPssPeriod(const GenPlan& pl, const PssArgs& a, hipStream_t stream);
size_t pssLdsBytes(const GenPlan& pl);

// Periodic AC analysis (kernels_pac.hip) of chunk instances b0 .. b0+Bc-1 of a batch of B at Fc <= 32 frequencies:
// the period kernel integrates the orbit from x0 as the periodic steady state does and carries the Fc complex
// perturbations p_k as 2 Fc real columns (re at 2 f, im at 2 f + 1) through J_k p_k = z (Hm p_{k-1}) + u; the close
// kernel (PeriodCloseArgs below) solves (I - z_K W_K) p_0 = r_K per (instance, frequency).  One launch of the period
// kernel with p0 == null (p_0 = 0, leaves r_K), the close kernel, a second launch from that p_0 with out != null (the
// sideband sums).
// Probe equations are checked by the caller: they index LDS.
struct PacArgs {
    const double* params;               // [P][B]
    int B, b0, Bc;
    double dt;
    int K, M;                           // steps per period, sidebands -M .. M
    int Fc, fFirst, F;                  // frequencies of this launch, the first one's index among the F of the call
    const int32_t* probeEq;             // [nProbe] equations, or null = every unknown (nProbe = N)
    int nProbe;
    const double *twc, *tws;            // [K] cos and sin of 2 pi j / K
    const double *acRe, *acIm;          // [nElem] the AC excitation of the sources
    const double *zr, *zi;              // [Fc] z of this launch's frequencies
    const double* x0;                   // [N][B] start of the period, not modified
    const uint32_t* wStatus;            // [B] status of the launch that made W_K
    const double* p0;                   // [Bc][N][2 Fc] start of the recursion, or null = zero
    double* pK;                         // [Bc][N][2 Fc]: period kernel p_K out; close kernel r_K in, p_0 out (in place)
    double* out;                        // [F][2 M + 1][nProbe][B] complex or null: the sideband transfers
    int32_t* stop;                      // [Bc] scratch, zeroed per frequency chunk: instances that stopped
    uint32_t* status;                   // [B], OR-ed
};
// bytes of dynamic LDS of the period kernel at Fc frequencies; pacMaxFc: the largest Fc <= 32 that fits, 0 = none
size_t pacLdsBytes(const GenPlan& pl, int Fc, int M, int nProbe);
int pacMaxFc(const GenPlan& pl, int M, int nProbe);
hipError_t launchPacPeriod(const GenPlan& pl, const PacArgs& a, hipStream_t stream);

// The closure of the periodic AC and the periodic noise analysis (k_period_close, kernels_pac.hip), one wavefront per
// (chunk instance, frequency): (I - z_K W_K) v = v in place, W_K read transposed for the adjoint (periodic noise).  A
// singular closure stops the instance: stop[c] = 1, CSIM_ST_PAC_SINGULAR | CSIM_ST_LU_TINY_PIVOT into its status.
struct PeriodCloseArgs {
    int b0, Bc, Fc;
    const double* W;                    // [Bc][N][N] W_K
    const double *zKr, *zKi;            // [Fc] z_K of this launch's frequencies
    double* v;                          // [Bc][N][2 Fc]: the right-hand sides in, the solutions out
    int32_t* stop;                      // [Bc]: stopped instances are skipped
    uint32_t* status;                   // [B], OR-ed
    bool transposeW;
};
hipError_t launchPeriodClose(const GenPlan& pl, const PeriodCloseArgs& a, hipStream_t stream);

// Periodic noise analysis (kernels_pnoise.hip) of chunk instances b0 .. b0+Bc-1 of a batch of B at Fc <= 32 output
// frequencies.  The orbit kernel integrates the period from x0 as the periodic steady state does and stores every
// converged state; the period kernel walks the stored orbit backwards, k = K .. 1, and carries the Fc complex adjoint
// vectors as 2 Fc real columns (re at 2 f, im at 2 f + 1) through J_k^T q_k = z g_k + d, g_{k-1} = Hm^T q_k; the close
// kernel (PeriodCloseArgs, transposeW) solves (I - z_K W_K^T) g_K = r per (instance, frequency).  One launch of the period kernel with g0 == null
// (g_K = 0, leaves r in gK), the close kernel, a second launch with g0 == gK, which adds the transfer sums and stores
// the outputs.  Generator S (one past the noise generators) is the input source with sigma = 1.  Output, input and
// generator equations are checked by the caller: they index LDS.
struct PnoiseArgs {
    const double* params;               // [P][B]
    int B, b0, Bc;
    double dt;
    int K, M;                           // steps per period, sidebands -M .. M
    int Fc, fFirst, F;                  // frequencies of this launch, the first one's index among the F of the call
    const double *twc, *tws;            // [K] cos and sin of 2 pi j / K
    const double *zr, *zi;              // [Fc] z of this launch's frequencies
    const double* x0;                   // [N][B] start of the period, not modified (orbit kernel)
    double* orbit;                      // [Bc][K][N]: x_1 .. x_K of every chunk instance
    const uint32_t* wStatus;            // [B] status of the launch that made W_K (orbit kernel)
    int outP, outM;                     // d = +1 at outP, -1 at outM (-1: ground)
    int S;                              // noise generators
    const int32_t *srcElem, *srcA, *srcB;   // [S] element and equations of every generator
    int inA, inB;                       // the input source's unit excitation: q(inA) - q(inB), -1 = none / ground
    double kT4;
    const double* g0;                   // [Bc][N][2 Fc] start of the recursion, or null = zero (the first pass)
    double* gK;                         // [Bc][N][2 Fc]: period kernel r out; close kernel r in, g_K out (in place)
    double* onoise;                     // [F][B]
    double* gain;                       // [F][2 M + 1][B] complex, or null
    double* contrib;                    // [F][S][B], or null
    double* side;                       // [F][2 M + 1][B], or null
    int32_t* orbitStop;                 // [Bc]: instances the orbit kernel stopped
    int32_t* stop;                      // [Bc] scratch, zeroed per frequency chunk: instances that stopped
    uint32_t* status;                   // [B], OR-ed
};
// bytes of dynamic LDS of the period kernel at Fc frequencies; pnoiseMaxFc: the largest Fc <= 32 that fits, 0 = none
size_t pnoiseLdsBytes(const GenPlan& pl, int Fc, int M, int S);
int pnoiseMaxFc(const GenPlan& pl, int M, int S);
hipError_t launchPnoiseOrbit(const GenPlan& pl, const PnoiseArgs& a, hipStream_t stream);
hipError_t launchPnoisePeriod(const GenPlan& pl, const PnoiseArgs& a, hipStream_t stream);

// layout helpers (transpose.hip): [rows][cols] <-> [cols][rows] of doubles
hipError_t launchTranspose(const double* dIn, double* dOut, int rows, int cols, hipStream_t stream);

} // namespace csim
