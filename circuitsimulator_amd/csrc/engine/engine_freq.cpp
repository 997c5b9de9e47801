// engine_freq.cpp -- C-ABI of the frequency-domain analyses: AC, noise, S-parameters, two-port noise, distortion,
// intermodulation, loop gain and poles, each as csim_*_batch_dev (device pointers, enqueue only), csim_*_batch (host pointers, DC operating point
// included) and csim_*_solve_batch (any system, no engine).  What they share is written once: kernel choice, the chunk
// driver, scratch growth, the card's frequencies, the operating point and the output list of the host-pointer forms.
// A new analysis supplies its setup function, its ...Args and its sweep launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <deque>
#include <string>
#include <vector>

#include "ac_disto.hpp"
#include "ac_imd.hpp"
#include "ac_noise.hpp"
#include "ac_port.hpp"
#include "ac_stb.hpp"
#include "csim.h"
#include "engine_host.hpp"
#include "kernels.hpp"
#include "pz.hpp"

using csim::setError;

namespace {

constexpr double FOUR_K_B = 4.0 * 1.380649e-23;         // J/K: a generator's PSD is FOUR_K_B * T * (its conductance)

// ---- what a call may ask for --------------------------------------------------

// the system of every instance lives in device scratch between assembly and sweep; instances are processed in
// chunks that keep it below 256 MiB; under ac_kernel=block the planes of the solve live there too, and a chunk may
// shrink to 32 instances (the planes of a 1024-unknown system are 16 MiB)
bool acBlock(const csim_engine* eng) { return eng->cfg.acKernel == csim::AC_KERNEL_BLOCK; }

int acChunk(const csim_engine* eng, int B)
{
    return (int)std::min<size_t>((size_t)B, csim::acChunkCap(eng));
}

// the sizes the frequency-domain analyses cover: 63 unknowns, or with ac_kernel=block (AC and noise) 1024
int acSizeCheck(const csim_engine* eng, const char* what)
{
    const int limit = acBlock(eng) ? 1024 : 63;
    if (eng->plan.N <= limit) return CSIM_OK;
    setError(std::string(what) + " covers circuits of up to " + std::to_string(limit) + " unknowns");
    return CSIM_ERR_UNSUPPORTED;
}

// the block kernel carries one right-hand side: the port analyses have none for it yet
int acBlockRefused(const csim_engine* eng, const char* what)
{
    if (!acBlock(eng)) return CSIM_OK;
    setError(std::string(what) + ": ac_kernel=block covers AC and noise analysis only");
    return CSIM_ERR_UNSUPPORTED;
}

int acCheck(const csim_engine* eng)
{
    if (const int rc = acSizeCheck(eng, "AC analysis")) return rc;
    if (!eng->acAnySource) { setError("AC analysis: no source carries an AC magnitude (V/I ... AC mag [phase])"); return CSIM_ERR_CONFIG; }
    return CSIM_OK;
}

// the sweep kernel of a call.  auto: register-resident (packed) up to 32 unknowns, one wave per system beyond; the
// block kernel is opt-in and stays as requested.  `who` names an engine-free entry in the refusal, null an engine's.
int acPickKernel(int requested, int N, const char* who, int* which)
{
    *which = requested != csim::AC_KERNEL_AUTO ? requested : (N <= 32 ? csim::AC_KERNEL_PACKED : csim::AC_KERNEL_WAVE);
    if (*which == csim::AC_KERNEL_PACKED && N > 32) {
        setError(who ? std::string(who) + ": the packed kernel covers n <= 32" : std::string("ac_kernel=packed covers N <= 32"));
        return CSIM_ERR_UNSUPPORTED;
    }
    return CSIM_OK;
}

// T in kelvin -> 4 k_B T
int noiseTemperature(double temp_k, const char* who, double* kT4)
{
    if (!(temp_k > 0.0) || !std::isfinite(temp_k)) {
        setError(std::string(who) + ": the temperature must be positive and finite (kelvin)");
        return CSIM_ERR_CONFIG;
    }
    *kT4 = FOUR_K_B * temp_k;
    return CSIM_OK;
}

// no frequency list given: the sweep of the netlist's card
int cardFreqs(const csim::SweepGrid& g, const char* who, const char* cardName, std::vector<double>& card,
              const double** freqs, int32_t* F)
{
    if (!g.enabled) {
        setError(std::string(who) + ": no frequencies given and the netlist has no " + cardName + " card");
        return CSIM_ERR_CONFIG;
    }
    const int64_t n = csim_ac_num_freqs(g.sweep, g.points, g.fstart, g.fstop);
    if (n < 0) return static_cast<int>(n);
    card.resize((size_t)n);
    if (const int rc = csim_ac_freqs(g.sweep, g.points, g.fstart, g.fstop, card.data())) return rc;
    *freqs = card.data();
    *F = static_cast<int32_t>(n);
    return CSIM_OK;
}

// ---- device tables and scratch of the sweeps -----------------------------------

// A new frequency or probe list for the sweeps: into a slot no enqueued sweep still reads (never the current one,
// which the previous call's kernels may be using), with a synchronous copy -- complete before the caller's next
// launch, whatever its stream.  The ring grows only while more than its size of distinct lists are in flight;
// at AC_MAX_SLOTS the oldest reader is waited for (that event alone, not the device).
constexpr size_t AC_MAX_SLOTS = 8;
int acUpload(std::vector<csim_engine::AcList>& ring, int& cur, const void* src, size_t bytes)
{
    int slot = -1;
    for (size_t i = 0; i < ring.size() && slot < 0; ++i) {
        if ((int)i == cur) continue;
        const hipError_t q = hipEventQuery(ring[i].done);
        if (q == hipSuccess) slot = (int)i;
        else if (q != hipErrorNotReady) HIPCHK(q);
    }
    (void)hipGetLastError();                     // "not ready" is an answer here, not an error for the next launch check
    if (slot < 0 && ring.size() < AC_MAX_SLOTS) {
        ring.emplace_back();
        slot = (int)ring.size() - 1;
        HIPCHK(hipEventCreateWithFlags(&ring[(size_t)slot].done, hipEventDisableTiming));
    }
    if (slot < 0) {
        slot = (cur + 1) % (int)ring.size();
        HIPCHK(hipEventSynchronize(ring[(size_t)slot].done));
    }
    csim_engine::AcList& s = ring[(size_t)slot];
    if (s.cap < bytes) {
        if (s.d) HIPCHK(hipFree(s.d));
        s.d = nullptr;
        s.cap = 0;
        HIPCHK(hipMalloc(&s.d, bytes));
        s.cap = bytes;
    }
    HIPCHK(hipMemcpy(s.d, src, bytes, hipMemcpyHostToDevice));
    cur = slot;
    return CSIM_OK;
}

// w = 2 pi f of a sweep's frequency list on the device: uploaded when the list changes, cached otherwise
int acOmega(csim_engine* eng, const double* freqs, int F, const double** dOmega)
{
    std::vector<double> omega((size_t)F);
    for (int f = 0; f < F; ++f) omega[(size_t)f] = 2.0 * eng->cir.ir.k.pi * freqs[f];
    if (eng->acOmegaCur < 0 || omega != eng->acOmegaCache) {
        eng->acOmegaCache.clear();
        if (const int rc = acUpload(eng->acOmegaSlots, eng->acOmegaCur, omega.data(), sizeof(double) * (size_t)F)) return rc;
        eng->acOmegaCache = omega;
    }
    *dOmega = static_cast<const double*>(eng->acOmegaSlots[(size_t)eng->acOmegaCur].d);
    return CSIM_OK;
}

// one of the engine's scratch areas, grown to `want` units (it never shrinks)
template <class Cap>
int growDevice(double*& d, Cap& cap, size_t want, size_t bytesPerUnit)
{
    if ((size_t)cap >= want) return CSIM_OK;
    if (d) HIPCHK(hipFree(d));
    d = nullptr;
    cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&d), bytesPerUnit * want));
    cap = (Cap)want;
    return CSIM_OK;
}

// the fields every ...Args carries under the same name
template <class Args>
void acCommonArgs(Args& a, int N, int F, int B, int b0, int Bc, double eps, const double* sys, const double* omega,
                  uint32_t* status)
{
    a.N = N; a.F = F; a.B = B; a.b0 = b0; a.Bc = Bc;
    a.eps = eps;
    a.sys = sys;
    a.omega = omega;
    a.status = status;
}

// where a noise sweep's generator PSDs go: the caller's [S][B] table, or (null) the engine's scratch of one chunk
struct PsdTarget {
    double kT4;
    double* user;
};

// The part of a csim_*_batch_dev call that no analysis owns: the angular frequencies, the chunk size and the scratch
// of a chunk; then per chunk the assembly of the systems, with `psd` the generator PSDs, and the caller's sweep
// (`a` holds the chunk, the scratch exists; PSD table, stride and offset are handed over); at the end the event
// that says when the frequency list's slot is free again.
template <class Args, class Sweep>
int acSweepChunks(csim_engine* eng, const double* d_params, int B, const double* d_xop, const double* freqs, int F, int which,
                  hipStream_t hs, const PsdTarget* psd, uint32_t* d_status, Args& a, Sweep sweep)
{
    const int N = eng->plan.N, S = eng->nNoiseSrc;
    const double* dOmega = nullptr;
    if (const int rc = acOmega(eng, freqs, F, &dOmega)) return rc;
    const int chunk = acChunk(eng, B);
    if (const int rc = growDevice(eng->dAcSys, eng->acSysCap, (size_t)chunk, sizeof(double) * csim::acSystemDoubles(N))) return rc;
    if (acBlock(eng))
        if (const int rc = growDevice(eng->dAcWork, eng->acWorkCap, (size_t)chunk, sizeof(double) * csim::acBlockWorkDoubles(N))) return rc;
    const bool ownPsd = psd && !psd->user;
    if (ownPsd)
        if (const int rc = growDevice(eng->dNoisePsd, eng->noisePsdCap, (size_t)S * (size_t)chunk, sizeof(double))) return rc;
    double* const dPsd = !psd ? nullptr : (ownPsd ? eng->dNoisePsd : psd->user);
    const size_t psdStride = ownPsd ? (size_t)chunk : (size_t)B;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int Bc = std::min(chunk, B - b0);
        const size_t psdOff = ownPsd ? 0 : (size_t)b0;
        acCommonArgs(a, N, F, B, b0, Bc, eng->cir.ir.k.lu_eps, eng->dAcSys, dOmega, d_status);
        HIPCHK(csim::launchAcAssemble(eng->gpTran, eng->dAcRe, eng->dAcIm, d_params, B, b0, Bc, d_xop, eng->dAcSys, hs, which));
        if (psd)
            HIPCHK(csim::launchNoisePsd(eng->gpTran, eng->dNoiseElem, S, d_params, B, b0, Bc, d_xop, psd->kT4, dPsd, psdStride,
                                        psdOff, hs));
        HIPCHK(sweep(dPsd, psdStride, psdOff));
    }
    HIPCHK(hipEventRecord(eng->acOmegaSlots[(size_t)eng->acOmegaCur].done, hs));
    return CSIM_OK;
}

// ---- host-pointer forms --------------------------------------------------------

// [F][X][B] on the device, W doubles per entry (1: real, 2: complex) -> [B][F][X] on the host
int toHost(const double* dSrc, int F, int X, int B, int W, double* dst)
{
    const size_t n = (size_t)W * F * X * B;
    if (n == 0) return CSIM_OK;
    std::vector<double> h(n);
    HIPCHK(hipMemcpy(h.data(), dSrc, sizeof(double) * n, hipMemcpyDeviceToHost));
    for (int f = 0; f < F; ++f)
        for (int t = 0; t < X; ++t)
            for (int b = 0; b < B; ++b) {
                const size_t src = (((size_t)f * X + t) * B + b) * W;
                const size_t at = (((size_t)b * F + f) * X + t) * W;
                for (int k = 0; k < W; ++k) dst[at + k] = h[src + k];
            }
    return CSIM_OK;
}

// The outputs of a host-pointer call.  add() names one: [B][F][X] at the caller's, W doubles per entry, and gives the
// device buffer the kernels fill ([F][X][B]), or null when the caller does not want it (a null host pointer).
// A failed allocation shows in rc, to be looked at once after the last add().
struct HostOutputs {
    struct Out { DevBuf d; double* host; int F, X, W; };
    const int F, B;
    int rc = CSIM_OK;
    std::deque<Out> outs;              // a deque: a DevBuf stays where it was made

    HostOutputs(int F_, int B_) : F(F_), B(B_) {}
    double* add(double* host, int X, int W, bool zeroed = false, bool perInstance = false)   // perInstance: [X][B] -> [B][X]
    {
        if (!host || rc) return nullptr;
        Out& o = outs.emplace_back();
        o.host = host; o.F = perInstance ? 1 : F; o.X = X; o.W = W;
        const size_t bytes = sizeof(double) * (size_t)W * o.F * X * B;
        rc = [&]() -> int {
            HIPCHK(o.d.alloc(bytes));
            if (zeroed) HIPCHK(hipMemset(o.d.p, 0, bytes));
            return CSIM_OK;
        }();
        return o.d.as<double>();
    }
    // after the sweeps: wait, then every output and the status words ([B] at dStatus) go home
    int finish(DevBuf& dStatus, uint32_t* status)
    {
        HIPCHK(hipDeviceSynchronize());
        for (Out& o : outs)
            if (const int frc = toHost(o.d.as<double>(), o.F, o.X, B, o.W, o.host)) return frc;
        if (status) HIPCHK(hipMemcpy(status, dStatus.p, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost));
        return CSIM_OK;
    }
};

// the DC operating point every csim_*_batch call starts from, and the buffers it leaves on the device
struct OpPoint {
    DevBuf params, x, iters, status;
};
int opPointSolve(csim_engine* eng, const double* params, int B, const HostOutputs& outs, OpPoint& op)
{
    if (outs.rc) return outs.rc;
    if (const int rc = csim::stageParams(eng, params, B, op.params)) return rc;
    HIPCHK(op.x.alloc(sizeof(double) * (size_t)eng->plan.N * B));
    HIPCHK(op.iters.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(op.status.alloc(sizeof(uint32_t) * (size_t)B));
    return csim_dc_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), op.iters.as<int32_t>(), op.status.as<uint32_t>(),
                             nullptr);
}

// ---- the analyses' setup -------------------------------------------------------

// output pair, input source and temperature of a noise call -> the kernels' numbers
int noiseSetup(const csim_engine* eng, int out_p, int out_m, int src_elem, double temp_k, csim::NoiseArgs& a, double& kT4)
{
    const int N = eng->plan.N;
    if (const int rc = acSizeCheck(eng, "noise analysis")) return rc;
    if (out_p < 0 || out_p >= N || out_m < -1 || out_m >= N || out_p == out_m) {
        setError("noise analysis: the output needs two different equations, out_p >= 0 (out_m = -1: ground)");
        return CSIM_ERR_ARG;
    }
    a.inKind = csim::NOISE_IN_NONE;
    a.inA = a.inB = -1;
    if (src_elem >= 0) {
        const csim::CircuitIR& c = eng->cir;
        if (src_elem >= c.ir.n_elems) { setError("noise analysis: bad input source element"); return CSIM_ERR_ARG; }
        const int kind = c.kind[(size_t)src_elem];
        if (kind == CSIM_V) {
            a.inKind = csim::NOISE_IN_V;
            a.inA = c.branchEq[(size_t)src_elem];
            if (a.inA < 0 || a.inA >= N) { setError("noise analysis: the input source has no branch equation"); return CSIM_ERR_ARG; }
        } else if (kind == CSIM_I) {                         // stampAC: J(p) -= I, J(m) += I (element.cpp:68-81)
            a.inKind = csim::NOISE_IN_I;
            a.inA = c.eq[4 * (size_t)src_elem + 1];
            a.inB = c.eq[4 * (size_t)src_elem + 0];
        } else { setError("noise analysis: the input source must be a V or I element"); return CSIM_ERR_ARG; }
    }
    if (const int rc = noiseTemperature(temp_k, "noise analysis", &kT4)) return rc;
    a.outP = out_p;
    a.outM = out_m;
    a.S = eng->nNoiseSrc;
    a.srcA = eng->dNoiseA;
    a.srcB = eng->dNoiseB;
    return CSIM_OK;
}

// the engine's ports -> the kernels' numbers (include/csim.h "S-parameter analysis")
int spSetup(const csim_engine* eng, csim::SpArgs& a)
{
    const int N = eng->plan.N;
    if (const int rc = acBlockRefused(eng, "S-parameter and two-port noise analysis")) return rc;
    if (!eng->spPortError.empty()) { setError(eng->spPortError); return CSIM_ERR_CONFIG; }
    const int P = (int)eng->spPortEq.size();
    if (P == 0) { setError("S-parameter analysis: the netlist declares no port (V ... PORTNUM k [Z0 r])"); return CSIM_ERR_CONFIG; }
    if (N > 63) { setError("S-parameter analysis covers circuits of up to 63 unknowns"); return CSIM_ERR_UNSUPPORTED; }
    a.K = a.P = P;
    for (int i = 0; i < P; ++i) {
        a.portEq[i] = eng->spPortEq[(size_t)i];
        a.sz[i] = std::sqrt(eng->spZ0[(size_t)i]);
        if (a.portEq[i] < 0 || a.portEq[i] >= N) { setError("S-parameter analysis: a port has no branch equation"); return CSIM_ERR_ARG; }
    }
    return CSIM_OK;
}

// the engine's ports, the temperature and the wish for noise parameters -> the kernels' numbers (include/csim.h
// "Two-port noise analysis"); port and size errors are those of the S-parameter analysis
int spNoiseSetup(const csim_engine* eng, double temp_k, bool wantParams, csim::SpNoiseArgs& a, double& kT4)
{
    csim::SpArgs sp{};
    if (const int rc = spSetup(eng, sp)) return rc;
    if (wantParams && sp.P != 2) { setError("two-port noise analysis: NF, Fmin, Rn and Yopt exist for two ports only"); return CSIM_ERR_CONFIG; }
    if (const int rc = noiseTemperature(temp_k, "two-port noise analysis", &kT4)) return rc;
    a.P = sp.P;
    for (int i = 0; i < sp.P; ++i) a.portEq[i] = sp.portEq[i];
    a.kT40 = FOUR_K_B * 290.0;
    a.gs = 1.0 / eng->spZ0[0];
    a.S = eng->nNoiseSrc;
    a.srcA = eng->dNoiseA;
    a.srcB = eng->dNoiseB;
    return CSIM_OK;
}

// output pair of a distortion or intermodulation call -> the kernels' numbers (include/csim.h "Distortion analysis",
// "Intermodulation analysis"); `what` names the analysis in a refusal
int distoSetup(const csim_engine* eng, const char* what, int out_p, int out_m, csim::ChainArgs& a)
{
    const int N = eng->plan.N;
    const std::string who(what);
    if (acBlock(eng)) { setError(who + ": ac_kernel=block covers AC and noise analysis only"); return CSIM_ERR_UNSUPPORTED; }
    if (N > 63) { setError(who + " covers circuits of up to 63 unknowns"); return CSIM_ERR_UNSUPPORTED; }
    if (out_p < 0 || out_p >= N || out_m < -1 || out_m >= N || out_p == out_m) {
        setError(who + ": the output needs two different equations, out_p >= 0 (out_m = -1: ground)");
        return CSIM_ERR_ARG;
    }
    if (!eng->acAnySource) { setError(who + ": no source carries an AC magnitude (V/I ... AC mag [phase])"); return CSIM_ERR_CONFIG; }
    a.outP = out_p;
    a.outM = out_m;
    a.M = eng->nDistoDev;
    a.devD = eng->dDistoD;
    a.devG = eng->dDistoG;
    a.devS = eng->dDistoS;
    return CSIM_OK;
}

// What csim_disto_batch_dev and csim_imd_batch_dev share once `a` is set up: the coefficients go to the caller's
// [M][7][B] table or to the engine's scratch of one chunk; per chunk the coefficient kernel, then the analysis's sweep
// (`sweep(a)`, which may first set what only it knows of the chunk)
template <class Sweep>
int distoSweepChunks(csim_engine* eng, const double* d_params, int B, const double* d_xop, const double* freqs, int F, int which,
                     hipStream_t hs, double* d_coef, uint32_t* d_status, csim::ChainArgs& a, Sweep sweep)
{
    const int M = eng->nDistoDev, chunk = acChunk(eng, B);
    if (!d_coef)
        if (const int rc = growDevice(eng->dDistoCoef, eng->distoCoefCap, (size_t)csim::DISTO_NCOEF * M * (size_t)chunk, sizeof(double))) return rc;
    return acSweepChunks(eng, d_params, B, d_xop, freqs, F, which, hs, nullptr, d_status, a, [&](const double*, size_t, size_t) {
        double* const dCoef = d_coef ? d_coef : eng->dDistoCoef;
        a.coef = dCoef;
        a.coefStride = d_coef ? (size_t)B : (size_t)chunk;
        a.coefOff = d_coef ? (size_t)a.b0 : 0;
        const hipError_t e = csim::launchDistoCoef(eng->gpTran, eng->dDistoElem, M, d_params, B, a.b0, a.Bc, d_xop, dCoef,
                                                   a.coefStride, a.coefOff, hs);
        return e != hipSuccess ? e : sweep(a);
    });
}

// the probe of a loop-gain call -> the kernels' numbers (include/csim.h "Loop-gain analysis"); probe_elem -1: the card's
int stbSetup(const csim_engine* eng, int probe_elem, csim::StbArgs& a)
{
    const int N = eng->plan.N;
    if (const int rc = acBlockRefused(eng, "loop-gain analysis")) return rc;
    if (N > 63) { setError("loop-gain analysis covers circuits of up to 63 unknowns"); return CSIM_ERR_UNSUPPORTED; }
    if (probe_elem == -1) {
        if (!eng->cards.stb.enabled) { setError("loop-gain analysis: no probe given and the netlist has no .STB card"); return CSIM_ERR_CONFIG; }
        probe_elem = eng->cards.stbElem;
    }
    const csim::CircuitIR& c = eng->cir;
    if (probe_elem < 0 || probe_elem >= c.ir.n_elems) { setError("loop-gain analysis: the probe is not an element of the netlist"); return CSIM_ERR_CONFIG; }
    if (c.kind[(size_t)probe_elem] != CSIM_V) { setError("loop-gain analysis: the probe must be a V source"); return CSIM_ERR_CONFIG; }
    a.eqP = c.eq[4 * (size_t)probe_elem + 0];
    a.eqM = c.eq[4 * (size_t)probe_elem + 1];
    a.eqBr = c.branchEq[(size_t)probe_elem];
    if (a.eqP < 0 || a.eqP >= N || a.eqM < 0 || a.eqM >= N || a.eqBr < 0 || a.eqBr >= N || a.eqP == a.eqM) {
        setError("loop-gain analysis: the probe needs two different nodes off ground");
        return CSIM_ERR_CONFIG;
    }
    return CSIM_OK;
}

// margins need strictly increasing positive frequencies
bool stbFreqsIncrease(const double* freqs, int F)
{
    for (int f = 0; f < F; ++f)
        if (!(freqs[f] > (f ? freqs[f - 1] : 0.0)) || !std::isfinite(freqs[f])) return false;
    return true;
}

// fmax and sigma0 of a pole call and the engine's refusals, in the order include/csim.h "Pole analysis" states;
// fmax NaN: the card's pair
int pzSetup(const csim_engine* eng, const char* who, double& fmax, double& sigma0)
{
    const bool fromCard = fmax != fmax;
    if ((!fromCard && (!std::isfinite(fmax) || !(fmax > 0.0))) || !std::isfinite(sigma0)) {
        setError(std::string(who) + ": fmax must be finite and > 0 (NaN: the .PZ card's), sigma0 finite");
        return CSIM_ERR_ARG;
    }
    if (acBlock(eng) || eng->cfg.acKernel == csim::AC_KERNEL_PACKED) {
        setError("pole analysis: there is one kernel, ac_kernel=block and ac_kernel=packed do not cover it");
        return CSIM_ERR_UNSUPPORTED;
    }
    if (eng->plan.N > csim::PZ_MAX_N) { setError("pole analysis covers circuits of up to 63 unknowns"); return CSIM_ERR_UNSUPPORTED; }
    if (fromCard) {
        if (!eng->cards.pz.enabled) { setError(std::string(who) + ": no fmax given and the netlist has no .PZ card"); return CSIM_ERR_CONFIG; }
        fmax = eng->cards.pz.fmax;
        sigma0 = eng->cards.pz.sigma0;
        if (!std::isfinite(fmax) || !(fmax > 0.0) || !std::isfinite(sigma0)) {
            setError(std::string(who) + ": the .PZ card needs fmax > 0 and a finite sigma0");
            return CSIM_ERR_CONFIG;
        }
    }
    return CSIM_OK;
}

// ---- engine-free forms -----------------------------------------------------------

// [B][n][n] row-major -> the layout the sweep kernels read: G, C column-major, J re, J im (zeros without a J)
std::vector<double> packAcSystems(int n, int B, const double* G, const double* Cm, const double* J)
{
    const size_t nn = (size_t)n * n, per = csim::acSystemDoubles(n);
    std::vector<double> sys(per * (size_t)B);
    for (int b = 0; b < B; ++b) {
        double* s = sys.data() + per * (size_t)b;
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j) {
                s[(size_t)j * n + i] = G[nn * b + (size_t)i * n + j];
                s[nn + (size_t)j * n + i] = Cm[nn * b + (size_t)i * n + j];
            }
            s[2 * nn + i] = J ? J[((size_t)b * n + i) * 2] : 0.0;
            s[2 * nn + n + i] = J ? J[((size_t)b * n + i) * 2 + 1] : 0.0;
        }
    }
    return sys;
}

// the selector values of the *_solve_batch entries (3 is none)
bool acKernelValid(int kernel)
{
    return (kernel >= csim::AC_KERNEL_AUTO && kernel <= csim::AC_KERNEL_PACKED) || kernel == csim::AC_KERNEL_BLOCK;
}

// The common front of the engine-free *_solve_batch entries: device check, kernel choice and its refusals; then, when
// there is work, the packed systems, the angular frequencies and zeroed flags on the device.
struct AcSolveFront {
    int which = csim::AC_KERNEL_AUTO;
    DevBuf dSys, dOmega, dF, dWork;         // dWork: the block kernel's planes
    template <class Args> void fill(Args& a, int n, int F, int B)
    {
        acCommonArgs(a, n, F, B, 0, B, 1e-15, dSys.as<double>(), dOmega.as<double>(), dF.as<uint32_t>());
    }
};
int acSolveFront(const char* entry, int device, int n, int B, const double* G, const double* Cm, const double* J,
                 const double* omega, int F, int kernel, bool work, AcSolveFront& fr, bool blockCovered = false)
{
    const std::string name(entry);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
        setError(name + ": no usable HIP device (this library has no CPU path)");
        return CSIM_ERR_NO_DEVICE;
    }
    if (kernel == csim::AC_KERNEL_BLOCK) {
        if (!blockCovered) { setError(name + ": the block kernel covers AC and noise analysis only"); return CSIM_ERR_UNSUPPORTED; }
        if (n > 1024) { setError(name + ": the block kernel covers n <= 1024"); return CSIM_ERR_UNSUPPORTED; }
    } else if (n > 63) { setError(name + " covers n <= 63"); return CSIM_ERR_UNSUPPORTED; }
    if (const int rc = acPickKernel(kernel, n, entry, &fr.which)) return rc;
    if (!work) return CSIM_OK;
    HIPCHK(hipSetDevice(device));
    const std::vector<double> sys = packAcSystems(n, B, G, Cm, J);
    HIPCHK(fr.dSys.alloc(sizeof(double) * sys.size()));
    HIPCHK(fr.dOmega.alloc(sizeof(double) * (size_t)F));
    HIPCHK(fr.dF.alloc(sizeof(uint32_t) * (size_t)B));
    if (fr.which == csim::AC_KERNEL_BLOCK) HIPCHK(fr.dWork.alloc(sizeof(double) * csim::acBlockWorkDoubles(n) * (size_t)B));
    HIPCHK(hipMemcpy(fr.dSys.p, sys.data(), sizeof(double) * sys.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(fr.dOmega.p, omega, sizeof(double) * (size_t)F, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(fr.dF.p, 0, sizeof(uint32_t) * (size_t)B));
    return CSIM_OK;
}

// the generator table of an engine-free noise call on the device: terminals [S] and PSDs [B][S] -> [S][B]
struct GeneratorTable {
    DevBuf a, b, psd;
};
int uploadGenerators(int S, int B, const int32_t* src_a, const int32_t* src_b, const double* psd, GeneratorTable& g)
{
    std::vector<double> psdT((size_t)S * B);
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s) psdT[(size_t)s * B + b] = psd[(size_t)b * S + s];
    HIPCHK(g.a.alloc(sizeof(int32_t) * (size_t)S));
    HIPCHK(g.b.alloc(sizeof(int32_t) * (size_t)S));
    HIPCHK(g.psd.alloc(sizeof(double) * psdT.size()));
    if (S > 0) {
        HIPCHK(hipMemcpy(g.a.p, src_a, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(g.b.p, src_b, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(g.psd.p, psdT.data(), sizeof(double) * psdT.size(), hipMemcpyHostToDevice));
    }
    return CSIM_OK;
}

// the device table of the distortion and intermodulation kernels on the device: terminals [M], and the coefficients
// [B][M][7] of the caller as [M][7][B]
struct DeviceTable {
    DevBuf d, g, s, coef;
};
// the equations of a *_solve_batch call that index LDS: the output pair and the device terminals
int checkDeviceTable(const char* entry, int n, int M, const int32_t* dev_d, const int32_t* dev_g, const int32_t* dev_s, int out_p,
                     int out_m)
{
    if (n <= 0) return CSIM_OK;
    bool ok = out_p >= 0 && out_p < n && out_m >= -1 && out_m < n && out_p != out_m;
    for (int m = 0; m < M && ok && dev_d && dev_g && dev_s; ++m)
        ok = dev_d[m] >= -1 && dev_d[m] < n && dev_g[m] >= -1 && dev_g[m] < n && dev_s[m] >= -1 && dev_s[m] < n;
    if (!ok) { setError(std::string(entry) + ": equation index out of range (or out_p == out_m)"); return CSIM_ERR_ARG; }
    return CSIM_OK;
}
int uploadDevices(int M, int B, const int32_t* dev_d, const int32_t* dev_g, const int32_t* dev_s, const double* coef,
                  DeviceTable& t, csim::ChainArgs& a)
{
    const size_t MK = (size_t)M * csim::DISTO_NCOEF;
    std::vector<double> coefT(MK * (size_t)B);
    for (int b = 0; b < B; ++b)
        for (size_t q = 0; q < MK; ++q) coefT[q * (size_t)B + b] = coef[(size_t)b * MK + q];
    HIPCHK(t.d.alloc(sizeof(int32_t) * (size_t)M));
    HIPCHK(t.g.alloc(sizeof(int32_t) * (size_t)M));
    HIPCHK(t.s.alloc(sizeof(int32_t) * (size_t)M));
    HIPCHK(t.coef.alloc(sizeof(double) * coefT.size()));
    if (M > 0) {
        HIPCHK(hipMemcpy(t.d.p, dev_d, sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t.g.p, dev_g, sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t.s.p, dev_s, sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t.coef.p, coefT.data(), sizeof(double) * coefT.size(), hipMemcpyHostToDevice));
    }
    a.M = M;
    a.devD = t.d.as<int32_t>();
    a.devG = t.g.as<int32_t>();
    a.devS = t.s.as<int32_t>();
    a.coef = t.coef.as<double>();
    a.coefStride = (size_t)B;
    return CSIM_OK;
}

} // namespace

int csim::noiseResolve(const csim_engine* eng, int out_p, int out_m, int src_elem, double temp_k, int* inA, int* inB, double* kT4)
{
    csim::NoiseArgs a{};
    if (const int rc = noiseSetup(eng, out_p, out_m, src_elem, temp_k, a, *kT4)) return rc;
    *inA = a.inA;
    *inB = a.inB;
    return CSIM_OK;
}

size_t csim::acChunkCap(const csim_engine* eng)
{
    size_t per = sizeof(double) * csim::acSystemDoubles(eng->plan.N);
    if (acBlock(eng)) per += sizeof(double) * csim::acBlockWorkDoubles(eng->plan.N);
    return std::max<size_t>(acBlock(eng) ? 32 : 256, ((size_t)256 << 20) / per);
}

extern "C" {

// ---- AC small-signal analysis ----------------------------------------------

int csim_ac_system_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, double* d_sys, void* stream)
{
    if (!eng || B < 0 || (B > 0 && (!d_params || !d_xop || !d_sys))) { setError("csim_ac_system_dev: bad argument"); return CSIM_ERR_ARG; }
    if (const int rc = acSizeCheck(eng, "AC analysis")) return rc;
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    HIPCHK(csim::launchAcAssemble(eng->gpTran, eng->dAcRe, eng->dAcIm, d_params, B, 0, B, d_xop, d_sys,
                                  static_cast<hipStream_t>(stream), eng->cfg.acKernel));
    return CSIM_OK;
}

int csim_ac_batch_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, const double* freqs,
                      int32_t F, const int32_t* probe_eq, int32_t n_probe, double* d_out, uint32_t* d_status, void* stream)
{
    if (!eng || B < 0 || F < 0 || (B > 0 && F > 0 && (!d_params || !d_xop || !freqs || !d_out || !d_status))) {
        setError("csim_ac_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    if (const int rc = acCheck(eng)) return rc;
    const int N = eng->plan.N;
    if (probe_eq) {
        if (n_probe <= 0) { setError("csim_ac_batch_dev: n_probe must be positive"); return CSIM_ERR_ARG; }
        for (int i = 0; i < n_probe; ++i)
            if (probe_eq[i] < 0 || probe_eq[i] >= N) { setError("probe equation index out of range"); return CSIM_ERR_ARG; }
    }
    int which;
    if (const int rc = acPickKernel(eng->cfg.acKernel, N, nullptr, &which)) return rc;
    if (B == 0 || F == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);

    // the probe list: uploaded when it changes, cached otherwise
    csim::AcArgs a{};
    a.nProbe = probe_eq ? n_probe : N;
    a.out = d_out;
    if (probe_eq) {
        std::vector<int32_t> want(probe_eq, probe_eq + n_probe);
        if (eng->acProbeCur < 0 || want != eng->acProbeCache) {
            eng->acProbeCache.clear();
            if (const int rc = acUpload(eng->acProbeSlots, eng->acProbeCur, want.data(), sizeof(int32_t) * want.size())) return rc;
            eng->acProbeCache = want;
        }
        a.probe = static_cast<const int32_t*>(eng->acProbeSlots[(size_t)eng->acProbeCur].d);
    }
    const int rc = acSweepChunks(eng, d_params, B, d_xop, freqs, F, which, hs, nullptr, d_status, a, [&](const double*, size_t, size_t) {
        a.work = eng->dAcWork;
        return csim::launchAcSweep(which, a, hs);
    });
    if (rc) return rc;
    if (a.probe) HIPCHK(hipEventRecord(eng->acProbeSlots[(size_t)eng->acProbeCur].done, hs));
    return CSIM_OK;
}

int csim_ac_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F,
                  const int32_t* probe_eq, int32_t n_probe, double* out, uint32_t* status)
{
    if (!eng || B < 0) { setError("csim_ac_batch: bad argument"); return CSIM_ERR_ARG; }
    if (const int rc = acCheck(eng)) return rc;
    std::vector<double> card;
    if (!freqs)
        if (const int rc = cardFreqs(eng->cards.ac, "csim_ac_batch", ".AC", card, &freqs, &F)) return rc;
    if (F < 0 || (B > 0 && F > 0 && !out)) { setError("csim_ac_batch: bad argument"); return CSIM_ERR_ARG; }
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    OpPoint op;
    HostOutputs outs(F, B);
    double* dOut = outs.add(out, std::max(probe_eq ? n_probe : eng->plan.N, 0), 2);
    int rc = opPointSolve(eng, params, B, outs, op);
    if (!rc) rc = csim_ac_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), freqs, F, probe_eq, n_probe, dOut,
                                    op.status.as<uint32_t>(), nullptr);
    return rc ? rc : outs.finish(op.status, status);
}

// ---- noise analysis ---------------------------------------------------------

int csim_noise_batch_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, const double* freqs,
                         int32_t F, int32_t out_p_eq, int32_t out_m_eq, int32_t src_elem, double temp_k, double* d_onoise,
                         double* d_gain, double* d_contrib, double* d_psd, uint32_t* d_status, void* stream)
{
    if (!eng || B < 0 || F < 0 || (B > 0 && F > 0 && (!d_params || !d_xop || !freqs || !d_onoise || !d_status))) {
        setError("csim_noise_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    csim::NoiseArgs a{};
    PsdTarget psd{0.0, d_psd};
    if (const int rc = noiseSetup(eng, out_p_eq, out_m_eq, src_elem, temp_k, a, psd.kT4)) return rc;
    int which;
    if (const int rc = acPickKernel(eng->cfg.acKernel, eng->plan.N, nullptr, &which)) return rc;
    if (B == 0 || F == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);
    a.onoise = d_onoise;
    a.gain = d_gain;
    a.contrib = d_contrib;
    return acSweepChunks(eng, d_params, B, d_xop, freqs, F, which, hs, &psd, d_status, a,
                         [&](const double* dPsd, size_t psdStride, size_t psdOff) {
        a.psd = dPsd;
        a.psdStride = psdStride;
        a.psdOff = psdOff;
        a.work = eng->dAcWork;
        return csim::launchNoiseSweep(which, a, hs);
    });
}

int csim_noise_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, int32_t out_p_eq,
                     int32_t out_m_eq, int32_t src_elem, double temp_k, double* onoise, double* gain, double* contrib,
                     double* psd, uint32_t* status)
{
    if (!eng || B < 0) { setError("csim_noise_batch: bad argument"); return CSIM_ERR_ARG; }
    if (const int rc = acSizeCheck(eng, "noise analysis")) return rc;
    std::vector<double> card;
    if (!freqs)
        if (const int rc = cardFreqs(eng->cards.noise, "noise analysis", ".NOISE", card, &freqs, &F)) return rc;
    if (out_p_eq == -2) {
        if (!eng->cards.noise.enabled) { setError("csim_noise_batch: no output given and the netlist has no .NOISE card"); return CSIM_ERR_CONFIG; }
        out_p_eq = eng->cards.noiseOut.outP;
        out_m_eq = eng->cards.noiseOut.outM;
        src_elem = eng->cards.noiseOut.srcElem;
    }
    if (F < 0 || (B > 0 && F > 0 && !onoise)) { setError("csim_noise_batch: bad argument"); return CSIM_ERR_ARG; }
    {
        csim::NoiseArgs probe{};
        double kT4 = 0.0;
        if (const int rc = noiseSetup(eng, out_p_eq, out_m_eq, src_elem, temp_k, probe, kT4)) return rc;
    }
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    const int S = eng->nNoiseSrc;
    OpPoint op;
    HostOutputs outs(F, B);
    double* dOn = outs.add(onoise, 1, 1);
    double* dGain = outs.add(src_elem >= 0 ? gain : nullptr, 1, 2);
    double* dCon = outs.add(contrib, S, 1);
    double* dPsd = outs.add(F ? psd : nullptr, S, 1, false, true);     // no frequency: no sweep writes it
    int rc = opPointSolve(eng, params, B, outs, op);
    if (!rc) rc = csim_noise_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), freqs, F, out_p_eq, out_m_eq, src_elem,
                                       temp_k, dOn, dGain, dCon, dPsd, op.status.as<uint32_t>(), nullptr);
    return rc ? rc : outs.finish(op.status, status);
}

// ---- S-parameter analysis ---------------------------------------------------

int csim_sp_batch_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, const double* freqs,
                      int32_t F, double* d_y, double* d_s, uint32_t* d_status, void* stream)
{
    if (!eng || B < 0 || F < 0) { setError("csim_sp_batch_dev: bad argument"); return CSIM_ERR_ARG; }
    csim::SpArgs a{};
    if (const int rc = spSetup(eng, a)) return rc;          // no port: CSIM_ERR_CONFIG, whatever the buffers
    if (B > 0 && F > 0 && (!d_params || !d_xop || !freqs || !d_y || !d_status)) {
        setError("csim_sp_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    int which;
    if (const int rc = acPickKernel(eng->cfg.acKernel, eng->plan.N, nullptr, &which)) return rc;
    if (B == 0 || F == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);
    a.y = d_y;
    a.s = d_s;
    return acSweepChunks(eng, d_params, B, d_xop, freqs, F, which, hs, nullptr, d_status, a,
                         [&](const double*, size_t, size_t) { return csim::launchSpSweep(which, a, hs); });
}

int csim_sp_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, double* y, double* s,
                  uint32_t* status)
{
    if (!eng || B < 0) { setError("csim_sp_batch: bad argument"); return CSIM_ERR_ARG; }
    {
        csim::SpArgs probe{};
        if (const int rc = spSetup(eng, probe)) return rc;
    }
    std::vector<double> card;
    if (!freqs)
        if (const int rc = cardFreqs(eng->cards.sp, "csim_sp_batch", ".SP", card, &freqs, &F)) return rc;
    if (F < 0 || (B > 0 && F > 0 && !y)) { setError("csim_sp_batch: bad argument"); return CSIM_ERR_ARG; }
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    const int PP = (int)(eng->spPortEq.size() * eng->spPortEq.size());
    OpPoint op;
    HostOutputs outs(F, B);
    double* dY = outs.add(y, PP, 2);
    double* dS = outs.add(s, PP, 2);
    int rc = opPointSolve(eng, params, B, outs, op);
    if (!rc) rc = csim_sp_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), freqs, F, dY, dS, op.status.as<uint32_t>(),
                                    nullptr);
    return rc ? rc : outs.finish(op.status, status);
}

// ---- two-port noise analysis ------------------------------------------------

int csim_spnoise_batch_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, const double* freqs,
                           int32_t F, double temp_k, double* d_y, double* d_cy, double* d_nf, double* d_fmin, double* d_rn,
                           double* d_yopt, uint32_t* d_status, void* stream)
{
    if (!eng || B < 0 || F < 0) { setError("csim_spnoise_batch_dev: bad argument"); return CSIM_ERR_ARG; }
    csim::SpNoiseArgs a{};
    PsdTarget psd{0.0, nullptr};
    if (const int rc = spNoiseSetup(eng, temp_k, d_nf || d_fmin || d_rn || d_yopt, a, psd.kT4)) return rc;
    if (B > 0 && F > 0 && (!d_params || !d_xop || !freqs || !d_cy || !d_status)) {
        setError("csim_spnoise_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    int which;
    if (const int rc = acPickKernel(eng->cfg.acKernel, eng->plan.N, nullptr, &which)) return rc;
    if (B == 0 || F == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);
    a.y = d_y;
    a.cy = d_cy;
    a.nf = d_nf;
    a.fmin = d_fmin;
    a.rn = d_rn;
    a.yopt = d_yopt;
    return acSweepChunks(eng, d_params, B, d_xop, freqs, F, which, hs, &psd, d_status, a,
                         [&](const double* dPsd, size_t psdStride, size_t psdOff) {
        a.psd = dPsd;
        a.psdStride = psdStride;
        a.psdOff = psdOff;
        return csim::launchSpNoiseSweep(which, a, hs);
    });
}

int csim_spnoise_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, double temp_k,
                       double* y, double* cy, double* nf, double* fmin, double* rn, double* yopt, uint32_t* status)
{
    if (!eng || B < 0) { setError("csim_spnoise_batch: bad argument"); return CSIM_ERR_ARG; }
    {
        csim::SpNoiseArgs probe{};
        double kT4 = 0.0;
        if (const int rc = spNoiseSetup(eng, temp_k, nf || fmin || rn || yopt, probe, kT4)) return rc;
    }
    std::vector<double> card;
    if (!freqs)
        if (const int rc = cardFreqs(eng->cards.sp, "csim_spnoise_batch", ".SP", card, &freqs, &F)) return rc;
    if (F < 0 || (B > 0 && F > 0 && !cy)) { setError("csim_spnoise_batch: bad argument"); return CSIM_ERR_ARG; }
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    const int PP = (int)(eng->spPortEq.size() * eng->spPortEq.size());
    OpPoint op;
    HostOutputs outs(F, B);
    double* dCy = outs.add(cy, PP, 2);
    double* dY = outs.add(y, PP, 2);
    double* dNf = outs.add(nf, 1, 1);
    double* dFmin = outs.add(fmin, 1, 1);
    double* dRn = outs.add(rn, 1, 1);
    double* dYopt = outs.add(yopt, 1, 2);
    int rc = opPointSolve(eng, params, B, outs, op);
    if (!rc) rc = csim_spnoise_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), freqs, F, temp_k, dY, dCy, dNf, dFmin,
                                         dRn, dYopt, op.status.as<uint32_t>(), nullptr);
    return rc ? rc : outs.finish(op.status, status);
}

// ---- distortion analysis ----------------------------------------------------

int csim_disto_batch_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, const double* freqs,
                         int32_t F, int32_t out_p_eq, int32_t out_m_eq, double* d_h, double* d_hd, double* d_coef,
                         uint32_t* d_status, void* stream)
{
    if (!eng || B < 0 || F < 0 || (B > 0 && F > 0 && (!d_params || !d_xop || !freqs || !d_hd || !d_status))) {
        setError("csim_disto_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    csim::ChainArgs a{};
    if (const int rc = distoSetup(eng, "distortion analysis", out_p_eq, out_m_eq, a)) return rc;
    int which;
    if (const int rc = acPickKernel(eng->cfg.acKernel, eng->plan.N, nullptr, &which)) return rc;
    if (B == 0 || F == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);
    a.h = d_h;
    a.ratio = d_hd;
    return distoSweepChunks(eng, d_params, B, d_xop, freqs, F, which, hs, d_coef, d_status, a, [&](csim::ChainArgs& c) {
        return csim::launchDistoSweep(which, c, eng->distoD.data(), eng->distoG.data(), eng->distoS.data(), hs);
    });
}

int csim_disto_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, int32_t out_p_eq,
                     int32_t out_m_eq, double* h, double* hd, double* coef, uint32_t* status)
{
    if (!eng || B < 0) { setError("csim_disto_batch: bad argument"); return CSIM_ERR_ARG; }
    std::vector<double> card;
    if (!freqs)
        if (const int rc = cardFreqs(eng->cards.disto, "distortion analysis", ".DISTO", card, &freqs, &F)) return rc;
    if (out_p_eq == -2) {
        if (!eng->cards.disto.enabled) { setError("csim_disto_batch: no output given and the netlist has no .DISTO card"); return CSIM_ERR_CONFIG; }
        out_p_eq = eng->cards.distoOut.outP;
        out_m_eq = eng->cards.distoOut.outM;
    }
    if (F < 0 || (B > 0 && F > 0 && !hd)) { setError("csim_disto_batch: bad argument"); return CSIM_ERR_ARG; }
    {
        csim::ChainArgs probe{};
        if (const int rc = distoSetup(eng, "distortion analysis", out_p_eq, out_m_eq, probe)) return rc;
    }
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    OpPoint op;
    HostOutputs outs(F, B);
    double* dH = outs.add(h, 3 * eng->plan.N, 2);
    double* dHd = outs.add(hd, 2, 1);
    double* dCoef = outs.add(F ? coef : nullptr, csim::DISTO_NCOEF * eng->nDistoDev, 1, false, true);   // no frequency: no sweep writes it
    int rc = opPointSolve(eng, params, B, outs, op);
    if (!rc) rc = csim_disto_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), freqs, F, out_p_eq, out_m_eq, dH, dHd,
                                       dCoef, op.status.as<uint32_t>(), nullptr);
    return rc ? rc : outs.finish(op.status, status);
}

// ---- intermodulation analysis -------------------------------------------------

int csim_imd_batch_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, const double* freqs,
                       int32_t F, double f2, int32_t out_p_eq, int32_t out_m_eq, double* d_h, double* d_im, double* d_coef,
                       uint32_t* d_status, void* stream)
{
    if (!eng || B < 0 || F < 0 || !std::isfinite(f2) ||
        (B > 0 && F > 0 && (!d_params || !d_xop || !freqs || !d_im || !d_status))) {
        setError("csim_imd_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    csim::ChainArgs a{};
    if (const int rc = distoSetup(eng, "intermodulation analysis", out_p_eq, out_m_eq, a)) return rc;
    int which;
    if (const int rc = acPickKernel(eng->cfg.acKernel, eng->plan.N, nullptr, &which)) return rc;
    if (B == 0 || F == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);
    a.h = d_h;
    a.ratio = d_im;
    a.j2 = nullptr;                                         // both tones drive the same AC sources
    // one list for the sweep driver: the first tone's F frequencies, then the second tone's
    std::vector<double> tones((size_t)2 * F, f2);
    std::copy(freqs, freqs + F, tones.begin());
    return distoSweepChunks(eng, d_params, B, d_xop, tones.data(), 2 * F, which, hs, d_coef, d_status, a, [&](csim::ChainArgs& c) {
        c.F = F;
        c.omega2 = c.omega + F;
        return csim::launchImdSweep(which, c, eng->distoD.data(), eng->distoG.data(), eng->distoS.data(), hs);
    });
}

int csim_imd_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, double f2,
                   int32_t out_p_eq, int32_t out_m_eq, double* h, double* im, double* coef, uint32_t* status)
{
    if (!eng || B < 0) { setError("csim_imd_batch: bad argument"); return CSIM_ERR_ARG; }
    std::vector<double> card;
    if (!freqs) {
        if (const int rc = cardFreqs(eng->cards.imd, "intermodulation analysis", ".IMD", card, &freqs, &F)) return rc;
        f2 = eng->cards.imdF2overF1 * eng->cards.imd.fstart;
    }
    if (out_p_eq == -2) {
        if (!eng->cards.imd.enabled) { setError("csim_imd_batch: no output given and the netlist has no .IMD card"); return CSIM_ERR_CONFIG; }
        out_p_eq = eng->cards.imdOut.outP;
        out_m_eq = eng->cards.imdOut.outM;
    }
    if (F < 0 || !std::isfinite(f2) || (B > 0 && F > 0 && !im)) { setError("csim_imd_batch: bad argument"); return CSIM_ERR_ARG; }
    {
        csim::ChainArgs probe{};
        if (const int rc = distoSetup(eng, "intermodulation analysis", out_p_eq, out_m_eq, probe)) return rc;
    }
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    OpPoint op;
    HostOutputs outs(F, B);
    double* dH = outs.add(h, csim::IMD_NSOLVE * eng->plan.N, 2);
    double* dIm = outs.add(im, csim::IMD_NRATIO, 1);
    double* dCoef = outs.add(F ? coef : nullptr, csim::DISTO_NCOEF * eng->nDistoDev, 1, false, true);   // no frequency: no sweep writes it
    int rc = opPointSolve(eng, params, B, outs, op);
    if (!rc) rc = csim_imd_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), freqs, F, f2, out_p_eq, out_m_eq, dH, dIm,
                                     dCoef, op.status.as<uint32_t>(), nullptr);
    return rc ? rc : outs.finish(op.status, status);
}

// ---- loop-gain analysis -----------------------------------------------------

int csim_stb_batch_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, const double* freqs,
                       int32_t F, int32_t probe_elem, double* d_t, double* d_x, double* d_margins, int32_t* d_found,
                       uint32_t* d_status, void* stream)
{
    if (!eng || B < 0 || F < 0 || (B > 0 && F > 0 && (!d_params || !d_xop || !freqs || !d_t || !d_status)) ||
        (d_found && !d_margins)) {
        setError("csim_stb_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    if (d_margins && B > 0 && !stbFreqsIncrease(freqs, F)) {
        setError("csim_stb_batch_dev: margins need strictly increasing positive frequencies");
        return CSIM_ERR_ARG;
    }
    csim::StbArgs a{};
    if (const int rc = stbSetup(eng, probe_elem, a)) return rc;
    int which;
    if (const int rc = acPickKernel(eng->cfg.acKernel, eng->plan.N, nullptr, &which)) return rc;
    if (B == 0 || (F == 0 && !d_margins)) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);
    // the frequencies in Hz for the margins kernel: uploaded when the list changes, cached otherwise
    const double* dFreqs = nullptr;
    if (d_margins && F > 0) {
        std::vector<double> want(freqs, freqs + F);
        if (eng->stbFreqCur < 0 || want != eng->stbFreqCache) {
            eng->stbFreqCache.clear();
            if (const int rc = acUpload(eng->stbFreqSlots, eng->stbFreqCur, want.data(), sizeof(double) * want.size())) return rc;
            eng->stbFreqCache = want;
        }
        dFreqs = static_cast<const double*>(eng->stbFreqSlots[(size_t)eng->stbFreqCur].d);
    }
    a.t = d_t;
    a.x = d_x;
    if (F > 0)
        if (const int rc = acSweepChunks(eng, d_params, B, d_xop, freqs, F, which, hs, nullptr, d_status, a,
                                         [&](const double*, size_t, size_t) { return csim::launchStbSweep(which, a, hs); })) return rc;
    if (d_margins) {
        HIPCHK(csim::launchStbMargins(F, B, dFreqs, d_t, d_margins, d_found, hs));
        if (dFreqs) HIPCHK(hipEventRecord(eng->stbFreqSlots[(size_t)eng->stbFreqCur].done, hs));
    }
    return CSIM_OK;
}

int csim_stb_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, int32_t probe_elem,
                   double* t, double* x, double* margins, int32_t* found, uint32_t* status)
{
    if (!eng || B < 0 || (found && !margins)) { setError("csim_stb_batch: bad argument"); return CSIM_ERR_ARG; }
    std::vector<double> card;
    if (!freqs)
        if (const int rc = cardFreqs(eng->cards.stb, "loop-gain analysis", ".STB", card, &freqs, &F)) return rc;
    if (F < 0 || (B > 0 && F > 0 && !t)) { setError("csim_stb_batch: bad argument"); return CSIM_ERR_ARG; }
    if (margins && B > 0 && !stbFreqsIncrease(freqs, F)) {
        setError("csim_stb_batch: margins need strictly increasing positive frequencies");
        return CSIM_ERR_ARG;
    }
    {
        csim::StbArgs probe{};
        if (const int rc = stbSetup(eng, probe_elem, probe)) return rc;
    }
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    OpPoint op;
    HostOutputs outs(F, B);
    double* dT = outs.add(t, 1, 2);
    double* dX = outs.add(x, 2 * eng->plan.N, 2);
    double* dMargins = outs.add(margins, 4, 1, false, true);
    DevBuf dFound;
    if (found) HIPCHK(dFound.alloc(sizeof(int32_t) * (size_t)B));
    int rc = opPointSolve(eng, params, B, outs, op);
    if (!rc) rc = csim_stb_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), freqs, F, probe_elem, dT, dX, dMargins,
                                     found ? dFound.as<int32_t>() : nullptr, op.status.as<uint32_t>(), nullptr);
    if (!rc) rc = outs.finish(op.status, status);
    if (!rc && found) HIPCHK(hipMemcpy(found, dFound.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    return rc;
}

// ---- pole analysis ----------------------------------------------------------

int csim_pz_batch_dev(csim_engine* eng, const double* d_params, int32_t B, const double* d_xop, double fmax, double sigma0,
                      double* d_poles, int32_t* d_n_poles, int32_t* d_n_rhp, double* d_max_re, uint32_t* d_status, void* stream)
{
    if (!eng || B < 0 || (B > 0 && (!d_params || !d_xop || !d_poles || !d_n_poles || !d_n_rhp || !d_max_re || !d_status))) {
        setError("csim_pz_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    if (const int rc = pzSetup(eng, "csim_pz_batch_dev", fmax, sigma0)) return rc;
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const int N = eng->plan.N;
    const int chunk = acChunk(eng, B);
    if (const int rc = growDevice(eng->dAcSys, eng->acSysCap, (size_t)chunk, sizeof(double) * csim::acSystemDoubles(N))) return rc;
    csim::PzArgs a{};
    a.N = N; a.B = B;
    a.eps = eng->cir.ir.k.lu_eps;
    a.sigma0 = sigma0;
    a.wmax = csim::pz_wmax(fmax);
    a.sys = eng->dAcSys;
    a.poles = d_poles;
    a.nPoles = d_n_poles;
    a.nRhp = d_n_rhp;
    a.maxRe = d_max_re;
    a.status = d_status;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        a.b0 = b0;
        a.Bc = std::min(chunk, B - b0);
        HIPCHK(csim::launchAcAssemble(eng->gpTran, eng->dAcRe, eng->dAcIm, d_params, B, b0, a.Bc, d_xop, eng->dAcSys, hs,
                                      csim::AC_KERNEL_WAVE));
        HIPCHK(csim::launchPz(a, hs));
    }
    return CSIM_OK;
}

int csim_pz_batch(csim_engine* eng, const double* params, int32_t B, double fmax, double sigma0, double* poles,
                  int32_t* n_poles, int32_t* n_rhp, double* max_re, uint32_t* status)
{
    if (!eng || B < 0 || (B > 0 && !poles)) { setError("csim_pz_batch: bad argument"); return CSIM_ERR_ARG; }
    if (const int rc = pzSetup(eng, "csim_pz_batch", fmax, sigma0)) return rc;
    if (B == 0) return CSIM_OK;
    HIPCHK(hipSetDevice(eng->device));
    const int N = eng->plan.N;
    OpPoint op;
    HostOutputs outs(1, B);
    double* dPoles = outs.add(poles, N, 2, false, true);                        // [N][B] -> [B][N]
    DevBuf dNp, dNr, dMx;
    HIPCHK(dNp.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dNr.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dMx.alloc(sizeof(double) * (size_t)B));
    int rc = opPointSolve(eng, params, B, outs, op);
    if (!rc) rc = csim_pz_batch_dev(eng, op.params.as<double>(), B, op.x.as<double>(), fmax, sigma0, dPoles, dNp.as<int32_t>(),
                                    dNr.as<int32_t>(), dMx.as<double>(), op.status.as<uint32_t>(), nullptr);
    if (!rc) rc = outs.finish(op.status, status);
    if (rc) return rc;
    if (n_poles) HIPCHK(hipMemcpy(n_poles, dNp.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    if (n_rhp) HIPCHK(hipMemcpy(n_rhp, dNr.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    if (max_re) HIPCHK(hipMemcpy(max_re, dMx.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost));
    return CSIM_OK;
}

// ---- engine-free forms: any system through the sweep kernels, without an engine or a netlist ----------------

// the complex counterpart of csim_lu_solve_batch: any (G + jwC) x = J through the AC sweep kernels
int csim_ac_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* Cm, const double* J,
                        const double* omega, int32_t F, int32_t kernel, double* x, uint32_t* flags)
{
    if (n < 0 || B < 0 || F < 0 || !acKernelValid(kernel) ||
        (n > 0 && B > 0 && F > 0 && (!G || !Cm || !J || !omega || !x))) {
        setError("csim_ac_solve_batch: bad argument");
        return CSIM_ERR_ARG;
    }
    const bool work = n > 0 && B > 0 && F > 0;
    AcSolveFront fr;
    if (const int rc = acSolveFront("csim_ac_solve_batch", device, n, B, G, Cm, J, omega, F, kernel, work, fr, true)) return rc;
    if (!work) return CSIM_OK;
    HostOutputs outs(F, B);
    csim::AcArgs a{};
    fr.fill(a, n, F, B);
    a.nProbe = n;
    a.out = outs.add(x, n, 2, true);
    a.work = fr.dWork.as<double>();
    if (outs.rc) return outs.rc;
    HIPCHK(csim::launchAcSweep(fr.which, a, nullptr));
    return outs.finish(fr.dF, flags);
}

// the noise kernels: any system, any generator table
int csim_noise_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* Cm, int32_t out_p,
                           int32_t out_m, int32_t S, const int32_t* src_a, const int32_t* src_b, const double* psd,
                           int32_t in_kind, int32_t in_a, int32_t in_b, const double* omega, int32_t F, int32_t kernel,
                           double* onoise, double* contrib, double* gain, double* y, uint32_t* flags)
{
    const bool work = n > 0 && B > 0 && F > 0;
    if (n < 0 || B < 0 || F < 0 || S < 0 || !acKernelValid(kernel) ||
        in_kind < csim::NOISE_IN_NONE || in_kind > csim::NOISE_IN_I ||
        (work && (!G || !Cm || !omega || !onoise || (S > 0 && (!src_a || !src_b || !psd))))) {
        setError("csim_noise_solve_batch: bad argument");
        return CSIM_ERR_ARG;
    }
    if (n > 0) {
        bool ok = out_p >= 0 && out_p < n && out_m >= -1 && out_m < n && out_p != out_m;
        for (int s = 0; s < S && ok && src_a && src_b; ++s)
            ok = src_a[s] >= -1 && src_a[s] < n && src_b[s] >= -1 && src_b[s] < n;
        if (in_kind == csim::NOISE_IN_V) ok = ok && in_a >= 0 && in_a < n;
        if (in_kind == csim::NOISE_IN_I) ok = ok && in_a >= -1 && in_a < n && in_b >= -1 && in_b < n;
        if (!ok) { setError("csim_noise_solve_batch: equation index out of range (or out_p == out_m)"); return CSIM_ERR_ARG; }
    }
    AcSolveFront fr;
    if (const int rc = acSolveFront("csim_noise_solve_batch", device, n, B, G, Cm, nullptr, omega, F, kernel, work, fr, true)) return rc;
    if (!work) return CSIM_OK;
    GeneratorTable gen;
    if (const int rc = uploadGenerators(S, B, src_a, src_b, psd, gen)) return rc;
    HostOutputs outs(F, B);
    csim::NoiseArgs a{};
    fr.fill(a, n, F, B);
    a.S = S;
    a.outP = out_p; a.outM = out_m;
    a.inKind = in_kind; a.inA = in_a; a.inB = in_b;
    a.srcA = gen.a.as<int32_t>();
    a.srcB = gen.b.as<int32_t>();
    a.psd = gen.psd.as<double>();
    a.psdStride = (size_t)B;
    a.onoise = outs.add(onoise, 1, 1);
    a.gain = outs.add(in_kind != csim::NOISE_IN_NONE ? gain : nullptr, 1, 2);
    a.contrib = outs.add(contrib, S, 1);
    a.y = outs.add(y, n, 2);
    a.work = fr.dWork.as<double>();
    if (outs.rc) return outs.rc;
    HIPCHK(csim::launchNoiseSweep(fr.which, a, nullptr));
    return outs.finish(fr.dF, flags);
}

// the S-parameter kernels: K right-hand sides per system, or (port_eq given) the ports' unit vectors with Y and S
int csim_sp_solve_batch(int32_t device, int32_t n, int32_t B, int32_t K, const double* G, const double* Cm, const double* J,
                        const double* omega, int32_t F, int32_t kernel, double* x, uint32_t* flags, const int32_t* port_eq,
                        const double* z0, double* y, double* s)
{
    const bool work = n > 0 && B > 0 && F > 0;
    const bool ports = port_eq != nullptr;
    if (n < 0 || B < 0 || F < 0 || !acKernelValid(kernel) ||
        (work && (!G || !Cm || !omega || (ports ? (!z0 || !y) : (!J || !x))))) {
        setError("csim_sp_solve_batch: bad argument");
        return CSIM_ERR_ARG;
    }
    if (K < 1 || K > csim::SP_MAX_PORTS) { setError("csim_sp_solve_batch: 1 to 4 right-hand sides / ports"); return CSIM_ERR_ARG; }
    if (ports && n > 0)
        for (int i = 0; i < K; ++i) {
            if (port_eq[i] < 0 || port_eq[i] >= n) { setError("csim_sp_solve_batch: port equation out of range"); return CSIM_ERR_ARG; }
            if (!(z0[i] > 0.0) || !std::isfinite(z0[i])) { setError("csim_sp_solve_batch: Z0 must be finite and > 0"); return CSIM_ERR_ARG; }
        }
    AcSolveFront fr;
    if (const int rc = acSolveFront("csim_sp_solve_batch", device, n, B, G, Cm, nullptr, omega, F, kernel, work, fr)) return rc;
    if (!work) return CSIM_OK;
    HostOutputs outs(F, B);
    DevBuf dJ;
    csim::SpArgs a{};
    fr.fill(a, n, F, B);
    a.K = K;
    a.P = ports ? K : 0;
    a.x = outs.add(x, K * n, 2, true);                                          // [F][K][n][B] -> [B][F][K][n]
    if (ports) {
        for (int i = 0; i < K; ++i) { a.portEq[i] = port_eq[i]; a.sz[i] = std::sqrt(z0[i]); }
        a.y = outs.add(y, K * K, 2);
        a.s = outs.add(s, K * K, 2);
    } else {
        HIPCHK(dJ.alloc(sizeof(double) * (size_t)2 * K * n * B));
        HIPCHK(hipMemcpy(dJ.p, J, sizeof(double) * (size_t)2 * K * n * B, hipMemcpyHostToDevice));
        a.rhs = dJ.as<double>();
    }
    if (outs.rc) return outs.rc;
    HIPCHK(csim::launchSpSweep(fr.which, a, nullptr));
    return outs.finish(fr.dF, flags);
}

// the two-port noise kernels: any system, any ports, any generator table
int csim_spnoise_solve_batch(int32_t device, int32_t n, int32_t B, int32_t P, const double* G, const double* Cm,
                             const int32_t* port_eq, const double* z0, int32_t S, const int32_t* src_a, const int32_t* src_b,
                             const double* psd, const double* omega, int32_t F, int32_t kernel, double* y, double* cy,
                             double* nf, double* fmin, double* rn, double* yopt, double* x, uint32_t* flags)
{
    const bool work = n > 0 && B > 0 && F > 0;
    if (n < 0 || B < 0 || F < 0 || S < 0 || !acKernelValid(kernel) || !port_eq || !z0 ||
        (work && (!G || !Cm || !omega || !cy || (S > 0 && (!src_a || !src_b || !psd))))) {
        setError("csim_spnoise_solve_batch: bad argument");
        return CSIM_ERR_ARG;
    }
    if (P < 1 || P > csim::SP_MAX_PORTS) { setError("csim_spnoise_solve_batch: 1 to 4 ports"); return CSIM_ERR_ARG; }
    for (int i = 0; i < P; ++i)
        if (!(z0[i] > 0.0) || !std::isfinite(z0[i])) { setError("csim_spnoise_solve_batch: Z0 must be finite and > 0"); return CSIM_ERR_ARG; }
    if (n > 0) {
        bool ok = true;
        for (int i = 0; i < P; ++i) ok = ok && port_eq[i] >= 0 && port_eq[i] < n;
        for (int s = 0; s < S && ok && src_a && src_b; ++s)
            ok = src_a[s] >= -1 && src_a[s] < n && src_b[s] >= -1 && src_b[s] < n;
        if (!ok) { setError("csim_spnoise_solve_batch: equation index out of range"); return CSIM_ERR_ARG; }
    }
    if (P != 2 && (nf || fmin || rn || yopt)) { setError("csim_spnoise_solve_batch: NF, Fmin, Rn and Yopt exist for two ports only"); return CSIM_ERR_CONFIG; }
    AcSolveFront fr;
    if (const int rc = acSolveFront("csim_spnoise_solve_batch", device, n, B, G, Cm, nullptr, omega, F, kernel, work, fr)) return rc;
    if (!work) return CSIM_OK;
    GeneratorTable gen;
    if (const int rc = uploadGenerators(S, B, src_a, src_b, psd, gen)) return rc;
    HostOutputs outs(F, B);
    csim::SpNoiseArgs a{};
    fr.fill(a, n, F, B);
    a.P = P;
    a.S = S;
    for (int i = 0; i < P; ++i) a.portEq[i] = port_eq[i];
    a.kT40 = FOUR_K_B * 290.0;
    a.gs = 1.0 / z0[0];
    a.srcA = gen.a.as<int32_t>();
    a.srcB = gen.b.as<int32_t>();
    a.psd = gen.psd.as<double>();
    a.psdStride = (size_t)B;
    a.cy = outs.add(cy, P * P, 2);
    a.y = outs.add(y, P * P, 2);
    a.nf = outs.add(nf, 1, 1);
    a.fmin = outs.add(fmin, 1, 1);
    a.rn = outs.add(rn, 1, 1);
    a.yopt = outs.add(yopt, 1, 2);
    a.x = outs.add(x, P * n, 2);                                                // [F][P][n][B] -> [B][F][P][n]
    if (outs.rc) return outs.rc;
    HIPCHK(csim::launchSpNoiseSweep(fr.which, a, nullptr));
    return outs.finish(fr.dF, flags);
}

// the distortion kernels: any system, any device table
int csim_disto_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* Cm, const double* J, int32_t M,
                           const int32_t* dev_d, const int32_t* dev_g, const int32_t* dev_s, const double* coef, int32_t out_p,
                           int32_t out_m, const double* omega, int32_t F, int32_t kernel, double* h, double* hd,
                           uint32_t* flags)
{
    const bool work = n > 0 && B > 0 && F > 0;
    if (n < 0 || B < 0 || F < 0 || M < 0 || !acKernelValid(kernel) ||
        (work && (!G || !Cm || !J || !omega || !hd || (M > 0 && (!dev_d || !dev_g || !dev_s || !coef))))) {
        setError("csim_disto_solve_batch: bad argument");
        return CSIM_ERR_ARG;
    }
    if (const int rc = checkDeviceTable("csim_disto_solve_batch", n, M, dev_d, dev_g, dev_s, out_p, out_m)) return rc;
    AcSolveFront fr;
    if (const int rc = acSolveFront("csim_disto_solve_batch", device, n, B, G, Cm, J, omega, F, kernel, work, fr)) return rc;
    if (!work) return CSIM_OK;
    csim::ChainArgs a{};
    fr.fill(a, n, F, B);
    DeviceTable dev;
    if (const int rc = uploadDevices(M, B, dev_d, dev_g, dev_s, coef, dev, a)) return rc;
    HostOutputs outs(F, B);
    a.outP = out_p; a.outM = out_m;
    a.ratio = outs.add(hd, 2, 1);
    a.h = outs.add(h, 3 * n, 2);
    if (outs.rc) return outs.rc;
    HIPCHK(csim::launchDistoSweep(fr.which, a, dev_d, dev_g, dev_s, nullptr));
    return outs.finish(fr.dF, flags);
}

// the intermodulation kernels: any system, any device table, any finite tone pairs; J2 null: the second tone is
// excited as the first
int csim_imd_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* Cm, const double* J,
                         const double* J2, int32_t M, const int32_t* dev_d, const int32_t* dev_g, const int32_t* dev_s,
                         const double* coef, int32_t out_p, int32_t out_m, const double* omega1, const double* omega2,
                         int32_t F, int32_t kernel, double* h, double* im, uint32_t* flags)
{
    const bool work = n > 0 && B > 0 && F > 0;
    if (n < 0 || B < 0 || F < 0 || M < 0 || !acKernelValid(kernel) ||
        (work && (!G || !Cm || !J || !omega1 || !omega2 || !im || (M > 0 && (!dev_d || !dev_g || !dev_s || !coef))))) {
        setError("csim_imd_solve_batch: bad argument");
        return CSIM_ERR_ARG;
    }
    if (const int rc = checkDeviceTable("csim_imd_solve_batch", n, M, dev_d, dev_g, dev_s, out_p, out_m)) return rc;
    std::vector<double> tones;                              // the first tone's F frequencies, then the second tone's
    if (work) {
        tones.assign(omega1, omega1 + F);
        tones.insert(tones.end(), omega2, omega2 + F);
        for (double w : tones)
            if (!std::isfinite(w)) { setError("csim_imd_solve_batch: the tone frequencies must be finite"); return CSIM_ERR_ARG; }
    }
    AcSolveFront fr;
    if (const int rc = acSolveFront("csim_imd_solve_batch", device, n, B, G, Cm, J, tones.data(), 2 * F, kernel, work, fr)) return rc;
    if (!work) return CSIM_OK;
    csim::ChainArgs a{};
    fr.fill(a, n, F, B);
    DeviceTable dev;
    if (const int rc = uploadDevices(M, B, dev_d, dev_g, dev_s, coef, dev, a)) return rc;
    DevBuf dJ2;                                             // J2 [B][n] complex -> [B][re [n], im [n]]
    if (J2) {
        std::vector<double> planar((size_t)2 * n * B);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < n; ++i) {
                planar[((size_t)b * 2) * n + i] = J2[((size_t)b * n + i) * 2];
                planar[((size_t)b * 2 + 1) * n + i] = J2[((size_t)b * n + i) * 2 + 1];
            }
        HIPCHK(dJ2.alloc(sizeof(double) * planar.size()));
        HIPCHK(hipMemcpy(dJ2.p, planar.data(), sizeof(double) * planar.size(), hipMemcpyHostToDevice));
    }
    HostOutputs outs(F, B);
    a.omega2 = a.omega + F;
    a.j2 = J2 ? dJ2.as<double>() : nullptr;
    a.outP = out_p; a.outM = out_m;
    a.ratio = outs.add(im, csim::IMD_NRATIO, 1);
    a.h = outs.add(h, csim::IMD_NSOLVE * n, 2);
    if (outs.rc) return outs.rc;
    HIPCHK(csim::launchImdSweep(fr.which, a, dev_d, dev_g, dev_s, nullptr));
    return outs.finish(fr.dF, flags);
}

// the loop-gain kernels: any system, any probe; the margins kernel on their T
int csim_stb_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* Cm, int32_t eq_p, int32_t eq_m,
                         int32_t eq_br, const double* omega, int32_t F, int32_t kernel, double* T, double* x, uint32_t* flags,
                         const double* freqs_hz, double* margins, int32_t* found)
{
    const bool work = n > 0 && B > 0 && F > 0;
    if (n < 0 || B < 0 || F < 0 || !acKernelValid(kernel) || (found && !margins) ||
        (work && (!G || !Cm || !omega || !T || (margins && !freqs_hz)))) {
        setError("csim_stb_solve_batch: bad argument");
        return CSIM_ERR_ARG;
    }
    if (work && margins && !stbFreqsIncrease(freqs_hz, F)) {
        setError("csim_stb_solve_batch: margins need strictly increasing positive frequencies");
        return CSIM_ERR_ARG;
    }
    if (n > 0 && (eq_p < 0 || eq_p >= n || eq_m < 0 || eq_m >= n || eq_br < 0 || eq_br >= n || eq_p == eq_m || eq_p == eq_br ||
                  eq_m == eq_br)) {
        setError("csim_stb_solve_batch: the probe needs three different equations in range");
        return CSIM_ERR_ARG;
    }
    AcSolveFront fr;
    if (const int rc = acSolveFront("csim_stb_solve_batch", device, n, B, G, Cm, nullptr, omega, F, kernel, work, fr)) return rc;
    if (!work) return CSIM_OK;
    HostOutputs outs(F, B);
    csim::StbArgs a{};
    fr.fill(a, n, F, B);
    a.eqP = eq_p; a.eqM = eq_m; a.eqBr = eq_br;
    a.t = outs.add(T, 1, 2);
    a.x = outs.add(x, 2 * n, 2);                                                // [F][2][n][B] -> [B][F][2][n]
    double* dMargins = outs.add(margins, 4, 1, false, true);                    // [4][B] -> [B][4]
    if (outs.rc) return outs.rc;
    DevBuf dFreqs, dFound;
    HIPCHK(csim::launchStbSweep(fr.which, a, nullptr));
    if (margins) {
        HIPCHK(dFreqs.alloc(sizeof(double) * (size_t)F));
        HIPCHK(hipMemcpy(dFreqs.p, freqs_hz, sizeof(double) * (size_t)F, hipMemcpyHostToDevice));
        if (found) HIPCHK(dFound.alloc(sizeof(int32_t) * (size_t)B));
        HIPCHK(csim::launchStbMargins(F, B, dFreqs.as<double>(), a.t, dMargins, found ? dFound.as<int32_t>() : nullptr, nullptr));
    }
    if (const int rc = outs.finish(fr.dF, flags)) return rc;
    if (margins && found) HIPCHK(hipMemcpy(found, dFound.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    return CSIM_OK;
}

// the pole kernel: any (G, C)
int csim_pz_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* Cm, double fmax, double sigma0,
                        double* poles, int32_t* n_poles, int32_t* n_rhp, double* max_re, uint32_t* flags)
{
    const bool work = n > 0 && B > 0;
    if (n < 0 || B < 0 || !std::isfinite(fmax) || !(fmax > 0.0) || !std::isfinite(sigma0) || (work && (!G || !Cm || !poles))) {
        setError("csim_pz_solve_batch: bad argument");
        return CSIM_ERR_ARG;
    }
    if (n > csim::PZ_MAX_N) { setError("csim_pz_solve_batch covers n <= 63"); return CSIM_ERR_UNSUPPORTED; }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
        setError("csim_pz_solve_batch: no usable HIP device (this library has no CPU path)");
        return CSIM_ERR_NO_DEVICE;
    }
    if (!work) return CSIM_OK;
    HIPCHK(hipSetDevice(device));
    const std::vector<double> sys = packAcSystems(n, B, G, Cm, nullptr);
    DevBuf dSys, dF, dNp, dNr, dMx;
    HIPCHK(dSys.alloc(sizeof(double) * sys.size()));
    HIPCHK(dF.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(dNp.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dNr.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dMx.alloc(sizeof(double) * (size_t)B));
    HIPCHK(hipMemcpy(dSys.p, sys.data(), sizeof(double) * sys.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dF.p, 0, sizeof(uint32_t) * (size_t)B));
    HostOutputs outs(1, B);
    csim::PzArgs a{};
    a.N = n; a.B = B; a.b0 = 0; a.Bc = B;
    a.eps = 1e-15;
    a.sigma0 = sigma0;
    a.wmax = csim::pz_wmax(fmax);
    a.sys = dSys.as<double>();
    a.poles = outs.add(poles, n, 2, false, true);                               // [n][B] -> [B][n]
    a.nPoles = dNp.as<int32_t>();
    a.nRhp = dNr.as<int32_t>();
    a.maxRe = dMx.as<double>();
    a.status = dF.as<uint32_t>();
    if (outs.rc) return outs.rc;
    HIPCHK(csim::launchPz(a, nullptr));
    if (const int rc = outs.finish(dF, flags)) return rc;
    if (n_poles) HIPCHK(hipMemcpy(n_poles, dNp.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    if (n_rhp) HIPCHK(hipMemcpy(n_rhp, dNr.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    if (max_re) HIPCHK(hipMemcpy(max_re, dMx.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost));
    return CSIM_OK;
}

} // extern "C"
