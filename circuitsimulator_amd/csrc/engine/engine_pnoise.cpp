// engine_pnoise.cpp -- C-ABI of the periodic noise analysis (include/csim.h "Periodic noise analysis"): the device form
// csim_pnoise_batch_dev (per instance chunk one W_K launch and one orbit launch, per frequency chunk two backward passes
// around the closure solve, on the caller's stream) and the host form csim_pnoise_batch (DC operating point, periodic
// steady state, then this).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "csim.h"
#include "engine_host.hpp"
#include "kernels.hpp"
#include "pnoise.hpp"
#include "pss.hpp"

using csim::setError;

namespace {

// what a call asks for, after the defaults: refused here, before anything looks at the device
struct PnoisePlan {
    double tstep, f0, kT4;
    int nSide, Fc, outP, outM, srcElem, inA, inB;
    int64_t K;
    std::vector<double> freqs;
};

int pnoiseResolve(const csim_engine* eng, const char* who, bool cardDefaults, double tstep, double f0, const double* freqs,
                  int F, int n_side, int out_p, int out_m, int src_elem, double temp_k, PnoisePlan& p)
{
    const std::string w(who);
    if (std::isnan(tstep) || std::isinf(tstep) || std::isnan(f0) || std::isinf(f0)) {
        setError(w + ": tstep and f0 must be finite");
        return CSIM_ERR_ARG;
    }
    if (F < 0 || (F > 0 && !freqs)) { setError(w + ": bad argument"); return CSIM_ERR_ARG; }
    if (n_side < 0) { setError(w + ": n_side must be >= 0"); return CSIM_ERR_ARG; }
    if (F == 0) {
        if (!cardDefaults || freqs || !eng->pnoiseEnabled) { setError(w + ": no frequencies given and no .PNOISE card to take them from"); return CSIM_ERR_ARG; }
        const int64_t n = csim_ac_num_freqs(eng->pnoiseSweep, eng->pnoisePoints, eng->pnoiseFstart, eng->pnoiseFstop);
        if (n < 0) return (int)n;
        p.freqs.resize((size_t)n);
        if (const int rc = csim_ac_freqs(eng->pnoiseSweep, eng->pnoisePoints, eng->pnoiseFstart, eng->pnoiseFstop, p.freqs.data())) return rc;
    } else {
        p.freqs.assign(freqs, freqs + F);
    }
    for (const double f : p.freqs)
        if (!std::isfinite(f) || !(f > 0.0)) { setError(w + ": every frequency must be finite and positive"); return CSIM_ERR_ARG; }
    if (cardDefaults && out_p == -2) {
        if (!eng->pnoiseEnabled) { setError(w + ": no output given and the netlist has no .PNOISE card"); return CSIM_ERR_CONFIG; }
        out_p = eng->pnoiseOutP;
        out_m = eng->pnoiseOutM;
        src_elem = eng->pnoiseSrcElem;
    }
    if (cardDefaults && !(f0 > 0.0)) {
        if (!eng->hbEnabled) { setError(w + ": no f0 given and the netlist has no .HB card"); return CSIM_ERR_CONFIG; }
        f0 = eng->hbF0;
    }
    if (cardDefaults && !(tstep > 0.0)) {
        if (!eng->tranEnabled) { setError(w + ": no tstep given and the netlist has no .TRAN card"); return CSIM_ERR_CONFIG; }
        tstep = eng->tranTstep;
    }
    if (!(f0 > 0.0)) { setError(w + ": no f0 given"); return CSIM_ERR_CONFIG; }
    const int64_t K = csim::pss_num_steps(tstep, f0);
    if (K < 0) {
        setError(w + ": the period 1/f0 must be a whole number of steps, at most 2^22 (|K tstep f0 - 1| <= 1e-9)");
        return (int)K;
    }
    if (K < 2 * (int64_t)n_side + 1) {
        setError(w + ": " + std::to_string(K) + " steps per period cannot tell " + std::to_string(n_side) + " sidebands apart (K >= 2 n_side + 1)");
        return CSIM_ERR_CONFIG;
    }
    const int N = eng->plan.N;
    if (N > 63) { setError("periodic noise analysis covers circuits of up to 63 unknowns"); return CSIM_ERR_UNSUPPORTED; }
    if (const int rc = csim::noiseResolve(eng, out_p, out_m, src_elem, temp_k, &p.inA, &p.inB, &p.kT4)) return rc;
    p.tstep = tstep;
    p.f0 = f0;
    p.nSide = n_side;
    p.K = K;
    p.outP = out_p;
    p.outM = out_m;
    p.srcElem = src_elem;
    p.Fc = csim::pnoiseMaxFc(eng->gpTran, p.nSide, eng->nNoiseSrc);
    if (p.Fc < 1) {
        setError(w + ": the transfer sums of " + std::to_string(eng->nNoiseSrc) + " generators and " + std::to_string(2 * n_side + 1) +
                 " sidebands do not fit the LDS at one frequency per launch");
        return CSIM_ERR_CONFIG;
    }
    const size_t perInstance = (size_t)K * (size_t)N * sizeof(double);
    if (perInstance > csim::PNOISE_ORBIT_BUDGET) {
        setError(w + ": the orbit of one instance, " + std::to_string(K) + " steps of " + std::to_string(N) + " unknowns (" +
                 std::to_string(perInstance) + " bytes), does not fit the orbit store of " + std::to_string(csim::PNOISE_ORBIT_BUDGET) + " bytes");
        return CSIM_ERR_CONFIG;
    }
    return CSIM_OK;
}

int pnoiseRun(csim_engine* eng, const PnoisePlan& p, const double* d_params, int B, const double* d_x0, double* d_onoise,
              double* d_gain, double* d_contrib, double* d_side, uint32_t* d_status, hipStream_t hs)
{
    const int N = eng->plan.N, F = (int)p.freqs.size(), Fc = p.Fc;
    // the periodic steady state's chunk, reduced until the orbit of a chunk fits its budget
    const size_t perInstance = (size_t)p.K * (size_t)N * sizeof(double);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)csim::pssChunk(eng, B), csim::PNOISE_ORBIT_BUDGET / perInstance));

    std::vector<double> tw(2 * (size_t)p.K);
    csim::pss_twiddles(p.K, tw.data(), tw.data() + p.K);
    std::vector<double> z(4 * (size_t)F);                   // zr, zi, zKr, zKi, [F] each
    for (int f = 0; f < F; ++f) csim::pac_z(p.freqs[(size_t)f], p.tstep, p.f0, &z[f], &z[F + f], &z[2 * F + f], &z[3 * F + f]);

    DevBuf dTw, dZ, dXk, dW, dDone, dWst, dGk, dStop, dOrbitStop, dOrbit;
    HIPCHK(dTw.alloc(sizeof(double) * tw.size()));
    HIPCHK(hipMemcpy(dTw.p, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice));
    HIPCHK(dZ.alloc(sizeof(double) * z.size()));
    HIPCHK(hipMemcpy(dZ.p, z.data(), sizeof(double) * z.size(), hipMemcpyHostToDevice));
    HIPCHK(dXk.alloc(sizeof(double) * (size_t)N * (size_t)B));
    HIPCHK(dW.alloc(sizeof(double) * (size_t)N * (size_t)N * (size_t)chunk));
    HIPCHK(dDone.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dWst.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(dGk.alloc(sizeof(double) * (size_t)N * 2 * (size_t)Fc * (size_t)chunk));
    HIPCHK(dStop.alloc(sizeof(int32_t) * (size_t)chunk));
    HIPCHK(dOrbitStop.alloc(sizeof(int32_t) * (size_t)chunk));
    HIPCHK(dOrbit.alloc(perInstance * (size_t)chunk));
    HIPCHK(hipMemsetAsync(dDone.p, 0, sizeof(int32_t) * (size_t)B, hs));
    HIPCHK(hipMemsetAsync(dWst.p, 0, sizeof(uint32_t) * (size_t)B, hs));

    // the W_K launch is the periodic steady state's period kernel on a status word of its own: no harmonics, no update
    csim::PssArgs wa{};
    wa.params = d_params; wa.B = B; wa.dt = p.tstep; wa.K = (int)p.K; wa.H = 0;
    wa.probeEq = nullptr; wa.nProbe = 0;
    wa.twc = dTw.as<double>(); wa.tws = dTw.as<double>() + p.K;
    wa.x0 = const_cast<double*>(d_x0);                      // the period kernel reads it only
    wa.xK = dXk.as<double>(); wa.harm = nullptr; wa.W = dW.as<double>();
    wa.status = dWst.as<uint32_t>(); wa.done = dDone.as<int32_t>();

    csim::PnoiseArgs a{};
    a.params = d_params; a.B = B; a.dt = p.tstep; a.K = (int)p.K; a.M = p.nSide; a.F = F;
    a.twc = wa.twc; a.tws = wa.tws;
    a.x0 = d_x0; a.orbit = dOrbit.as<double>(); a.W = dW.as<double>(); a.wStatus = dWst.as<uint32_t>();
    a.outP = p.outP; a.outM = p.outM;
    a.S = eng->nNoiseSrc; a.srcElem = eng->dNoiseElem; a.srcA = eng->dNoiseA; a.srcB = eng->dNoiseB;
    a.inA = p.inA; a.inB = p.inB; a.kT4 = p.kT4;
    a.gK = dGk.as<double>();
    a.onoise = d_onoise; a.gain = d_gain; a.contrib = d_contrib; a.side = d_side;
    a.orbitStop = dOrbitStop.as<int32_t>(); a.stop = dStop.as<int32_t>(); a.status = d_status;

    // The scratch above lives until the stream has drained: the one exit below comes after a synchronisation.
    hipError_t e = hipSuccess;
    for (int b0 = 0; b0 < B && e == hipSuccess; b0 += chunk) {
        wa.b0 = a.b0 = b0;
        wa.Bc = a.Bc = std::min(chunk, B - b0);
        e = csim::launchPssPeriod(eng->gpTran, wa, hs);
        if (e == hipSuccess) e = hipMemsetAsync(dOrbitStop.p, 0, sizeof(int32_t) * (size_t)a.Bc, hs);
        if (e == hipSuccess) e = csim::launchPnoiseOrbit(eng->gpTran, a, hs);
        for (int f0i = 0; f0i < F && e == hipSuccess; f0i += Fc) {
            a.fFirst = f0i;
            a.Fc = std::min(Fc, F - f0i);
            a.zr = dZ.as<double>() + f0i; a.zi = a.zr + F; a.zKr = a.zi + F; a.zKi = a.zKr + F;
            e = hipMemsetAsync(dStop.p, 0, sizeof(int32_t) * (size_t)a.Bc, hs);
            a.g0 = nullptr;
            if (e == hipSuccess) e = csim::launchPnoisePeriod(eng->gpTran, a, hs);
            if (e == hipSuccess) e = csim::launchPnoiseClose(eng->gpTran, a, hs);
            a.g0 = a.gK;
            if (e == hipSuccess) e = csim::launchPnoisePeriod(eng->gpTran, a, hs);
        }
    }
    const hipError_t es = hipStreamSynchronize(hs);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { setError(std::string("csim_pnoise_batch_dev: ") + hipGetErrorString(e)); return CSIM_ERR_HIP; }
    return CSIM_OK;
}

} // namespace

extern "C" {

int csim_pnoise_batch_dev(csim_engine* eng, const double* d_params, int32_t B, double tstep, double f0, const double* d_x0,
                          const double* freqs, int32_t F, int32_t n_side, int32_t out_p_eq, int32_t out_m_eq, int32_t src_elem,
                          double temp_k, double* d_onoise, double* d_gain, double* d_contrib, double* d_side,
                          uint32_t* d_status, void* stream)
{
    if (!eng || !d_params || !d_x0 || !freqs || !d_onoise || !d_status || B <= 0 || F <= 0) {
        setError("csim_pnoise_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    PnoisePlan p{};
    if (const int rc = pnoiseResolve(eng, "csim_pnoise_batch_dev", false, tstep, f0, freqs, F, n_side, out_p_eq, out_m_eq,
                                     src_elem, temp_k, p)) return rc;
    HIPCHK(hipSetDevice(eng->device));
    return pnoiseRun(eng, p, d_params, B, d_x0, d_onoise, d_gain, d_contrib, d_side, d_status, static_cast<hipStream_t>(stream));
}

int csim_pnoise_batch(csim_engine* eng, const double* params, int32_t B, double tstep, double f0, const double* freqs,
                      int32_t F, int32_t n_side, int32_t out_p_eq, int32_t out_m_eq, int32_t src_elem, double temp_k,
                      double* onoise, double* gain, double* contrib, double* side, double* x0_out, int32_t* rounds,
                      uint32_t* status)
{
    if (!eng || !onoise || B <= 0) { setError("csim_pnoise_batch: bad argument"); return CSIM_ERR_ARG; }
    PnoisePlan p{};
    if (const int rc = pnoiseResolve(eng, "csim_pnoise_batch", true, tstep, f0, freqs, F, n_side, out_p_eq, out_m_eq, src_elem,
                                     temp_k, p)) return rc;
    HIPCHK(hipSetDevice(eng->device));
    const int N = eng->plan.N, nF = (int)p.freqs.size(), nSb = 2 * p.nSide + 1, S = eng->nNoiseSrc;
    DevBuf dParams, dX, dIters, dStatus, dHarm, dRounds, dOn, dGain, dCon, dSide;
    if (const int rc = csim::stageParams(eng, params, B, dParams)) return rc;
    HIPCHK(dX.alloc(sizeof(double) * (size_t)N * B));
    HIPCHK(dIters.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dStatus.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(dHarm.alloc(sizeof(double) * 2));
    HIPCHK(dRounds.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dOn.alloc(sizeof(double) * (size_t)nF * B));
    if (gain) HIPCHK(dGain.alloc(sizeof(double) * 2 * (size_t)nF * nSb * B));
    if (contrib) HIPCHK(dCon.alloc(sizeof(double) * (size_t)nF * S * B));
    if (side) HIPCHK(dSide.alloc(sizeof(double) * (size_t)nF * nSb * B));
    if (const int rc = csim_dc_batch_dev(eng, dParams.as<double>(), B, dX.as<double>(), dIters.as<int32_t>(),
                                         dStatus.as<uint32_t>(), nullptr)) return rc;
    // the steady state with no harmonics stored: an empty probe list
    const int32_t none = 0;
    if (const int rc = csim_pss_batch_dev(eng, dParams.as<double>(), B, p.tstep, p.f0, 0, &none, 0, 0.0, 0, dX.as<double>(),
                                          dHarm.as<double>(), dRounds.as<int32_t>(), dStatus.as<uint32_t>(), nullptr)) return rc;
    if (const int rc = pnoiseRun(eng, p, dParams.as<double>(), B, dX.as<double>(), dOn.as<double>(), dGain.as<double>(),
                                 dCon.as<double>(), dSide.as<double>(), dStatus.as<uint32_t>(), nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    // [F][per][B] (x width) on the device -> [B][F][per] (x width) for the caller
    auto fetch = [&](DevBuf& d, double* out, size_t per, int width) -> int {
        if (!out) return CSIM_OK;
        const size_t rows = (size_t)nF * per;
        std::vector<double> h(rows * (size_t)B * width);
        HIPCHK(hipMemcpy(h.data(), d.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < rows; ++e)
            for (int b = 0; b < B; ++b)
                for (int k = 0; k < width; ++k) out[((size_t)b * rows + e) * width + k] = h[(e * B + b) * width + k];
        return CSIM_OK;
    };
    if (const int rc = fetch(dOn, onoise, 1, 1)) return rc;
    if (const int rc = fetch(dGain, gain, (size_t)nSb, 2)) return rc;
    if (const int rc = fetch(dCon, contrib, (size_t)S, 1)) return rc;
    if (const int rc = fetch(dSide, side, (size_t)nSb, 1)) return rc;
    if (x0_out) {
        std::vector<double> x((size_t)N * B);
        HIPCHK(hipMemcpy(x.data(), dX.p, sizeof(double) * x.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i)
            for (int b = 0; b < B; ++b) x0_out[(size_t)b * N + i] = x[(size_t)i * B + b];
    }
    if (rounds) HIPCHK(hipMemcpy(rounds, dRounds.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, dStatus.p, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost));
    return CSIM_OK;
}

} // extern "C"
