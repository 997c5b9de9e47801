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
    if (const int rc = csim::periodResolveFreqs(w, cardDefaults, eng->cards.pnoise, ".PNOISE", freqs, F, p.freqs)) return rc;
    if (cardDefaults && out_p == -2) {
        if (!eng->cards.pnoise.enabled) { setError(w + ": no output given and the netlist has no .PNOISE card"); return CSIM_ERR_CONFIG; }
        out_p = eng->cards.pnoiseOut.outP;
        out_m = eng->cards.pnoiseOut.outM;
        src_elem = eng->cards.pnoiseOut.srcElem;
    }
    if (cardDefaults && !(f0 > 0.0)) {
        if (!eng->cards.hb.enabled) { setError(w + ": no f0 given and the netlist has no .HB card"); return CSIM_ERR_CONFIG; }
        f0 = eng->cards.hb.f0;
    }
    int64_t K = 0;
    if (const int rc = csim::periodResolveSteps(eng, w, cardDefaults, tstep, f0, K)) return rc;
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

    csim::PeriodWk wk;
    DevBuf dGk, dStop, dOrbitStop, dOrbit;
    if (const int rc = csim::periodWkSetup(wk, eng, d_params, B, chunk, p.tstep, p.f0, p.K, p.freqs, d_x0, hs)) return rc;
    HIPCHK(dGk.alloc(sizeof(double) * (size_t)N * 2 * (size_t)Fc * (size_t)chunk));
    HIPCHK(dStop.alloc(sizeof(int32_t) * (size_t)chunk));
    HIPCHK(dOrbitStop.alloc(sizeof(int32_t) * (size_t)chunk));
    HIPCHK(dOrbit.alloc(perInstance * (size_t)chunk));
    csim::PssArgs& wa = wk.args;

    csim::PnoiseArgs a{};
    a.params = d_params; a.B = B; a.dt = p.tstep; a.K = (int)p.K; a.M = p.nSide; a.F = F;
    a.twc = wa.twc; a.tws = wa.tws;
    a.x0 = d_x0; a.orbit = dOrbit.as<double>(); a.wStatus = wa.status;
    a.outP = p.outP; a.outM = p.outM;
    a.S = eng->nNoiseSrc; a.srcElem = eng->dNoiseElem; a.srcA = eng->dNoiseA; a.srcB = eng->dNoiseB;
    a.inA = p.inA; a.inB = p.inB; a.kT4 = p.kT4;
    a.gK = dGk.as<double>();
    a.onoise = d_onoise; a.gain = d_gain; a.contrib = d_contrib; a.side = d_side;
    a.orbitStop = dOrbitStop.as<int32_t>(); a.stop = dStop.as<int32_t>(); a.status = d_status;

    csim::PeriodCloseArgs cl{};
    cl.W = wa.W; cl.v = a.gK; cl.stop = a.stop; cl.status = d_status; cl.transposeW = true;

    // The scratch above lives until the stream has drained: the one exit below comes after a synchronisation.
    hipError_t e = hipSuccess;
    for (int b0 = 0; b0 < B && e == hipSuccess; b0 += chunk) {
        wa.b0 = a.b0 = cl.b0 = b0;
        wa.Bc = a.Bc = cl.Bc = std::min(chunk, B - b0);
        e = csim::launchPssPeriod(eng->gpTran, wa, hs);
        if (e == hipSuccess) e = hipMemsetAsync(dOrbitStop.p, 0, sizeof(int32_t) * (size_t)a.Bc, hs);
        if (e == hipSuccess) e = csim::launchPnoiseOrbit(eng->gpTran, a, hs);
        for (int f0i = 0; f0i < F && e == hipSuccess; f0i += Fc) {
            a.fFirst = f0i;
            a.Fc = cl.Fc = std::min(Fc, F - f0i);
            a.zr = wk.dZ.as<double>() + f0i; a.zi = a.zr + F; cl.zKr = a.zi + F; cl.zKi = cl.zKr + F;
            e = hipMemsetAsync(dStop.p, 0, sizeof(int32_t) * (size_t)a.Bc, hs);
            a.g0 = nullptr;
            if (e == hipSuccess) e = csim::launchPnoisePeriod(eng->gpTran, a, hs);
            if (e == hipSuccess) e = csim::launchPeriodClose(eng->gpTran, cl, hs);
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
    const int nF = (int)p.freqs.size(), nSb = 2 * p.nSide + 1, S = eng->nNoiseSrc;
    csim::PeriodHostState s;
    DevBuf dOn, dGain, dCon, dSide;
    HIPCHK(dOn.alloc(sizeof(double) * (size_t)nF * B));
    if (gain) HIPCHK(dGain.alloc(sizeof(double) * 2 * (size_t)nF * nSb * B));
    if (contrib) HIPCHK(dCon.alloc(sizeof(double) * (size_t)nF * S * B));
    if (side) HIPCHK(dSide.alloc(sizeof(double) * (size_t)nF * nSb * B));
    if (const int rc = csim::periodHostPrologue(eng, params, B, p.tstep, p.f0, s)) return rc;
    if (const int rc = pnoiseRun(eng, p, s.dParams.as<double>(), B, s.dX.as<double>(), dOn.as<double>(), dGain.as<double>(),
                                 dCon.as<double>(), dSide.as<double>(), s.dStatus.as<uint32_t>(), nullptr)) return rc;
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
    return csim::periodHostEpilogue(eng, B, s, x0_out, rounds, status);
}

} // extern "C"
