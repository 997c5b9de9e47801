// engine_pac.cpp -- C-ABI of the periodic AC analysis (include/csim.h "Periodic AC analysis"): the device form
// csim_pac_batch_dev (per instance chunk one W_K launch, per frequency chunk two period passes around the closure
// solve, on the caller's stream) and the host form csim_pac_batch (DC operating point, periodic steady state, then this).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "csim.h"
#include "engine_host.hpp"
#include "kernels.hpp"
#include "pac.hpp"
#include "pss.hpp"

using csim::setError;

namespace {

// what a call asks for, after the defaults: refused here, before anything looks at the device
struct PacPlan {
    double tstep, f0;
    int nSide, nProbe, Fc;
    int64_t K;
    std::vector<double> freqs;
};

int pacResolve(const csim_engine* eng, const char* who, bool cardDefaults, double tstep, double f0, const double* freqs,
               int F, int n_side, const int32_t* probe_eq, int n_probe, PacPlan& p)
{
    const std::string w(who);
    if (std::isnan(tstep) || std::isinf(tstep) || std::isnan(f0) || std::isinf(f0)) {
        setError(w + ": tstep and f0 must be finite");
        return CSIM_ERR_ARG;
    }
    if ((probe_eq && n_probe < 0) || F < 0 || (F > 0 && !freqs)) { setError(w + ": bad argument"); return CSIM_ERR_ARG; }
    if (n_side < 0) { setError(w + ": n_side must be >= 0"); return CSIM_ERR_ARG; }
    if (const int rc = csim::periodResolveFreqs(w, cardDefaults, eng->cards.pac, ".PAC", freqs, F, p.freqs)) return rc;
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
    if (!eng->acAnySource) { setError(w + ": no source of the netlist has an AC magnitude"); return CSIM_ERR_CONFIG; }
    const int N = eng->plan.N;
    if (N > 63) { setError("periodic AC analysis covers circuits of up to 63 unknowns"); return CSIM_ERR_UNSUPPORTED; }
    if (probe_eq)
        for (int i = 0; i < n_probe; ++i)
            if (probe_eq[i] < 0 || probe_eq[i] >= N) { setError(w + ": probe equation index out of range"); return CSIM_ERR_ARG; }
    p.tstep = tstep;
    p.f0 = f0;
    p.nSide = n_side;
    p.K = K;
    p.nProbe = probe_eq ? n_probe : N;
    p.Fc = csim::pacMaxFc(eng->gpTran, p.nSide, p.nProbe);
    if (p.Fc < 1) {
        setError(w + ": the sideband sums of " + std::to_string(p.nProbe) + " probes and " + std::to_string(2 * n_side + 1) +
                 " sidebands do not fit the LDS at one frequency per launch");
        return CSIM_ERR_CONFIG;
    }
    return CSIM_OK;
}

int pacRun(csim_engine* eng, const PacPlan& p, const double* d_params, int B, const int32_t* probe_eq, const double* d_x0,
           double* d_out, uint32_t* d_status, hipStream_t hs)
{
    const int N = eng->plan.N, F = (int)p.freqs.size(), Fc = p.Fc;
    const int chunk = csim::pssChunk(eng, B);

    csim::PeriodWk wk;
    DevBuf dProbe, dPk, dStop;
    if (const int rc = csim::periodWkSetup(wk, eng, d_params, B, chunk, p.tstep, p.f0, p.K, p.freqs, d_x0, hs)) return rc;
    if (probe_eq && p.nProbe > 0) {
        HIPCHK(dProbe.alloc(sizeof(int32_t) * (size_t)p.nProbe));
        HIPCHK(hipMemcpy(dProbe.p, probe_eq, sizeof(int32_t) * (size_t)p.nProbe, hipMemcpyHostToDevice));
    }
    HIPCHK(dPk.alloc(sizeof(double) * (size_t)N * 2 * (size_t)Fc * (size_t)chunk));
    HIPCHK(dStop.alloc(sizeof(int32_t) * (size_t)chunk));
    csim::PssArgs& wa = wk.args;

    csim::PacArgs a{};
    a.params = d_params; a.B = B; a.dt = p.tstep; a.K = (int)p.K; a.M = p.nSide; a.F = F;
    a.probeEq = (probe_eq && p.nProbe > 0) ? dProbe.as<int32_t>() : nullptr; a.nProbe = p.nProbe;
    a.twc = wa.twc; a.tws = wa.tws;
    a.acRe = eng->dAcRe; a.acIm = eng->dAcIm;
    a.x0 = d_x0; a.wStatus = wa.status;
    a.pK = dPk.as<double>(); a.stop = dStop.as<int32_t>(); a.status = d_status;

    csim::PeriodCloseArgs cl{};
    cl.W = wa.W; cl.v = a.pK; cl.stop = a.stop; cl.status = d_status; cl.transposeW = false;

    // The scratch above lives until the stream has drained: the one exit below comes after a synchronisation.
    hipError_t e = hipSuccess;
    for (int b0 = 0; b0 < B && e == hipSuccess; b0 += chunk) {
        wa.b0 = a.b0 = cl.b0 = b0;
        wa.Bc = a.Bc = cl.Bc = std::min(chunk, B - b0);
        e = csim::launchPssPeriod(eng->gpTran, wa, hs);
        for (int f0i = 0; f0i < F && e == hipSuccess; f0i += Fc) {
            a.fFirst = f0i;
            a.Fc = cl.Fc = std::min(Fc, F - f0i);
            a.zr = wk.dZ.as<double>() + f0i; a.zi = a.zr + F; cl.zKr = a.zi + F; cl.zKi = cl.zKr + F;
            e = hipMemsetAsync(dStop.p, 0, sizeof(int32_t) * (size_t)a.Bc, hs);
            a.p0 = nullptr; a.out = nullptr;
            if (e == hipSuccess) e = csim::launchPacPeriod(eng->gpTran, a, hs);
            if (e == hipSuccess) e = csim::launchPeriodClose(eng->gpTran, cl, hs);
            a.p0 = a.pK; a.out = d_out;
            if (e == hipSuccess) e = csim::launchPacPeriod(eng->gpTran, a, hs);
        }
    }
    const hipError_t es = hipStreamSynchronize(hs);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { setError(std::string("csim_pac_batch_dev: ") + hipGetErrorString(e)); return CSIM_ERR_HIP; }
    return CSIM_OK;
}

} // namespace

extern "C" {

int csim_pac_batch_dev(csim_engine* eng, const double* d_params, int32_t B, double tstep, double f0, const double* d_x0,
                       const double* freqs, int32_t F, int32_t n_side, const int32_t* probe_eq, int32_t n_probe,
                       double* d_out, uint32_t* d_status, void* stream)
{
    if (!eng || !d_params || !d_x0 || !freqs || !d_out || !d_status || B <= 0 || F <= 0) {
        setError("csim_pac_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    PacPlan p{};
    if (const int rc = pacResolve(eng, "csim_pac_batch_dev", false, tstep, f0, freqs, F, n_side, probe_eq, n_probe, p)) return rc;
    HIPCHK(hipSetDevice(eng->device));
    return pacRun(eng, p, d_params, B, probe_eq, d_x0, d_out, d_status, static_cast<hipStream_t>(stream));
}

int csim_pac_batch(csim_engine* eng, const double* params, int32_t B, double tstep, double f0, const double* freqs,
                   int32_t F, int32_t n_side, const int32_t* probe_eq, int32_t n_probe, double* out, double* x0_out,
                   int32_t* rounds, uint32_t* status)
{
    if (!eng || !out || B <= 0) { setError("csim_pac_batch: bad argument"); return CSIM_ERR_ARG; }
    PacPlan p{};
    if (const int rc = pacResolve(eng, "csim_pac_batch", true, tstep, f0, freqs, F, n_side, probe_eq, n_probe, p)) return rc;
    HIPCHK(hipSetDevice(eng->device));
    const int nF = (int)p.freqs.size(), S = 2 * p.nSide + 1;
    const size_t per = (size_t)nF * S * p.nProbe;
    csim::PeriodHostState s;
    DevBuf dOut;
    HIPCHK(dOut.alloc(sizeof(double) * 2 * per * B));
    if (const int rc = csim::periodHostPrologue(eng, params, B, p.tstep, p.f0, s)) return rc;
    if (const int rc = pacRun(eng, p, s.dParams.as<double>(), B, probe_eq, s.dX.as<double>(), dOut.as<double>(),
                              s.dStatus.as<uint32_t>(), nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    // [F][S][nProbe][B] complex -> [B][F][S][nProbe] complex
    std::vector<double> h(2 * per * B);
    HIPCHK(hipMemcpy(h.data(), dOut.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < per; ++e)
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 2; ++k) out[2 * ((size_t)b * per + e) + k] = h[2 * (e * B + b) + k];
    return csim::periodHostEpilogue(eng, B, s, x0_out, rounds, status);
}

} // extern "C"
