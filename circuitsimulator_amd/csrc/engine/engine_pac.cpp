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
    if (F == 0) {
        if (!cardDefaults || freqs || !eng->pacEnabled) { setError(w + ": no frequencies given and no .PAC card to take them from"); return CSIM_ERR_ARG; }
        const int64_t n = csim_ac_num_freqs(eng->pacSweep, eng->pacPoints, eng->pacFstart, eng->pacFstop);
        if (n < 0) return (int)n;
        p.freqs.resize((size_t)n);
        if (const int rc = csim_ac_freqs(eng->pacSweep, eng->pacPoints, eng->pacFstart, eng->pacFstop, p.freqs.data())) return rc;
    } else {
        p.freqs.assign(freqs, freqs + F);
    }
    for (const double f : p.freqs)
        if (!std::isfinite(f) || !(f > 0.0)) { setError(w + ": every frequency must be finite and positive"); return CSIM_ERR_ARG; }
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

    std::vector<double> tw(2 * (size_t)p.K);
    csim::pss_twiddles(p.K, tw.data(), tw.data() + p.K);
    std::vector<double> z(4 * (size_t)F);                   // zr, zi, zKr, zKi, [F] each
    for (int f = 0; f < F; ++f) csim::pac_z(p.freqs[(size_t)f], p.tstep, p.f0, &z[f], &z[F + f], &z[2 * F + f], &z[3 * F + f]);

    DevBuf dTw, dZ, dProbe, dXk, dW, dDone, dWst, dPk, dStop;
    HIPCHK(dTw.alloc(sizeof(double) * tw.size()));
    HIPCHK(hipMemcpy(dTw.p, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice));
    HIPCHK(dZ.alloc(sizeof(double) * z.size()));
    HIPCHK(hipMemcpy(dZ.p, z.data(), sizeof(double) * z.size(), hipMemcpyHostToDevice));
    if (probe_eq && p.nProbe > 0) {
        HIPCHK(dProbe.alloc(sizeof(int32_t) * (size_t)p.nProbe));
        HIPCHK(hipMemcpy(dProbe.p, probe_eq, sizeof(int32_t) * (size_t)p.nProbe, hipMemcpyHostToDevice));
    }
    HIPCHK(dXk.alloc(sizeof(double) * (size_t)N * (size_t)B));
    HIPCHK(dW.alloc(sizeof(double) * (size_t)N * (size_t)N * (size_t)chunk));
    HIPCHK(dDone.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dWst.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(dPk.alloc(sizeof(double) * (size_t)N * 2 * (size_t)Fc * (size_t)chunk));
    HIPCHK(dStop.alloc(sizeof(int32_t) * (size_t)chunk));
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

    csim::PacArgs a{};
    a.params = d_params; a.B = B; a.dt = p.tstep; a.K = (int)p.K; a.M = p.nSide; a.F = F;
    a.probeEq = (probe_eq && p.nProbe > 0) ? dProbe.as<int32_t>() : nullptr; a.nProbe = p.nProbe;
    a.twc = wa.twc; a.tws = wa.tws;
    a.acRe = eng->dAcRe; a.acIm = eng->dAcIm;
    a.x0 = d_x0; a.W = dW.as<double>(); a.wStatus = dWst.as<uint32_t>();
    a.pK = dPk.as<double>(); a.stop = dStop.as<int32_t>(); a.status = d_status;

    // The scratch above lives until the stream has drained: the one exit below comes after a synchronisation.
    hipError_t e = hipSuccess;
    for (int b0 = 0; b0 < B && e == hipSuccess; b0 += chunk) {
        wa.b0 = a.b0 = b0;
        wa.Bc = a.Bc = std::min(chunk, B - b0);
        e = csim::launchPssPeriod(eng->gpTran, wa, hs);
        for (int f0i = 0; f0i < F && e == hipSuccess; f0i += Fc) {
            a.fFirst = f0i;
            a.Fc = std::min(Fc, F - f0i);
            a.zr = dZ.as<double>() + f0i; a.zi = a.zr + F; a.zKr = a.zi + F; a.zKi = a.zKr + F;
            e = hipMemsetAsync(dStop.p, 0, sizeof(int32_t) * (size_t)a.Bc, hs);
            a.p0 = nullptr; a.out = nullptr;
            if (e == hipSuccess) e = csim::launchPacPeriod(eng->gpTran, a, hs);
            if (e == hipSuccess) e = csim::launchPacClose(eng->gpTran, a, hs);
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
    const int N = eng->plan.N, nF = (int)p.freqs.size(), S = 2 * p.nSide + 1;
    const size_t per = (size_t)nF * S * p.nProbe;
    DevBuf dParams, dX, dIters, dStatus, dHarm, dRounds, dOut;
    if (const int rc = csim::stageParams(eng, params, B, dParams)) return rc;
    HIPCHK(dX.alloc(sizeof(double) * (size_t)N * B));
    HIPCHK(dIters.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dStatus.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(dHarm.alloc(sizeof(double) * 2));
    HIPCHK(dRounds.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dOut.alloc(sizeof(double) * 2 * per * B));
    if (const int rc = csim_dc_batch_dev(eng, dParams.as<double>(), B, dX.as<double>(), dIters.as<int32_t>(),
                                         dStatus.as<uint32_t>(), nullptr)) return rc;
    // the steady state with no harmonics stored: an empty probe list
    const int32_t none = 0;
    if (const int rc = csim_pss_batch_dev(eng, dParams.as<double>(), B, p.tstep, p.f0, 0, &none, 0, 0.0, 0, dX.as<double>(),
                                          dHarm.as<double>(), dRounds.as<int32_t>(), dStatus.as<uint32_t>(), nullptr)) return rc;
    if (const int rc = pacRun(eng, p, dParams.as<double>(), B, probe_eq, dX.as<double>(), dOut.as<double>(),
                              dStatus.as<uint32_t>(), nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    // [F][S][nProbe][B] complex -> [B][F][S][nProbe] complex, [N][B] -> [B][N]
    std::vector<double> h(2 * per * B);
    HIPCHK(hipMemcpy(h.data(), dOut.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < per; ++e)
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 2; ++k) out[2 * ((size_t)b * per + e) + k] = h[2 * (e * B + b) + k];
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
