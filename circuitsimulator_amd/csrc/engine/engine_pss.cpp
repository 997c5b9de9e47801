// engine_pss.cpp -- C-ABI of the periodic-steady-state analysis (include/csim.h "Periodic steady state"): the device
// form csim_pss_batch_dev (shooting rounds on the caller's stream, one counter read back per round), the host form
// csim_pss_batch (DC operating point first) and the two helpers that give a test the library's own K and table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "csim.h"
#include "engine_host.hpp"
#include "kernels.hpp"
#include "pss.hpp"

using csim::setError;

namespace {

// what a call asks for, after the defaults: refused here, before anything looks at the device
struct PssPlan {
    double tstep, f0, tol;
    int nHarm, maxRounds, nProbe;
    int64_t K;
};

int pssResolve(const csim_engine* eng, const char* who, bool cardDefaults, double tstep, double f0, int n_harm,
               const int32_t* probe_eq, int n_probe, double tol, int max_rounds, PssPlan& p)
{
    const std::string w(who);
    if (std::isnan(tstep) || std::isinf(tstep) || std::isnan(f0) || std::isinf(f0) || std::isnan(tol) || std::isinf(tol)) {
        setError(w + ": tstep, f0 and tol must be finite");
        return CSIM_ERR_ARG;
    }
    if (probe_eq && n_probe < 0) { setError(w + ": bad argument"); return CSIM_ERR_ARG; }
    const bool fromCard = cardDefaults && !(f0 > 0.0);      // then n_harm is the card's too
    if (!fromCard && n_harm < 0) { setError(w + ": n_harm must be >= 0"); return CSIM_ERR_ARG; }
    if (fromCard) {
        if (!eng->hbEnabled) { setError(w + ": no f0 given and the netlist has no .HB card"); return CSIM_ERR_CONFIG; }
        f0 = eng->hbF0;
        n_harm = eng->hbNHarm;
        if (n_harm < 0) { setError(w + ": the .HB card's harmonic count is negative"); return CSIM_ERR_CONFIG; }
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
    if (K < 2 * (int64_t)n_harm + 1) {
        setError(w + ": " + std::to_string(K) + " steps per period cannot carry " + std::to_string(n_harm) + " harmonics (K >= 2 n_harm + 1)");
        return CSIM_ERR_CONFIG;
    }
    const int N = eng->plan.N;
    if (N > 63) { setError("periodic steady state covers circuits of up to 63 unknowns"); return CSIM_ERR_UNSUPPORTED; }
    if (probe_eq)
        for (int i = 0; i < n_probe; ++i)
            if (probe_eq[i] < 0 || probe_eq[i] >= N) { setError(w + ": probe equation index out of range"); return CSIM_ERR_ARG; }
    p.tstep = tstep;
    p.f0 = f0;
    p.nHarm = n_harm;
    p.K = K;
    p.nProbe = probe_eq ? n_probe : N;
    p.tol = tol > 0.0 ? tol : eng->cfg.pssTol;
    p.maxRounds = max_rounds > 0 ? max_rounds : eng->cfg.pssMaxRounds;
    return CSIM_OK;
}

} // namespace

int csim::pssChunk(const csim_engine* eng, int B)
{
    const size_t cap = eng->cfg.pssChunk > 0 ? (size_t)eng->cfg.pssChunk : csim::acChunkCap(eng);
    return (int)std::min<size_t>((size_t)B, cap);
}

extern "C" {

int64_t csim_pss_num_steps(double tstep, double f0)
{
    const int64_t K = csim::pss_num_steps(tstep, f0);
    if (K < 0) setError("csim_pss_num_steps: the period 1/f0 must be a whole number of steps, at most 2^22");
    return K;
}

int csim_pss_twiddles(int64_t K, double* cos_out, double* sin_out)
{
    if (K < 1 || K > csim::PSS_MAX_STEPS || !cos_out || !sin_out) { setError("csim_pss_twiddles: bad argument"); return CSIM_ERR_ARG; }
    csim::pss_twiddles(K, cos_out, sin_out);
    return CSIM_OK;
}

int csim_pss_batch_dev(csim_engine* eng, const double* d_params, int32_t B, double tstep, double f0, int32_t n_harm,
                       const int32_t* probe_eq, int32_t n_probe, double tol, int32_t max_rounds, double* d_x0,
                       double* d_harm, int32_t* d_rounds, uint32_t* d_status, void* stream)
{
    if (!eng || !d_params || !d_x0 || !d_harm || !d_rounds || !d_status || B <= 0) {
        setError("csim_pss_batch_dev: bad argument");
        return CSIM_ERR_ARG;
    }
    PssPlan p{};
    if (const int rc = pssResolve(eng, "csim_pss_batch_dev", false, tstep, f0, n_harm, probe_eq, n_probe, tol, max_rounds, p)) return rc;
    HIPCHK(hipSetDevice(eng->device));
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const int N = eng->plan.N;
    const int chunk = csim::pssChunk(eng, B);

    std::vector<double> tw(2 * (size_t)p.K);
    csim::pss_twiddles(p.K, tw.data(), tw.data() + p.K);
    DevBuf dTw, dProbe, dXk, dW, dDone, dCount;
    HIPCHK(dTw.alloc(sizeof(double) * tw.size()));
    HIPCHK(hipMemcpy(dTw.p, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice));
    if (probe_eq && n_probe > 0) {
        HIPCHK(dProbe.alloc(sizeof(int32_t) * (size_t)n_probe));
        HIPCHK(hipMemcpy(dProbe.p, probe_eq, sizeof(int32_t) * (size_t)n_probe, hipMemcpyHostToDevice));
    }
    HIPCHK(dXk.alloc(sizeof(double) * (size_t)N * (size_t)B));
    HIPCHK(dW.alloc(sizeof(double) * (size_t)N * (size_t)N * (size_t)chunk));
    HIPCHK(dDone.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dCount.alloc(sizeof(int32_t)));
    HIPCHK(hipMemsetAsync(dDone.p, 0, sizeof(int32_t) * (size_t)B, hs));
    HIPCHK(hipMemsetAsync(d_rounds, 0, sizeof(int32_t) * (size_t)B, hs));

    csim::PssArgs a{};
    a.params = d_params; a.B = B; a.dt = p.tstep; a.K = (int)p.K; a.H = p.nHarm;
    a.probeEq = probe_eq ? dProbe.as<int32_t>() : nullptr; a.nProbe = p.nProbe;
    a.twc = dTw.as<double>(); a.tws = dTw.as<double>() + p.K;
    a.tol = p.tol; a.maxRounds = p.maxRounds;
    a.x0 = d_x0; a.xK = dXk.as<double>(); a.harm = d_harm; a.W = dW.as<double>();
    a.rounds = d_rounds; a.status = d_status; a.done = dDone.as<int32_t>(); a.unfinished = dCount.as<int32_t>();

    // A round per pass; the update kernel of the last allowed round closes every instance, so the counter is zero then.
    // The scratch above lives until the stream has drained: every exit below comes after a synchronisation.
    int rc = CSIM_OK;
    for (int round = 0; round < p.maxRounds && !rc; ++round) {
        hipError_t e = hipMemsetAsync(dCount.p, 0, sizeof(int32_t), hs);
        for (int b0 = 0; b0 < B && e == hipSuccess; b0 += chunk) {
            a.b0 = b0;
            a.Bc = std::min(chunk, B - b0);
            e = csim::launchPssRound(eng->gpTran, a, hs);
        }
        int32_t left = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&left, dCount.p, sizeof(int32_t), hipMemcpyDeviceToHost, hs);
        const hipError_t es = hipStreamSynchronize(hs);
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) { setError(std::string("csim_pss_batch_dev: ") + hipGetErrorString(e)); rc = CSIM_ERR_HIP; }
        if (left == 0) break;
    }
    return rc;
}

int csim_pss_batch(csim_engine* eng, const double* params, int32_t B, double tstep, double f0, int32_t n_harm,
                   const int32_t* probe_eq, int32_t n_probe, double tol, int32_t max_rounds, double* x0_out,
                   double* harm_out, int32_t* rounds, uint32_t* status)
{
    if (!eng || !harm_out || B <= 0) { setError("csim_pss_batch: bad argument"); return CSIM_ERR_ARG; }
    PssPlan p{};
    if (const int rc = pssResolve(eng, "csim_pss_batch", true, tstep, f0, n_harm, probe_eq, n_probe, tol, max_rounds, p)) return rc;
    HIPCHK(hipSetDevice(eng->device));
    const int N = eng->plan.N, H1 = p.nHarm + 1;
    DevBuf dParams, dX, dIters, dStatus, dHarm, dRounds;
    if (const int rc = csim::stageParams(eng, params, B, dParams)) return rc;
    HIPCHK(dX.alloc(sizeof(double) * (size_t)N * B));
    HIPCHK(dIters.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(dStatus.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(dHarm.alloc(sizeof(double) * 2 * (size_t)H1 * p.nProbe * B));
    HIPCHK(dRounds.alloc(sizeof(int32_t) * (size_t)B));
    if (const int rc = csim_dc_batch_dev(eng, dParams.as<double>(), B, dX.as<double>(), dIters.as<int32_t>(),
                                         dStatus.as<uint32_t>(), nullptr)) return rc;
    if (const int rc = csim_pss_batch_dev(eng, dParams.as<double>(), B, p.tstep, p.f0, p.nHarm, probe_eq, n_probe, p.tol,
                                          p.maxRounds, dX.as<double>(), dHarm.as<double>(), dRounds.as<int32_t>(),
                                          dStatus.as<uint32_t>(), nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    // [H+1][nProbe][B] complex -> [B][H+1][nProbe] complex, [N][B] -> [B][N]
    std::vector<double> h(2 * (size_t)H1 * p.nProbe * B);
    HIPCHK(hipMemcpy(h.data(), dHarm.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < (size_t)H1 * p.nProbe; ++e)
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 2; ++k) harm_out[2 * ((size_t)b * H1 * p.nProbe + e) + k] = h[2 * (e * B + b) + k];
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
