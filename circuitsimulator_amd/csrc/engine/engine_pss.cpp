// engine_pss.cpp -- C-ABI of the periodic-steady-state analysis (include/csim.h "Periodic steady state"): the device
// form csim_pss_batch_dev (shooting rounds on the caller's stream, one counter read back per round), the host form
// csim_pss_batch (DC operating point first) and the two helpers that give a test the library's own K and table; and
// what the periodic AC and noise analyses share with it on the host (engine_host.hpp): the resolve blocks, the W_K
// launch's scratch, the host forms' prologue and epilogue.
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
        if (!eng->cards.hb.enabled) { setError(w + ": no f0 given and the netlist has no .HB card"); return CSIM_ERR_CONFIG; }
        f0 = eng->cards.hb.f0;
        n_harm = eng->cards.hb.nHarm;
        if (n_harm < 0) { setError(w + ": the .HB card's harmonic count is negative"); return CSIM_ERR_CONFIG; }
    }
    int64_t K = 0;
    if (const int rc = csim::periodResolveSteps(eng, w, cardDefaults, tstep, f0, K)) return rc;
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

int csim::periodResolveSteps(const csim_engine* eng, const std::string& w, bool cardDefaults, double& tstep, double f0, int64_t& K)
{
    if (cardDefaults && !(tstep > 0.0)) {
        if (!eng->cards.tran.enabled) { setError(w + ": no tstep given and the netlist has no .TRAN card"); return CSIM_ERR_CONFIG; }
        tstep = eng->cards.tran.tstep;
    }
    if (!(f0 > 0.0)) { setError(w + ": no f0 given"); return CSIM_ERR_CONFIG; }
    K = csim::pss_num_steps(tstep, f0);
    if (K < 0) {
        setError(w + ": the period 1/f0 must be a whole number of steps, at most 2^22 (|K tstep f0 - 1| <= 1e-9)");
        return (int)K;
    }
    return CSIM_OK;
}

int csim::periodResolveFreqs(const std::string& w, bool cardDefaults, const SweepGrid& card, const char* cardName,
                             const double* freqs, int F, std::vector<double>& out)
{
    if (F == 0) {
        if (!cardDefaults || freqs || !card.enabled) {
            setError(w + ": no frequencies given and no " + cardName + " card to take them from");
            return CSIM_ERR_ARG;
        }
        const int64_t n = csim_ac_num_freqs(card.sweep, card.points, card.fstart, card.fstop);
        if (n < 0) return (int)n;
        out.resize((size_t)n);
        if (const int rc = csim_ac_freqs(card.sweep, card.points, card.fstart, card.fstop, out.data())) return rc;
    } else {
        out.assign(freqs, freqs + F);
    }
    for (const double f : out)
        if (!std::isfinite(f) || !(f > 0.0)) { setError(w + ": every frequency must be finite and positive"); return CSIM_ERR_ARG; }
    return CSIM_OK;
}

int csim::periodWkSetup(PeriodWk& wk, const csim_engine* eng, const double* d_params, int B, int chunk, double tstep, double f0,
                        int64_t K, const std::vector<double>& freqs, const double* d_x0, hipStream_t hs)
{
    const int N = eng->plan.N;
    const size_t F = freqs.size();
    std::vector<double> tw(2 * (size_t)K);
    csim::pss_twiddles(K, tw.data(), tw.data() + K);
    std::vector<double> z(4 * F);                           // zr, zi, zKr, zKi, [F] each
    for (size_t f = 0; f < F; ++f) csim::pac_z(freqs[f], tstep, f0, &z[f], &z[F + f], &z[2 * F + f], &z[3 * F + f]);

    HIPCHK(wk.dTw.alloc(sizeof(double) * tw.size()));
    HIPCHK(hipMemcpy(wk.dTw.p, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice));
    HIPCHK(wk.dZ.alloc(sizeof(double) * z.size()));
    HIPCHK(hipMemcpy(wk.dZ.p, z.data(), sizeof(double) * z.size(), hipMemcpyHostToDevice));
    HIPCHK(wk.dXk.alloc(sizeof(double) * (size_t)N * (size_t)B));
    HIPCHK(wk.dW.alloc(sizeof(double) * (size_t)N * (size_t)N * (size_t)chunk));
    HIPCHK(wk.dDone.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(wk.dWst.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(hipMemsetAsync(wk.dDone.p, 0, sizeof(int32_t) * (size_t)B, hs));
    HIPCHK(hipMemsetAsync(wk.dWst.p, 0, sizeof(uint32_t) * (size_t)B, hs));

    csim::PssArgs& wa = wk.args;
    wa.params = d_params; wa.B = B; wa.dt = tstep; wa.K = (int)K; wa.H = 0;
    wa.probeEq = nullptr; wa.nProbe = 0;
    wa.twc = wk.dTw.as<double>(); wa.tws = wk.dTw.as<double>() + K;
    wa.x0 = const_cast<double*>(d_x0);                      // the period kernel reads it only
    wa.xK = wk.dXk.as<double>(); wa.harm = nullptr; wa.W = wk.dW.as<double>();
    wa.status = wk.dWst.as<uint32_t>(); wa.done = wk.dDone.as<int32_t>();
    return CSIM_OK;
}

int csim::periodHostPrologue(csim_engine* eng, const double* params, int B, double tstep, double f0, PeriodHostState& h)
{
    const int N = eng->plan.N;
    if (const int rc = csim::stageParams(eng, params, B, h.dParams)) return rc;
    HIPCHK(h.dX.alloc(sizeof(double) * (size_t)N * B));
    HIPCHK(h.dIters.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(h.dStatus.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(h.dHarm.alloc(sizeof(double) * 2));
    HIPCHK(h.dRounds.alloc(sizeof(int32_t) * (size_t)B));
    if (const int rc = csim_dc_batch_dev(eng, h.dParams.as<double>(), B, h.dX.as<double>(), h.dIters.as<int32_t>(),
                                         h.dStatus.as<uint32_t>(), nullptr)) return rc;
    // the steady state with no harmonics stored: an empty probe list
    const int32_t none = 0;
    return csim_pss_batch_dev(eng, h.dParams.as<double>(), B, tstep, f0, 0, &none, 0, 0.0, 0, h.dX.as<double>(),
                              h.dHarm.as<double>(), h.dRounds.as<int32_t>(), h.dStatus.as<uint32_t>(), nullptr);
}

int csim::periodHostEpilogue(const csim_engine* eng, int B, PeriodHostState& h, double* x0_out, int32_t* rounds, uint32_t* status)
{
    const int N = eng->plan.N;
    if (x0_out) {                                           // [N][B] -> [B][N]
        std::vector<double> x((size_t)N * B);
        HIPCHK(hipMemcpy(x.data(), h.dX.p, sizeof(double) * x.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i)
            for (int b = 0; b < B; ++b) x0_out[(size_t)b * N + i] = x[(size_t)i * B + b];
    }
    if (rounds) HIPCHK(hipMemcpy(rounds, h.dRounds.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, h.dStatus.p, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost));
    return CSIM_OK;
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
    csim::PeriodHostState s;                                // as periodHostPrologue, but with the harmonics asked for
    if (const int rc = csim::stageParams(eng, params, B, s.dParams)) return rc;
    HIPCHK(s.dX.alloc(sizeof(double) * (size_t)N * B));
    HIPCHK(s.dIters.alloc(sizeof(int32_t) * (size_t)B));
    HIPCHK(s.dStatus.alloc(sizeof(uint32_t) * (size_t)B));
    HIPCHK(s.dHarm.alloc(sizeof(double) * 2 * (size_t)H1 * p.nProbe * B));
    HIPCHK(s.dRounds.alloc(sizeof(int32_t) * (size_t)B));
    if (const int rc = csim_dc_batch_dev(eng, s.dParams.as<double>(), B, s.dX.as<double>(), s.dIters.as<int32_t>(),
                                         s.dStatus.as<uint32_t>(), nullptr)) return rc;
    if (const int rc = csim_pss_batch_dev(eng, s.dParams.as<double>(), B, p.tstep, p.f0, p.nHarm, probe_eq, n_probe, p.tol,
                                          p.maxRounds, s.dX.as<double>(), s.dHarm.as<double>(), s.dRounds.as<int32_t>(),
                                          s.dStatus.as<uint32_t>(), nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    // [H+1][nProbe][B] complex -> [B][H+1][nProbe] complex
    std::vector<double> h(2 * (size_t)H1 * p.nProbe * B);
    HIPCHK(hipMemcpy(h.data(), s.dHarm.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < (size_t)H1 * p.nProbe; ++e)
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 2; ++k) harm_out[2 * ((size_t)b * H1 * p.nProbe + e) + k] = h[2 * (e * B + b) + k];
    return csim::periodHostEpilogue(eng, B, s, x0_out, rounds, status);
}

} // extern "C"
