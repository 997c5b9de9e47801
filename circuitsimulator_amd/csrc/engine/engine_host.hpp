// engine_host.hpp -- what the translation units of the C-ABI (engine.cpp, engine_freq.cpp) share besides the handle
// (library-private).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "csim.h"
#include "engine_internal.hpp"
#include "kernels.hpp"
#include "netlist_internal.hpp"

#define HIPCHK(call)                                                                   \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            csim::setError(std::string(#call) + ": " + hipGetErrorString(e_));         \
            return CSIM_ERR_HIP;                                                       \
        }                                                                              \
    } while (0)

// scratch allocation that frees itself
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    template <class T> T* as() { return static_cast<T*>(p); }
};

namespace csim {

// host parameters [B][P] (null: the nominal values, B times) -> [P][B] on the device (engine.cpp)
int stageParams(csim_engine* eng, const double* params, int B, DevBuf& dParams);

// most instances per chunk of the frequency-domain sweeps, csim_engine_stat("ac_chunk") (engine_freq.cpp)
size_t acChunkCap(const csim_engine* eng);

// the checks of a noise call (output pair, input source element or -1, temperature; engine_freq.cpp) -> the input's
// unit excitation y(inA) - y(inB) (-1: none or ground) and 4 k_B T; the periodic noise analysis refuses what .NOISE does
int noiseResolve(const csim_engine* eng, int out_p, int out_m, int src_elem, double temp_k, int* inA, int* inB, double* kT4);

// instances per chunk of the W_K scratch of the periodic steady state and the periodic AC analysis: the option
// pss_chunk, else the sweeps' chunk (engine_pss.cpp)
int pssChunk(const csim_engine* eng, int B);

// ---- what the periodic analyses (engine_pss.cpp, engine_pac.cpp, engine_pnoise.cpp) share; all in engine_pss.cpp

// tstep from the .TRAN card when cardDefaults and none is given, the f0 check, K = the steps per period.  `who` heads
// the messages.
int periodResolveSteps(const csim_engine* eng, const std::string& who, bool cardDefaults, double& tstep, double f0, int64_t& K);

// the frequencies of a call: the caller's F, or with F == 0 those of the .PAC or .PNOISE card (`card`, named
// `cardName` in the message); every one finite and positive
int periodResolveFreqs(const std::string& who, bool cardDefaults, const SweepGrid& card, const char* cardName,
                       const double* freqs, int F, std::vector<double>& out);

// The W_K launch of the analyses that follow a steady state: the periodic steady state's period kernel on a status word
// of its own, no harmonics, no update.  Holds on the device its scratch, the twiddle table (args.twc, args.tws) and
// zr, zi, zKr, zKi ([F] each, in this order in dZ), and the filled launch record but for b0 and Bc: W_K comes out in
// args.W, the launch's status in args.status.  The scratch must live until the stream has drained: keep the holder
// until after a synchronisation.
struct PeriodWk {
    DevBuf dTw, dZ, dXk, dW, dDone, dWst;
    PssArgs args{};
};
// allocates for chunks of `chunk` instances, uploads the tables and queues the memsets on hs
int periodWkSetup(PeriodWk& wk, const csim_engine* eng, const double* d_params, int B, int chunk, double tstep, double f0,
                  int64_t K, const std::vector<double>& freqs, const double* d_x0, hipStream_t hs);

// The host forms of the analyses that follow a steady state: the parameters staged, the DC operating point and the
// periodic steady state with no harmonics stored (prologue); x0, rounds and status copied back (epilogue, null = skip).
struct PeriodHostState { DevBuf dParams, dX, dIters, dStatus, dHarm, dRounds; };
int periodHostPrologue(csim_engine* eng, const double* params, int B, double tstep, double f0, PeriodHostState& h);
int periodHostEpilogue(const csim_engine* eng, int B, PeriodHostState& h, double* x0_out, int32_t* rounds, uint32_t* status);

} // namespace csim
