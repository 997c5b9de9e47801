// engine_host.hpp -- what the translation units of the C-ABI (engine.cpp, engine_freq.cpp) share besides the handle
// (library-private).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "csim.h"
#include "engine_internal.hpp"
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

} // namespace csim
