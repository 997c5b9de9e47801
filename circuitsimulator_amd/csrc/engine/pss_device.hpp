// pss_device.hpp -- device functions the period kernels of the periodic steady state (kernels_pss.hip) and of the
// periodic AC analysis (kernels_pac.hip) share: the finiteness vote, the right-hand side alone, and the history terms
// with every source at zero (what Hm = d(right-hand side)/d(x_prev) is differenced from).
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.hpp"

namespace csim {

namespace {

__device__ __forceinline__ bool pss_all_finite(double v, int N, int lane)
{
    const bool bad = (lane < N) && !isfinite(v);
    return __ballot(bad) == 0ull;
}

// the right-hand side alone, as assemble() forms it: out[0 .. N-1]
__device__ __forceinline__ void pss_rhs(const GenPlan& pl, const double* T, double* out, int lane)
{
    if (lane < pl.N) out[lane] = 0.0;
    wave_sync();
    for (int n = lane; n < pl.nnzI; n += 64) {
        double acc = 0.0;
        for (int c = pl.iPtr[n]; c < pl.iPtr[n + 1]; ++c) {
            const int con = pl.iCon[c];
            const double v = T[con >> 1];
            acc = (con & 1) ? acc - v : acc + v;
        }
        out[pl.iRow[n]] = acc;
    }
    wave_sync();
}

// the history terms at xp with every source at zero
__device__ __forceinline__ void pss_terms_history(const GenPlan& pl, const double* Pv, double* T, const double* xp, int lane)
{
    terms_step_tran(pl, Pv, T, xp, 0.0, lane);
    wave_sync();
    for (int e = lane; e < pl.nElem; e += 64) {
        const int kind = pl.kind[e];
        if (kind == CSIM_V || kind == CSIM_I) T[pl.termBase[e] + T_SRC_VAL] = 0.0;
    }
    wave_sync();
}

} // namespace

} // namespace csim
