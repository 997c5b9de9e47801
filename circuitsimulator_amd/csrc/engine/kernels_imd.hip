// kernels_imd.hip -- two-tone intermodulation analysis: IM2+, IM2- and IM3 of B instances x F tone pairs by a Volterra
// series at the operating point (include/csim.h "Intermodulation analysis", arithmetic in ac_imd.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major, J); the coefficients are those of
// disto_coef_kernel (kernels_disto.hip).  Two kernels:
//
//   ac_imd_wave_kernel     one wavefront per instance, N <= 63
//   ac_imd_packed_kernel   N <= 32: 32 lanes per instance
//
// Both are the bodies of ac_chain.hpp (the device round, the solves, the layout in LDS) on the chain below: six solves,
// k = 0 .. 5 at w1, w2, w1 + w2, w1 - w2, 2 w1 and 2 w1 - w2; x0, x1, x3 and x4 are kept for the currents, x2 is only
// written out (|v2| is taken on the way), x5 stays in the solution.
#include <hip/hip_runtime.h>

#include "ac_chain.hpp"
#include "ac_imd.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

struct ImdChain {
    enum { NSOLVE = IMD_NSOLVE, NTONE = 2, NKEPT = 4, NRATIO = IMD_NRATIO };
    static constexpr int slot(int k) { return k == 2 || k == 5 ? -1 : (k < 2 ? k : k - 1); }      // x0, x1, x3, x4 -> 0 .. 3
    static constexpr int numerator(int q) { return q == 0 ? 2 : (q == 1 ? 3 : 5); }                // IM2+, IM2-, IM3
    static __device__ __forceinline__ double freq(int k, double w1, double w2) { return imd_freq(k, w1, w2); }
    static __device__ __forceinline__ cpx current(int k, const double* cf, int d, int g, int s, const double* K, int stride)
    {
        return imd_current(k, cf, d, g, s, K, K + stride, K + 2 * stride, K + 3 * stride, K + 4 * stride, K + 5 * stride,
                           K + 6 * stride, K + 7 * stride);
    }
};

__global__ void __launch_bounds__(64) ac_imd_wave_kernel(ChainArgs a) { chain_wave<ImdChain>(a); }

template <int NP>
__global__ void __launch_bounds__(64) ac_imd_packed_kernel(ChainArgs a) { chain_packed<ImdChain, NP>(a); }

} // namespace

hipError_t launchImdSweep(int which, const ChainArgs& a, const int32_t* hostD, const int32_t* hostG, const int32_t* hostS,
                          hipStream_t stream)
{
    return launchChainSweep<ImdChain>(which, a, hostD, hostG, hostS, stream, ac_imd_wave_kernel,
                                      [](auto np) { return ac_imd_packed_kernel<decltype(np)::value>; });
}

} // namespace csim
