// kernels_disto.hip -- small-signal distortion analysis: HD2 and HD3 of B instances x F frequencies by a Volterra
// series at the operating point (include/csim.h "Distortion analysis", arithmetic in ac_disto.hpp).
//
// The system of an instance is the one ac_assemble_kernel leaves (G, C column-major, J).  Three kernels:
//
//   disto_coef_kernel        one thread per (MOSFET, instance), ONCE per instance: the seven derivatives of the drain
//                            current at x_op (disto_coef), region decided as mos_eval decides it.
//   ac_disto_wave_kernel     one wavefront per instance, N <= 63
//   ac_disto_packed_kernel   N <= 32: 32 lanes per instance
//
// The two sweep kernels are the bodies of ac_chain.hpp (the device round, the solves, the layout in LDS) on the chain
// below: three solves at w, 2 w and 3 w; x1 and x2 are kept for the currents, x3 stays in the solution.
#include <hip/hip_runtime.h>

#include "ac_chain.hpp"

namespace csim {

#pragma clang fp contract(off)

namespace {

__global__ void __launch_bounds__(256) disto_coef_kernel(GenPlan pl, const int32_t* __restrict__ devElem, int M,
                                                         const double* __restrict__ params, int B, int b0, int Bc,
                                                         const double* __restrict__ xop, double* __restrict__ coef,
                                                         size_t coefStride, size_t coefOff)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)M * (size_t)Bc) return;
    const int m = (int)(t / (size_t)Bc), c = (int)(t - (size_t)m * (size_t)Bc);
    const size_t b = (size_t)b0 + (size_t)c;
    const int e = devElem[m];
    const int kind = pl.kind[e], slot = pl.slot[e];
    auto P = [&](int p) { return params[(size_t)(slot + p) * (size_t)B + b]; };
    auto X = [&](int eq) { return eq >= 0 ? xop[(size_t)eq * (size_t)B + b] : 0.0; };
    const int32_t* q = pl.eq + 4 * e;
    const DistoCoef r = disto_coef(kind == CSIM_PMOS, P(0), P(1), P(2), X(q[0]), X(q[1]), X(q[2]));
#pragma unroll
    for (int k = 0; k < DISTO_NCOEF; ++k) coef[((size_t)m * DISTO_NCOEF + k) * coefStride + coefOff + (size_t)c] = r.c[k];
}

// solve k = 0 .. 2 is order k + 1
struct DistoChain {
    enum { NSOLVE = 3, NTONE = 1, NKEPT = 2, NRATIO = 2 };
    static constexpr int slot(int k) { return k < 2 ? k : -1; }
    static constexpr int numerator(int q) { return q + 1; }                    // HD2 = |v2| / |v1|, HD3 = |v3| / |v1|
    static __device__ __forceinline__ double freq(int k, double w, double) { return (double)(k + 1) * w; }
    static __device__ __forceinline__ cpx current(int k, const double* cf, int d, int g, int s, const double* K, int stride)
    {
        const cpx Ug = disto_u(K, K + stride, g, s), Ud = disto_u(K, K + stride, d, s);
        if (k == 1) return disto_i2(cf, Ug, Ud);
        return disto_i3(cf, Ug, Ud, disto_u(K + 2 * stride, K + 3 * stride, g, s), disto_u(K + 2 * stride, K + 3 * stride, d, s));
    }
};

__global__ void __launch_bounds__(64) ac_disto_wave_kernel(ChainArgs a) { chain_wave<DistoChain>(a); }

template <int NP>
__global__ void __launch_bounds__(64) ac_disto_packed_kernel(ChainArgs a) { chain_packed<DistoChain, NP>(a); }

} // namespace

hipError_t launchDistoCoef(const GenPlan& pl, const int32_t* dDevElem, int M, const double* dParams, int B, int b0, int Bc,
                           const double* dXop, double* dCoef, size_t coefStride, size_t coefOff, hipStream_t stream)
{
    if (Bc <= 0 || M <= 0) return hipSuccess;
    const size_t total = (size_t)M * (size_t)Bc;
    hipLaunchKernelGGL(disto_coef_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, pl, dDevElem, M, dParams,
                       B, b0, Bc, dXop, dCoef, coefStride, coefOff);
    return hipGetLastError();
}

hipError_t launchDistoSweep(int which, const ChainArgs& a, const int32_t* hostD, const int32_t* hostG, const int32_t* hostS,
                            hipStream_t stream)
{
    return launchChainSweep<DistoChain>(which, a, hostD, hostG, hostS, stream, ac_disto_wave_kernel,
                                        [](auto np) { return ac_disto_packed_kernel<decltype(np)::value>; });
}

} // namespace csim
