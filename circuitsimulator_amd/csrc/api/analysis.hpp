// analysis.hpp -- the batch analysis API (C++ face of include/csim.h).
//
// Upstream's include/analysis.hpp is an empty file; here it is the home of
// what the reference does not have: DC and transient analysis of a BATCH of
// circuit instances (Monte-Carlo samples, sweep points) on the GPU.  The
// scalar entry points of dcanalysis.hpp / tanalisis.hpp are the B = 1 case of
// this class.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include <complex>

#include "circuit.hpp"
#include "csim.h"
#include "sim.hpp"

namespace csim {

struct BatchDcResult {
    std::vector<double> x;            // [B][N]
    std::vector<int32_t> iters;       // NR iterations per instance
    std::vector<uint32_t> status;     // CSIM_ST_* bits per instance
};

struct BatchTranResult {
    int64_t rows = 0;                 // rows per instance in wave
    std::vector<double> wave;         // [B][rows][n_probe] (empty if no probes)
    std::vector<double> xFinal;       // [B][N]
    std::vector<int64_t> iters;
    std::vector<uint32_t> status;
};

struct BatchAcResult {
    std::vector<double> freqs;                    // [F] Hz
    int nProbe = 0;
    std::vector<std::complex<double>> v;          // [B][F][n_probe]
    std::vector<uint32_t> status;                 // DC and AC bits (CSIM_ST_LU_TINY_PIVOT: a singular frequency)
};

struct BatchNoiseResult {
    std::vector<double> freqs;                    // [F] Hz
    int nSources = 0;                             // S noise generators (csim_netlist_noise_source order)
    std::vector<double> onoise;                   // [B][F] output noise PSD, V^2/Hz
    std::vector<std::complex<double>> gain;       // [B][F] input source -> output (empty without a source)
    std::vector<double> contrib;                  // [B][F][S] (empty unless asked for)
    std::vector<uint32_t> status;                 // DC and LU bits (CSIM_ST_LU_TINY_PIVOT: a singular frequency)
};

struct BatchSpResult {
    std::vector<double> freqs;                    // [F] Hz
    int nPorts = 0;                               // P (csim_netlist_port order)
    std::vector<std::complex<double>> y, s;       // [B][F][P][P], row i then column j (s empty unless asked for)
    std::vector<uint32_t> status;                 // DC and LU bits (CSIM_ST_LU_TINY_PIVOT: a singular frequency)
};

struct BatchSpNoiseResult {
    std::vector<double> freqs;                    // [F] Hz
    int nPorts = 0;                               // P (csim_netlist_port order)
    std::vector<std::complex<double>> y, cy;      // [B][F][P][P]: admittance, port noise-current correlation (A^2/Hz)
    std::vector<double> nf, fmin, rn;             // [B][F], linear; two ports only (empty otherwise)
    std::vector<std::complex<double>> yopt;       // [B][F]; two ports only
    std::vector<uint32_t> status;                 // DC and LU bits (CSIM_ST_LU_TINY_PIVOT: a singular frequency)
};

struct BatchDistoResult {
    std::vector<double> freqs;                    // [F] Hz
    int nDevices = 0;                             // M non-linear devices (csim_netlist_disto_device order)
    std::vector<std::complex<double>> h;          // [B][F][3][N]: the phasors of order 1, 2, 3 (empty unless asked for)
    std::vector<double> hd;                       // [B][F][2]: HD2, HD3 at the output
    std::vector<uint32_t> status;                 // DC and LU bits (CSIM_ST_LU_TINY_PIVOT: a singular order)
};

struct BatchImdResult {
    std::vector<double> freqs;                    // [F] Hz: the first tone
    double f2 = 0.0;                              // Hz: the second tone
    int nDevices = 0;                             // M non-linear devices (csim_netlist_disto_device order)
    std::vector<std::complex<double>> h;          // [B][F][6][N]: the solutions at f1, f2, f1 + f2, f1 - f2, 2 f1, 2 f1 - f2 (empty unless asked for)
    std::vector<double> im;                       // [B][F][3]: IM2+, IM2-, IM3 at the output
    std::vector<uint32_t> status;                 // DC and LU bits (CSIM_ST_LU_TINY_PIVOT: a singular solve)
};

struct BatchStbResult {
    std::vector<double> freqs;                    // [F] Hz
    std::vector<std::complex<double>> t;          // [B][F]: the loop gain
    std::vector<double> margins;                  // [B][4]: PM (degrees), fc (Hz), GM (dB), f180 (Hz); NaN where not found
    std::vector<int32_t> found;                   // [B]: bit 0 the unity crossing, bit 1 the phase crossing
    std::vector<uint32_t> status;                 // DC and LU bits (CSIM_ST_LU_TINY_PIVOT: a singular frequency, or den == 0)
};

struct BatchPzResult {
    std::vector<std::complex<double>> poles;      // [B][N]: dominant pole first, NaN beyond nPoles
    std::vector<int32_t> nPoles, nRhp;            // [B]: finite poles, and those with Re s > 0
    std::vector<double> maxRe;                    // [B]: the largest Re s, NaN without a pole
    std::vector<uint32_t> status;                 // DC bits, CSIM_ST_PZ_SINGULAR, CSIM_ST_PZ_NONCONV
};

struct BatchPssResult {
    int nHarm = 0, nProbe = 0;
    std::vector<double> x0;                       // [B][N]: the state the period starts and ends at
    std::vector<std::complex<double>> harm;       // [B][nHarm+1][nProbe]: peak phasors, cosine reference at t = 0
    std::vector<int32_t> rounds;                  // [B]: shooting rounds used
    std::vector<uint32_t> status;                 // DC and transient bits, CSIM_ST_PSS_NONCONV, CSIM_ST_PSS_SINGULAR
};

struct BatchPacResult {
    int nSide = 0, nProbe = 0;
    std::vector<double> freqs;                    // [F] Hz: the input frequencies
    std::vector<std::complex<double>> p;          // [B][F][2 nSide + 1][nProbe]: transfer to f + m f0 at index m + nSide
    std::vector<double> x0;                       // [B][N]: the start of the orbit the analysis linearised around
    std::vector<int32_t> rounds;                  // [B]: shooting rounds the steady state used
    std::vector<uint32_t> status;                 // DC, transient and steady-state bits, CSIM_ST_PAC_SINGULAR
};

struct BatchPnoiseResult {
    int nSide = 0, nSrc = 0;
    std::vector<double> freqs;                    // [F] Hz: the output frequencies
    std::vector<double> onoise;                   // [B][F] V^2/Hz
    std::vector<std::complex<double>> gain;       // [B][F][2 nSide + 1]: from f + m f0 at the source to the output at f, index m + nSide
    std::vector<double> contrib;                  // [B][F][nSrc]: per generator (csim_netlist_noise_source's order)
    std::vector<double> side;                     // [B][F][2 nSide + 1]: per sideband
    std::vector<double> x0;                       // [B][N]: the start of the orbit the analysis linearised around
    std::vector<int32_t> rounds;                  // [B]: shooting rounds the steady state used
    std::vector<uint32_t> status;                 // DC, transient and steady-state bits, CSIM_ST_PAC_SINGULAR
};

// One engine per (circuit, GPU).  Throws std::runtime_error when no HIP
// device is usable: there is no CPU path.
class BatchEngine {
public:
    // assignEquationIndices() must have run on ckt (as in src/main.cpp:34)
    explicit BatchEngine(const Circuit& ckt, int device = 0);
    ~BatchEngine();
    BatchEngine(const BatchEngine&) = delete;
    BatchEngine& operator=(const BatchEngine&) = delete;

    int numUnknowns() const { return ir_.view()->n_unknowns; }
    int numParams() const { return ir_.view()->n_params; }
    const CircuitIR& ir() const { return ir_; }
    csim_engine* handle() const { return eng_; }          // for the C-ABI entry points without a C++ wrapper
    const std::vector<double>& nominalParams() const { return ir_.nominal; }
    // Monte-Carlo table [B][P] (instance-major) for instances bFirst..bFirst+B-1
    std::vector<double> monteCarloParams(uint64_t seed, double sigma, int64_t bFirst, int B) const;

    // params: [B][P] instance-major; empty = nominal for every instance
    BatchDcResult dc(const std::vector<double>& params, int B);
    BatchTranResult tran(const std::vector<double>& params, int B, double tstep, double tstop, double tstart,
                         const std::vector<int32_t>& probeEq, int outStride);
    // AC small-signal sweep (csim_ac_batch, include/csim.h): DC operating point, then (G + jwC) v = J at every
    // frequency of freqs (Hz); probeEq empty = every unknown.
    BatchAcResult ac(const std::vector<double>& params, int B, const std::vector<double>& freqs,
                     const std::vector<int32_t>& probeEq = {});

    // Small-signal noise (csim_noise_batch, include/csim.h): DC operating point, then one adjoint solve per frequency.
    // Output V(outP) - V(outM) (equations; outM = -1: ground); srcElem: V/I element for the gain, -1 none.
    BatchNoiseResult noise(const std::vector<double>& params, int B, const std::vector<double>& freqs, int outP,
                           int outM = -1, int srcElem = -1, double tempK = 300.15, bool wantContrib = false);

    // S-parameters of the netlist's ports (csim_sp_batch, include/csim.h): DC operating point, then one factorisation
    // with one right-hand side per port and frequency; Y always, S when asked for.  freqs empty: the .SP card (an
    // error when the netlist has none).
    BatchSpResult sp(const std::vector<double>& params, int B, const std::vector<double>& freqs, bool wantS = true);

    // Two-port noise of the netlist's ports (csim_spnoise_batch, include/csim.h): DC operating point, then one
    // factorisation of the transposed system with one adjoint right-hand side per port and frequency; Y and Cy always,
    // NF / Fmin / Rn / Yopt for two ports.  freqs empty: the .SP card (an error when the netlist has none).
    BatchSpNoiseResult spNoise(const std::vector<double>& params, int B, const std::vector<double>& freqs,
                               double tempK = 300.15);

    // Single-tone harmonic distortion (csim_disto_batch, include/csim.h): DC operating point, then three factorisations
    // per frequency, at w, 2 w and 3 w.  Output V(outP) - V(outM) (equations; outM = -1: ground).
    BatchDistoResult disto(const std::vector<double>& params, int B, const std::vector<double>& freqs, int outP,
                           int outM = -1, bool wantPhasors = false);

    // Two-tone intermodulation (csim_imd_batch, include/csim.h): DC operating point, then six factorisations per point;
    // the first tone runs over freqs, the second stays at f2 (Hz).  Output V(outP) - V(outM) (equations; outM = -1: ground).
    BatchImdResult imd(const std::vector<double>& params, int B, const std::vector<double>& freqs, double f2, int outP,
                       int outM = -1, bool wantPhasors = false);

    // Loop gain at a V source in series in the loop (csim_stb_batch, include/csim.h): DC operating point, then one
    // factorisation with two right-hand sides per frequency.  probeElem -1: the .STB card's probe; margins need
    // strictly increasing positive frequencies.
    BatchStbResult stb(const std::vector<double>& params, int B, const std::vector<double>& freqs, int probeElem = -1,
                       bool wantMargins = true);

    // Poles of every instance's linearisation at its operating point (csim_pz_batch, include/csim.h "Pole analysis"):
    // eigenvalues slower than 1 / (2 pi fmax) are poles at infinity; sigma0 shifts G + sigma0 C.  fmax must be positive
    // (std::invalid_argument otherwise): a BatchEngine has no cards, pass the .PZ card's numbers from SimulationConfig.
    BatchPzResult pz(const std::vector<double>& params, int B, double fmax, double sigma0 = 0.0);

    // Periodic steady state of the backward-Euler transient by shooting Newton (csim_pss_batch, include/csim.h): DC
    // operating point, then rounds of one period each; harmonics 0 .. nHarm of probeEq (empty = every unknown).
    // tol, maxRounds <= 0: the engine's pss_tol, pss_max_rounds.  tstep and f0 must be positive (std::invalid_argument
    // otherwise): this engine is built from a Circuit and has no cards to fall back on -- pass sim.tran.tstep,
    // sim.hb.f0 and sim.hb.nHarm of the parsed SimulationConfig.
    BatchPssResult pss(const std::vector<double>& params, int B, double tstep, double f0, int nHarm,
                       const std::vector<int32_t>& probeEq = {}, double tol = 0.0, int maxRounds = 0);

    // Periodic AC analysis (csim_pac_batch, include/csim.h): DC operating point, periodic steady state, then the
    // transfer from the `AC mag [phase]` sources to probeEq (empty = every unknown) at the sidebands f + m f0,
    // m = -nSide .. nSide, of every input frequency of freqs (Hz).  tstep and f0 must be positive and freqs not empty
    // (std::invalid_argument otherwise), for the reason given at pss(): pass the cards' numbers from SimulationConfig.
    BatchPacResult pac(const std::vector<double>& params, int B, double tstep, double f0, const std::vector<double>& freqs,
                       int nSide = 1, const std::vector<int32_t>& probeEq = {});

    // Periodic noise analysis (csim_pnoise_batch, include/csim.h): DC operating point, periodic steady state, then the
    // output noise at outP - outM (equations, -1 = ground) at every output frequency of freqs (Hz), folded down from the
    // sidebands f + m f0, m = -nSide .. nSide, with the contribution of every generator and of every sideband, and the
    // conversion gains from the V or I source srcElem (-1: none, gain stays zero).  tstep and f0 must be positive and
    // freqs not empty (std::invalid_argument otherwise), for the reason given at pss().
    BatchPnoiseResult pnoise(const std::vector<double>& params, int B, double tstep, double f0, const std::vector<double>& freqs,
                             int outP, int outM = -1, int srcElem = -1, int nSide = 1, double tempK = 300.15);

    // the transient of instance `instance` of params ([B][P], empty = nominal) as the reference's CSV
    // (src/tanalisis.cpp:189-231); probeEq empty: the netlist's .PLOTNV/.PRINT probes when `sim` names any, else
    // every unknown.  Throws std::runtime_error on failure.
    void writeCsv(const std::vector<double>& params, int B, int instance, const SimulationConfig& sim,
                  const std::string& path, const std::vector<int32_t>& probeEq = {});

private:
    CircuitIR ir_;
    csim_netlist* nl_ = nullptr;      // netlist handle wrapping ir_ for the C-ABI
    csim_engine* eng_ = nullptr;
};

} // namespace csim
