// analysis.cpp -- C++ shims over the C-ABI: the reference's scalar entry points
// are the batch-of-one case of the GPU engine.
#include "analysis.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "dcanalysis.hpp"
#include "solver.hpp"
#include "tanalisis.hpp"
#include "../engine/netlist_internal.hpp"

namespace csim {

namespace {
[[noreturn]] void fail(const char* what)
{
    throw std::runtime_error(std::string(what) + ": " + csim_last_error());
}
} // namespace

BatchEngine::BatchEngine(const Circuit& ckt, int device)
{
    ir_ = flatten(ckt);
    ir_.view();
    // wrap the already-built circuit in a netlist handle for the C-ABI
    nl_ = new csim_netlist();
    nl_->ckt = ckt;
    nl_->cir = ir_;
    nl_->cir.view();
    if (csim_engine_create(nl_, device, &eng_) != CSIM_OK) {
        delete nl_;
        nl_ = nullptr;
        fail("csim_engine_create");
    }
}

BatchEngine::~BatchEngine()
{
    if (eng_) csim_engine_destroy(eng_);
    delete nl_;
}

std::vector<double> BatchEngine::monteCarloParams(uint64_t seed, double sigma, int64_t bFirst, int B) const
{
    const int P = numParams();
    std::vector<double> slotMajor(static_cast<std::size_t>(P) * static_cast<std::size_t>(B));
    if (csim_mc_params_host(nl_, seed, sigma, bFirst, B, slotMajor.data()) != CSIM_OK) fail("csim_mc_params_host");
    std::vector<double> out(slotMajor.size());
    for (int p = 0; p < P; ++p)
        for (int b = 0; b < B; ++b)
            out[static_cast<std::size_t>(b) * P + p] = slotMajor[static_cast<std::size_t>(p) * B + b];
    return out;
}

BatchDcResult BatchEngine::dc(const std::vector<double>& params, int B)
{
    BatchDcResult r;
    const int N = numUnknowns();
    r.x.assign(static_cast<std::size_t>(B) * N, 0.0);
    r.iters.assign(static_cast<std::size_t>(B), 0);
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_dc_batch(eng_, params.empty() ? nullptr : params.data(), B, r.x.data(), r.iters.data(),
                      r.status.data()) != CSIM_OK)
        fail("csim_dc_batch");
    return r;
}

BatchAcResult BatchEngine::ac(const std::vector<double>& params, int B, const std::vector<double>& freqs,
                              const std::vector<int32_t>& probeEq)
{
    BatchAcResult r;
    r.freqs = freqs;
    r.nProbe = probeEq.empty() ? numUnknowns() : static_cast<int>(probeEq.size());
    const int F = static_cast<int>(freqs.size());
    r.v.assign(static_cast<std::size_t>(B) * F * r.nProbe, std::complex<double>());
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_ac_batch(eng_, params.empty() ? nullptr : params.data(), B, freqs.data(), F,
                      probeEq.empty() ? nullptr : probeEq.data(), r.nProbe, reinterpret_cast<double*>(r.v.data()),
                      r.status.data()) != CSIM_OK)
        fail("csim_ac_batch");
    return r;
}

BatchNoiseResult BatchEngine::noise(const std::vector<double>& params, int B, const std::vector<double>& freqs, int outP,
                                    int outM, int srcElem, double tempK, bool wantContrib)
{
    BatchNoiseResult r;
    r.freqs = freqs;
    r.nSources = csim_netlist_num_noise_sources(nl_);
    const std::size_t FB = static_cast<std::size_t>(B) * freqs.size();
    r.onoise.assign(FB, 0.0);
    if (srcElem >= 0) r.gain.assign(FB, std::complex<double>());
    if (wantContrib) r.contrib.assign(FB * static_cast<std::size_t>(r.nSources), 0.0);
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_noise_batch(eng_, params.empty() ? nullptr : params.data(), B, freqs.data(), static_cast<int>(freqs.size()),
                         outP, outM, srcElem, tempK, r.onoise.data(),
                         srcElem >= 0 ? reinterpret_cast<double*>(r.gain.data()) : nullptr,
                         wantContrib ? r.contrib.data() : nullptr, nullptr, r.status.data()) != CSIM_OK)
        fail("csim_noise_batch");
    return r;
}

BatchDistoResult BatchEngine::disto(const std::vector<double>& params, int B, const std::vector<double>& freqs, int outP,
                                    int outM, bool wantPhasors)
{
    BatchDistoResult r;
    r.freqs = freqs;
    r.nDevices = csim_netlist_num_disto_devices(nl_);
    const std::size_t FB = static_cast<std::size_t>(B) * freqs.size();
    if (wantPhasors) r.h.assign(FB * 3 * static_cast<std::size_t>(numUnknowns()), std::complex<double>());
    r.hd.assign(FB * 2, 0.0);
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_disto_batch(eng_, params.empty() ? nullptr : params.data(), B, freqs.data(), static_cast<int>(freqs.size()),
                         outP, outM, wantPhasors ? reinterpret_cast<double*>(r.h.data()) : nullptr, r.hd.data(), nullptr,
                         r.status.data()) != CSIM_OK)
        fail("csim_disto_batch");
    return r;
}

BatchImdResult BatchEngine::imd(const std::vector<double>& params, int B, const std::vector<double>& freqs, double f2, int outP,
                                int outM, bool wantPhasors)
{
    BatchImdResult r;
    r.freqs = freqs;
    r.f2 = f2;
    r.nDevices = csim_netlist_num_disto_devices(nl_);
    const std::size_t FB = static_cast<std::size_t>(B) * freqs.size();
    if (wantPhasors) r.h.assign(FB * 6 * static_cast<std::size_t>(numUnknowns()), std::complex<double>());
    r.im.assign(FB * 3, 0.0);
    r.status.assign(static_cast<std::size_t>(B), 0);
    // an empty list is no sweep, not the card's (a null pointer would ask for the card)
    static const double none = 0.0;
    if (csim_imd_batch(eng_, params.empty() ? nullptr : params.data(), B, freqs.empty() ? &none : freqs.data(),
                       static_cast<int>(freqs.size()), f2, outP, outM, wantPhasors ? reinterpret_cast<double*>(r.h.data()) : nullptr,
                       r.im.data(), nullptr, r.status.data()) != CSIM_OK)
        fail("csim_imd_batch");
    return r;
}

BatchStbResult BatchEngine::stb(const std::vector<double>& params, int B, const std::vector<double>& freqs, int probeElem,
                                bool wantMargins)
{
    BatchStbResult r;
    r.freqs = freqs;
    r.t.assign(static_cast<std::size_t>(B) * freqs.size(), std::complex<double>());
    if (wantMargins) {
        r.margins.assign(static_cast<std::size_t>(B) * 4, 0.0);
        r.found.assign(static_cast<std::size_t>(B), 0);
    }
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_stb_batch(eng_, params.empty() ? nullptr : params.data(), B, freqs.data(), static_cast<int>(freqs.size()),
                       probeElem, reinterpret_cast<double*>(r.t.data()), nullptr, wantMargins ? r.margins.data() : nullptr,
                       wantMargins ? r.found.data() : nullptr, r.status.data()) != CSIM_OK)
        fail("csim_stb_batch");
    return r;
}

BatchPzResult BatchEngine::pz(const std::vector<double>& params, int B, double fmax, double sigma0)
{
    // a BatchEngine has no cards: fmax NaN would ask csim_pz_batch for one
    if (!(fmax > 0.0) || B < 1)
        throw std::invalid_argument("BatchEngine::pz: fmax must be positive, B >= 1 (pass the .PZ card's numbers from "
                                    "SimulationConfig)");
    BatchPzResult r;
    const std::size_t n = static_cast<std::size_t>(numUnknowns());
    r.poles.assign(static_cast<std::size_t>(B) * n, std::complex<double>());
    r.nPoles.assign(static_cast<std::size_t>(B), 0);
    r.nRhp.assign(static_cast<std::size_t>(B), 0);
    r.maxRe.assign(static_cast<std::size_t>(B), 0.0);
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_pz_batch(eng_, params.empty() ? nullptr : params.data(), B, fmax, sigma0, reinterpret_cast<double*>(r.poles.data()),
                      r.nPoles.data(), r.nRhp.data(), r.maxRe.data(), r.status.data()) != CSIM_OK)
        fail("csim_pz_batch");
    return r;
}

BatchPssResult BatchEngine::pss(const std::vector<double>& params, int B, double tstep, double f0, int nHarm,
                                const std::vector<int32_t>& probeEq, double tol, int maxRounds)
{
    // The engine is built from a Circuit and carries no cards, so nothing here may be left to them: the result is
    // sized from nHarm before the call, and csim_pss_batch would take another count from a card when f0 <= 0.
    if (!(tstep > 0.0) || !(f0 > 0.0) || nHarm < 0 || B <= 0)
        throw std::invalid_argument("BatchEngine::pss: tstep and f0 must be positive, nHarm >= 0, B >= 1 (pass the .TRAN "
                                    "card's step and the .HB card's numbers from SimulationConfig)");
    BatchPssResult r;
    r.nHarm = nHarm;
    r.nProbe = probeEq.empty() ? numUnknowns() : static_cast<int>(probeEq.size());
    const std::size_t nB = static_cast<std::size_t>(B > 0 ? B : 0), nH = static_cast<std::size_t>(nHarm >= 0 ? nHarm + 1 : 0);
    r.x0.assign(nB * static_cast<std::size_t>(numUnknowns()), 0.0);
    r.harm.assign(nB * nH * static_cast<std::size_t>(r.nProbe), std::complex<double>());
    r.rounds.assign(nB, 0);
    r.status.assign(nB, 0);
    if (csim_pss_batch(eng_, params.empty() ? nullptr : params.data(), B, tstep, f0, nHarm,
                       probeEq.empty() ? nullptr : probeEq.data(), static_cast<int>(probeEq.size()), tol, maxRounds,
                       r.x0.data(), reinterpret_cast<double*>(r.harm.data()), r.rounds.data(), r.status.data()) != CSIM_OK)
        fail("csim_pss_batch");
    return r;
}

BatchPacResult BatchEngine::pac(const std::vector<double>& params, int B, double tstep, double f0,
                                const std::vector<double>& freqs, int nSide, const std::vector<int32_t>& probeEq)
{
    if (!(tstep > 0.0) || !(f0 > 0.0) || freqs.empty() || nSide < 0 || B <= 0)
        throw std::invalid_argument("BatchEngine::pac: tstep and f0 must be positive, freqs not empty, nSide >= 0, B >= 1 "
                                    "(pass the .TRAN, .HB and .PAC cards' numbers from SimulationConfig)");
    BatchPacResult r;
    r.nSide = nSide;
    r.nProbe = probeEq.empty() ? numUnknowns() : static_cast<int>(probeEq.size());
    r.freqs = freqs;
    const std::size_t nB = static_cast<std::size_t>(B);
    r.p.assign(nB * freqs.size() * static_cast<std::size_t>(2 * nSide + 1) * static_cast<std::size_t>(r.nProbe), std::complex<double>());
    r.x0.assign(nB * static_cast<std::size_t>(numUnknowns()), 0.0);
    r.rounds.assign(nB, 0);
    r.status.assign(nB, 0);
    if (csim_pac_batch(eng_, params.empty() ? nullptr : params.data(), B, tstep, f0, freqs.data(), static_cast<int>(freqs.size()),
                       nSide, probeEq.empty() ? nullptr : probeEq.data(), static_cast<int>(probeEq.size()),
                       reinterpret_cast<double*>(r.p.data()), r.x0.data(), r.rounds.data(), r.status.data()) != CSIM_OK)
        fail("csim_pac_batch");
    return r;
}

BatchPnoiseResult BatchEngine::pnoise(const std::vector<double>& params, int B, double tstep, double f0,
                                      const std::vector<double>& freqs, int outP, int outM, int srcElem, int nSide, double tempK)
{
    if (!(tstep > 0.0) || !(f0 > 0.0) || freqs.empty() || nSide < 0 || B <= 0)
        throw std::invalid_argument("BatchEngine::pnoise: tstep and f0 must be positive, freqs not empty, nSide >= 0, B >= 1 "
                                    "(pass the .TRAN, .HB and .PNOISE cards' numbers from SimulationConfig)");
    BatchPnoiseResult r;
    r.nSide = nSide;
    r.nSrc = csim_netlist_num_noise_sources(nl_);
    r.freqs = freqs;
    const std::size_t nB = static_cast<std::size_t>(B), nF = freqs.size(), nSb = static_cast<std::size_t>(2 * nSide + 1);
    r.onoise.assign(nB * nF, 0.0);
    r.gain.assign(nB * nF * nSb, std::complex<double>());
    r.contrib.assign(nB * nF * static_cast<std::size_t>(r.nSrc), 0.0);
    r.side.assign(nB * nF * nSb, 0.0);
    r.x0.assign(nB * static_cast<std::size_t>(numUnknowns()), 0.0);
    r.rounds.assign(nB, 0);
    r.status.assign(nB, 0);
    if (csim_pnoise_batch(eng_, params.empty() ? nullptr : params.data(), B, tstep, f0, freqs.data(), static_cast<int>(nF), nSide,
                          outP, outM, srcElem, tempK, r.onoise.data(), srcElem >= 0 ? reinterpret_cast<double*>(r.gain.data()) : nullptr,
                          r.contrib.data(), r.side.data(), r.x0.data(), r.rounds.data(), r.status.data()) != CSIM_OK)
        fail("csim_pnoise_batch");
    return r;
}

BatchSpResult BatchEngine::sp(const std::vector<double>& params, int B, const std::vector<double>& freqs, bool wantS)
{
    BatchSpResult r;
    r.freqs = freqs;
    if (r.freqs.empty()) {                                  // the .SP card
        int32_t enabled = 0, sweep = 0, nPoints = 0;
        double fstart = 0.0, fstop = 0.0;
        if (csim_netlist_sp(nl_, &enabled, &sweep, &nPoints, &fstart, &fstop) != CSIM_OK) fail("csim_netlist_sp");
        const int64_t n = enabled ? csim_ac_num_freqs(sweep, nPoints, fstart, fstop) : 0;
        if (n <= 0) { csim::setError("BatchEngine::sp: no frequencies given and the netlist has no .SP card"); fail("BatchEngine::sp"); }
        r.freqs.resize(static_cast<std::size_t>(n));
        if (csim_ac_freqs(sweep, nPoints, fstart, fstop, r.freqs.data()) != CSIM_OK) fail("csim_ac_freqs");
    }
    r.nPorts = std::max(0, csim_netlist_num_ports(nl_));
    const std::size_t n = static_cast<std::size_t>(B) * r.freqs.size() * static_cast<std::size_t>(r.nPorts * r.nPorts);
    r.y.assign(n, std::complex<double>());
    if (wantS) r.s.assign(n, std::complex<double>());
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_sp_batch(eng_, params.empty() ? nullptr : params.data(), B, r.freqs.data(), static_cast<int>(r.freqs.size()),
                      reinterpret_cast<double*>(r.y.data()), wantS ? reinterpret_cast<double*>(r.s.data()) : nullptr,
                      r.status.data()) != CSIM_OK)
        fail("csim_sp_batch");
    return r;
}

BatchSpNoiseResult BatchEngine::spNoise(const std::vector<double>& params, int B, const std::vector<double>& freqs, double tempK)
{
    BatchSpNoiseResult r;
    r.freqs = freqs;
    if (r.freqs.empty()) {                                  // the .SP card
        int32_t enabled = 0, sweep = 0, nPoints = 0;
        double fstart = 0.0, fstop = 0.0;
        if (csim_netlist_sp(nl_, &enabled, &sweep, &nPoints, &fstart, &fstop) != CSIM_OK) fail("csim_netlist_sp");
        const int64_t n = enabled ? csim_ac_num_freqs(sweep, nPoints, fstart, fstop) : 0;
        if (n <= 0) { csim::setError("BatchEngine::spNoise: no frequencies given and the netlist has no .SP card"); fail("BatchEngine::spNoise"); }
        r.freqs.resize(static_cast<std::size_t>(n));
        if (csim_ac_freqs(sweep, nPoints, fstart, fstop, r.freqs.data()) != CSIM_OK) fail("csim_ac_freqs");
    }
    r.nPorts = std::max(0, csim_netlist_num_ports(nl_));
    const std::size_t FB = static_cast<std::size_t>(B) * r.freqs.size();
    const std::size_t n = FB * static_cast<std::size_t>(r.nPorts * r.nPorts);
    const bool two = r.nPorts == 2;
    r.y.assign(n, std::complex<double>());
    r.cy.assign(n, std::complex<double>());
    if (two) {
        r.nf.assign(FB, 0.0);
        r.fmin.assign(FB, 0.0);
        r.rn.assign(FB, 0.0);
        r.yopt.assign(FB, std::complex<double>());
    }
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_spnoise_batch(eng_, params.empty() ? nullptr : params.data(), B, r.freqs.data(), static_cast<int>(r.freqs.size()),
                           tempK, reinterpret_cast<double*>(r.y.data()), reinterpret_cast<double*>(r.cy.data()),
                           two ? r.nf.data() : nullptr, two ? r.fmin.data() : nullptr, two ? r.rn.data() : nullptr,
                           two ? reinterpret_cast<double*>(r.yopt.data()) : nullptr, r.status.data()) != CSIM_OK)
        fail("csim_spnoise_batch");
    return r;
}

BatchTranResult BatchEngine::tran(const std::vector<double>& params, int B, double tstep, double tstop,
                                  double tstart, const std::vector<int32_t>& probeEq, int outStride)
{
    BatchTranResult r;
    const int N = numUnknowns();
    const int np = static_cast<int>(probeEq.size());
    r.rows = np ? csim_tran_num_rows(tstep, tstop, tstart, outStride) : 0;
    if (np && r.rows < 0) { csim::setError("invalid .TRAN numbers"); fail("csim_tran_num_rows"); }
    r.wave.assign(static_cast<std::size_t>(B) * static_cast<std::size_t>(r.rows) * np, 0.0);
    r.xFinal.assign(static_cast<std::size_t>(B) * N, 0.0);
    r.iters.assign(static_cast<std::size_t>(B), 0);
    r.status.assign(static_cast<std::size_t>(B), 0);
    if (csim_tran_batch(eng_, params.empty() ? nullptr : params.data(), B, tstep, tstop, tstart,
                        np ? probeEq.data() : nullptr, np, outStride, np ? r.wave.data() : nullptr,
                        r.xFinal.data(), r.iters.data(), r.status.data()) != CSIM_OK)
        fail("csim_tran_batch");
    return r;
}

void BatchEngine::writeCsv(const std::vector<double>& params, int B, int instance, const SimulationConfig& sim,
                           const std::string& path, const std::vector<int32_t>& probeEq)
{
    std::vector<int32_t> cols = probeEq;
    if (cols.empty()) {
        // node-voltage probes of .PLOTNV / .PRINT cards, in card order (src/parser.cpp:630-723)
        for (const PrintCommand& pc : sim.printCommands)
            for (const ProbeSpec& ps : pc.probes) {
                if (ps.kind != ProbeKind::NodeVoltage) continue;
                const int eq = csim_netlist_node_eq(nl_, ps.node1.c_str());
                if (eq >= 0 && std::find(cols.begin(), cols.end(), eq) == cols.end()) cols.push_back(eq);
            }
    }
    if (cols.empty())
        for (int i = 0; i < numUnknowns(); ++i) cols.push_back(i);
    if (csim_tran_write_csv(eng_, params.empty() ? nullptr : params.data(), B, instance, sim.tran.tstep, sim.tran.tstop,
                            sim.tran.tstart, cols.data(), static_cast<int32_t>(cols.size()), path.c_str()) != CSIM_OK)
        fail("csim_tran_write_csv");
}

} // namespace csim

// ------------------------------------------------------------ dcanalysis.hpp

ConvController::ConvController()
    : alphaMin(0.1), alphaMax(0.5), gminHighBase(1e-6), gminLowBase(3.35e-7), gminAbsMax(1e-4),
      fastConvRatio(0.7), slowConvRatio(1.05) {}

double ConvController::baseGmin(double rampScale) const
{
    const double s = rampScale < 0.0 ? 0.0 : (rampScale > 1.0 ? 1.0 : rampScale);
    return gminHighBase * (1.0 - s) + gminLowBase * s;
}

Eigen::VectorXd dcSolveLU(const Circuit& ckt)
{
    const int N = ckt.numUnknowns();
    if (N == 0) {                                           // dcanalysis.cpp:50-53, 99-102
        std::cerr << "DC solve (LU): no unknowns.\n";
        return Eigen::VectorXd::Zero(0);
    }
    csim::BatchEngine eng(ckt, 0);
    const csim::BatchDcResult r = eng.dc({}, 1);
    if (r.status[0] & CSIM_ST_DC_NONCONV)
        std::cerr << "WARNING: Newton (LU) did not converge within the iteration cap at one or more ramp steps\n";
    if (r.status[0] & CSIM_ST_LU_TINY_PIVOT) std::cerr << "LU solve: decomposition failed.\n";
    Eigen::VectorXd x(N);
    for (int i = 0; i < N; ++i) x(i) = r.x[static_cast<std::size_t>(i)];
    return x;
}

Eigen::VectorXd dcSolve(const Circuit& ckt) { return dcSolveLU(ckt); }

Eigen::VectorXd dcSolveGaussSeidel(const Circuit& ckt)
{
    const int N = ckt.numUnknowns();
    if (N == 0) {                                           // dcanalysis.cpp:75-78, 170-173
        std::cerr << "DC solve (GS): no unknowns.\n";
        return Eigen::VectorXd::Zero(0);
    }
    csim::BatchEngine eng(ckt, 0);
    std::vector<double> x(static_cast<std::size_t>(N), 0.0);
    int32_t iters = 0;
    uint32_t status = 0;
    if (csim_dc_gs_batch(eng.handle(), nullptr, 1, x.data(), &iters, &status) != CSIM_OK)
        throw std::runtime_error(std::string("csim_dc_gs_batch: ") + csim_last_error());
    if (status & CSIM_ST_DC_NONFINITE) std::cerr << "WARNING: GS produced non-finite x at one or more Newton passes (gmin was raised)\n";
    if (status & CSIM_ST_DC_NONCONV) std::cerr << "WARNING: Newton (GS) did not converge within the iteration cap at one or more ramp steps\n";
    Eigen::VectorXd out(N);
    for (int i = 0; i < N; ++i) out(i) = x[static_cast<std::size_t>(i)];
    return out;
}

// host arithmetic, for callers of the reference's header only (dcanalysis.hpp): src/dcanalysis.cpp:268-307
ConvStatus ConvController::update(const Eigen::VectorXd& x, const Eigen::VectorXd& xRaw, double prevErr, int iter,
                                  double /*alphaCurrent*/, double gminCurrent, double rampScale, double tol) const
{
    ConvStatus st;
    double alpha = 0.35 < alphaMin ? alphaMin : (0.35 > alphaMax ? alphaMax : 0.35);       // :274
    const long n = x.size();
    Eigen::VectorXd xNew(n);
    double ss = 0.0;
    for (long i = 0; i < n; ++i) xNew(i) = x(i) + alpha * (xRaw(i) - x(i));
    for (long i = 0; i < n; ++i) { const double d = xNew(i) - x(i); ss += d * d; }
    const double err = std::sqrt(ss);
    const double gminBase = baseGmin(rampScale);
    double gminNext = gminBase;
    if (!(iter == 0 || !std::isfinite(prevErr))) {
        if (err > prevErr * slowConvRatio) { alpha = std::fmax(alpha * 0.7, alphaMin); gminNext = std::fmin(gminCurrent * 2.0, gminAbsMax); }
        else if (err < prevErr * fastConvRatio) { alpha = std::fmin(alpha * 1.1, alphaMax); gminNext = 0.5 * gminCurrent + 0.5 * gminBase; }
        else gminNext = 0.7 * gminCurrent + 0.3 * gminBase;
    }
    st.xNext = xNew;
    st.alphaNext = alpha;
    st.gminNext = gminNext;
    st.error = err;
    st.converged = err < tol;
    return st;
}

// ------------------------------------------------------------- tanalisis.hpp

Eigen::VectorXd computeDcOperatingPoint(const Circuit& ckt) { return dcSolve(ckt); }

void runTransientAnalysisBackwardEuler(const Circuit& ckt, const SimulationConfig& sim, const std::string& outFile)
{
    const TranConfig& cfg = sim.tran;
    if (!cfg.enabled) { std::cerr << "Transient analysis is not enabled (.TRAN missing).\n"; return; }
    if (cfg.tstep <= 0.0 || cfg.tstop <= 0.0) { std::cerr << "Invalid .TRAN card: tstep and tstop must be > 0.\n"; return; }
    const int N = ckt.numUnknowns();
    if (N <= 0) { std::cerr << "Transient: circuit has no unknowns.\n"; return; }

    csim::BatchEngine eng(ckt, 0);
    std::ofstream ofs(outFile);
    if (!ofs) { std::cerr << "Cannot open transient output file '" << outFile << "'.\n"; return; }

    std::vector<int32_t> probes(static_cast<std::size_t>(N));
    for (int i = 0; i < N; ++i) probes[static_cast<std::size_t>(i)] = i;
    const int64_t nSteps = csim_tran_num_steps(cfg.tstep, cfg.tstop);
    std::cout << "[TRAN] tstep=" << std::scientific << cfg.tstep << ", tstop=" << cfg.tstop
              << ", tstart=" << cfg.tstart << "\n[TRAN] total steps = " << nSteps << "\n";

    const csim::BatchTranResult r = eng.tran({}, 1, cfg.tstep, cfg.tstop, cfg.tstart, probes, 1);
    if (r.status[0] & CSIM_ST_TRAN_NONFINITE) throw std::runtime_error("Transient: LU produced NaN/Inf.");
    if (r.status[0] & CSIM_ST_TRAN_NONCONV)
        std::cerr << "WARNING: transient Newton did not converge within the iteration cap at one or more steps\n";

    // CSV in the reference's format (tanalisis.cpp:189-231)
    const csim_ir* ir = eng.ir().view();
    ofs << "time";
    for (int eq = 0; eq < N; ++eq)
        ofs << (eq < ir->n_node_eq ? ",V(" : ",I(") << eng.ir().eqNames[static_cast<std::size_t>(eq)] << ")";
    ofs << "\n";
    const int64_t allRows = nSteps + 1;
    const int64_t first = allRows - r.rows;                 // rows with t < tstart were dropped
    char buf[32];
    for (int64_t k = 0; k < r.rows; ++k) {
        const int64_t row = first + k;
        const double t = row == 0 ? 0.0 : static_cast<double>(static_cast<int>(row)) * cfg.tstep;
        std::snprintf(buf, sizeof buf, "%.9e", t);
        ofs << buf;
        for (int i = 0; i < N; ++i) {
            std::snprintf(buf, sizeof buf, "%.9e", r.wave[static_cast<std::size_t>(k) * N + i]);
            ofs << "," << buf;
        }
        ofs << "\n";
    }
    std::cout << "Transient analysis (Backward Euler) finished. Results written to '" << outFile << "'.\n";
}

// ---------------------------------------------------------------- solver.hpp

namespace Solver {

bool luDecompose(const MatrixXd& A, MatrixXd& LU, std::vector<int>& perm)
{
    const int n = static_cast<int>(A.rows());
    if (n == 0) return false;
    if (A.cols() != n) { std::cerr << "LU: matrix is not square.\n"; return false; }
    std::vector<double> a(static_cast<std::size_t>(n) * n), lu(a.size());
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) a[static_cast<std::size_t>(i) * n + j] = A(i, j);
    std::vector<int32_t> p(static_cast<std::size_t>(n));
    uint32_t flags = 0;
    if (csim_lu_decompose_batch(0, n, 1, a.data(), lu.data(), p.data(), &flags) != CSIM_OK)
        throw std::runtime_error(std::string("csim_lu_decompose_batch: ") + csim_last_error());
    if (flags & CSIM_ST_LU_TINY_PIVOT) { std::cerr << "LU: zero (or tiny) pivot.\n"; return false; }
    LU = MatrixXd(n, n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) LU(i, j) = lu[static_cast<std::size_t>(i) * n + j];
    perm.assign(p.begin(), p.end());
    return true;
}

VectorXd solveLinearSystemLU(const MatrixXd& A, const VectorXd& b)
{
    const int n = static_cast<int>(A.rows());
    VectorXd x = VectorXd::Zero(n);
    if (n == 0) return x;
    if (A.cols() != n || b.size() != n) { std::cerr << "LU solve: dimension mismatch.\n"; return x; }
    std::vector<double> a(static_cast<std::size_t>(n) * n), rhs(static_cast<std::size_t>(n)), sol(rhs.size());
    for (int i = 0; i < n; ++i) {
        rhs[static_cast<std::size_t>(i)] = b(i);
        for (int j = 0; j < n; ++j) a[static_cast<std::size_t>(i) * n + j] = A(i, j);
    }
    uint32_t flags = 0;
    if (csim_lu_solve_batch(0, n, 1, a.data(), rhs.data(), sol.data(), &flags) != CSIM_OK)
        throw std::runtime_error(std::string("csim_lu_solve_batch: ") + csim_last_error());
    if (flags & CSIM_ST_LU_TINY_PIVOT) std::cerr << "LU solve: decomposition failed.\n";
    for (int i = 0; i < n; ++i) x(i) = sol[static_cast<std::size_t>(i)];
    return x;
}

VectorXd solveLinearSystemGaussSeidel(const MatrixXd& A, const VectorXd& b, const VectorXd& x0, int maxIters, double tol)
{
    const int n = static_cast<int>(A.rows());
    if (n == 0) return x0;                                                   // solver.hpp:146
    if (A.cols() != n || b.size() != n) { std::cerr << "Gauss-Seidel: dimension mismatch.\n"; return VectorXd::Zero(n); }
    std::vector<double> a(static_cast<std::size_t>(n) * n), rhs(static_cast<std::size_t>(n)), start(rhs.size(), 0.0), sol(rhs.size());
    for (int i = 0; i < n; ++i) {
        rhs[static_cast<std::size_t>(i)] = b(i);
        if (x0.size() == n) start[static_cast<std::size_t>(i)] = x0(i);      // a wrong-sized x0 starts from zero (:154-157)
        for (int j = 0; j < n; ++j) a[static_cast<std::size_t>(i) * n + j] = A(i, j);
    }
    if (csim_gs_solve_batch(0, n, 1, a.data(), rhs.data(), start.data(), maxIters, tol, sol.data(), nullptr) != CSIM_OK)
        throw std::runtime_error(std::string("csim_gs_solve_batch: ") + csim_last_error());
    VectorXd x(n);
    for (int i = 0; i < n; ++i) x(i) = sol[static_cast<std::size_t>(i)];
    return x;
}

VectorXd solveLinearSystemGaussSeidel(const MatrixXd& A, const VectorXd& b, int maxIters, double tol)
{
    return solveLinearSystemGaussSeidel(A, b, VectorXd::Zero(b.size()), maxIters, tol);       // solver.hpp:197-204
}

} // namespace Solver
