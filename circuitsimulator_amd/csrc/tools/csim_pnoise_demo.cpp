// csim_pnoise_demo -- the periodic noise analysis through the C++ batch API (api/analysis.hpp):
// parse -> index -> BatchEngine -> Monte-Carlo table -> BatchEngine::pnoise with the numbers of the netlist's .TRAN, .HB and
// .PNOISE cards, which the caller hands over (a BatchEngine is built from a Circuit and has no cards of its own); the
// card's node and source names are resolved here, against the indexed circuit.
// Prints one JSON line per instance, then one line that says whether an empty frequency list was refused
// (used by tests/test_pnoise_gpu.py::test_cpp_batch_api_pnoise).
//
//   csim_pnoise_demo <netlist.sp> <B>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "../api/analysis.hpp"
#include "../api/parser.hpp"
#include "../api/utils.hpp"
#include "csim.h"

int main(int argc, char** argv)
{
    if (argc != 3) { std::cerr << "usage: csim_pnoise_demo <netlist.sp> <B>\n"; return 1; }
    const int B = std::atoi(argv[2]);
    Circuit ckt;
    SimulationConfig sim;
    if (!parseNetlist(argv[1], ckt, sim)) return 1;
    if (!sim.hb.enabled || !sim.tran.enabled || !sim.pnoise.enabled) {
        std::cerr << "csim_pnoise_demo: the netlist needs .TRAN, .HB and .PNOISE cards\n";
        return 1;
    }
    ckt.assignEquationIndices();
    const int outP = csim::cardNodeEquation(ckt, sim.pnoise.outNode), outM = csim::cardNodeEquation(ckt, sim.pnoise.refNode);
    const int src = sim.pnoise.srcName.empty() ? -1 : csim::elementIndex(ckt, sim.pnoise.srcName, -1);
    const int sweep = acSweepCode(sim.pnoise.sweepType);
    const int64_t nF = csim_ac_num_freqs(sweep, sim.pnoise.nPoints, sim.pnoise.fstart, sim.pnoise.fstop);
    if (nF <= 0) { std::cerr << "csim_pnoise_demo: " << csim_last_error() << "\n"; return 1; }
    std::vector<double> freqs((size_t)nF);
    if (csim_ac_freqs(sweep, sim.pnoise.nPoints, sim.pnoise.fstart, sim.pnoise.fstop, freqs.data()) != CSIM_OK) return 1;
    try {
        csim::BatchEngine eng(ckt, 0);
        const std::vector<double> params = eng.monteCarloParams(12345, 0.05, 0, B);
        const int N = eng.numUnknowns();
        const csim::BatchPnoiseResult r = eng.pnoise(params, B, sim.tran.tstep, sim.hb.f0, freqs, outP, outM, src, sim.pnoise.nSide);
        const size_t nSb = (size_t)(2 * r.nSide + 1), F = freqs.size();
        if (r.onoise.size() != (size_t)B * F || r.gain.size() != (size_t)B * F * nSb || r.contrib.size() != (size_t)B * F * r.nSrc ||
            r.side.size() != (size_t)B * F * nSb || r.x0.size() != (size_t)B * N) { std::cerr << "csim_pnoise_demo: bad result sizes\n"; return 3; }
        auto reals = [](const char* key, const double* v, size_t n) {
            std::printf(", \"%s\": [", key);
            for (size_t e = 0; e < n; ++e) std::printf("%s%.17g", e ? ", " : "", v[e]);
            std::printf("]");
        };
        for (int b = 0; b < B; ++b) {
            std::printf("{\"b\": %d, \"rounds\": %d, \"status\": %u, \"n_freq\": %d, \"n_side\": %d, \"n_src\": %d", b, r.rounds[b],
                        r.status[b], (int)F, r.nSide, r.nSrc);
            reals("onoise", r.onoise.data() + b * F, F);
            reals("contrib", r.contrib.data() + b * F * r.nSrc, F * r.nSrc);
            reals("side", r.side.data() + b * F * nSb, F * nSb);
            std::printf(", \"gain\": [");
            for (size_t e = 0; e < F * nSb; ++e)
                std::printf("%s[%.17g, %.17g]", e ? ", " : "", r.gain[b * F * nSb + e].real(), r.gain[b * F * nSb + e].imag());
            std::printf("]}\n");
        }
        bool refused = false;
        try {
            (void)eng.pnoise(params, B, sim.tran.tstep, sim.hb.f0, {}, outP, outM, src, sim.pnoise.nSide);   // no card to take the grid from
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        std::printf("{\"no_freqs_refused\": %s}\n", refused ? "true" : "false");
    } catch (const std::exception& e) {
        std::cerr << "csim_pnoise_demo: " << e.what() << "\n";
        return 2;
    }
    return 0;
}
