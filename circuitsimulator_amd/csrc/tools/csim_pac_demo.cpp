// csim_pac_demo -- the periodic AC analysis through the C++ batch API (api/analysis.hpp):
// parse -> index -> BatchEngine -> Monte-Carlo table -> BatchEngine::pac with the numbers of the netlist's .TRAN, .HB and
// .PAC cards, which the caller hands over (a BatchEngine is built from a Circuit and has no cards of its own).
// Prints one JSON line per instance, then one line that says whether an empty frequency list was refused
// (used by tests/test_pac_gpu.py::test_cpp_batch_api_pac).
//
//   csim_pac_demo <netlist.sp> <B>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "../api/analysis.hpp"
#include "../api/parser.hpp"
#include "csim.h"

int main(int argc, char** argv)
{
    if (argc != 3) { std::cerr << "usage: csim_pac_demo <netlist.sp> <B>\n"; return 1; }
    const int B = std::atoi(argv[2]);
    Circuit ckt;
    SimulationConfig sim;
    if (!parseNetlist(argv[1], ckt, sim)) return 1;
    if (!sim.hb.enabled || !sim.tran.enabled || !sim.pac.enabled) {
        std::cerr << "csim_pac_demo: the netlist needs .TRAN, .HB and .PAC cards\n";
        return 1;
    }
    ckt.assignEquationIndices();
    const int sweep = acSweepCode(sim.pac.sweepType);
    const int64_t nF = csim_ac_num_freqs(sweep, sim.pac.nPoints, sim.pac.fstart, sim.pac.fstop);
    if (nF <= 0) { std::cerr << "csim_pac_demo: " << csim_last_error() << "\n"; return 1; }
    std::vector<double> freqs((size_t)nF);
    if (csim_ac_freqs(sweep, sim.pac.nPoints, sim.pac.fstart, sim.pac.fstop, freqs.data()) != CSIM_OK) return 1;
    try {
        csim::BatchEngine eng(ckt, 0);
        const std::vector<double> params = eng.monteCarloParams(12345, 0.05, 0, B);
        const int N = eng.numUnknowns();
        const csim::BatchPacResult r = eng.pac(params, B, sim.tran.tstep, sim.hb.f0, freqs, sim.pac.nSide);
        const size_t per = freqs.size() * (size_t)(2 * r.nSide + 1) * r.nProbe;
        if (r.p.size() != (size_t)B * per || r.x0.size() != (size_t)B * N) { std::cerr << "csim_pac_demo: bad result sizes\n"; return 3; }
        for (int b = 0; b < B; ++b) {
            std::printf("{\"b\": %d, \"rounds\": %d, \"status\": %u, \"n_freq\": %d, \"n_side\": %d, \"n_probe\": %d, \"p\": [", b,
                        r.rounds[b], r.status[b], (int)freqs.size(), r.nSide, r.nProbe);
            for (size_t e = 0; e < per; ++e)
                std::printf("%s[%.17g, %.17g]", e ? ", " : "", r.p[b * per + e].real(), r.p[b * per + e].imag());
            std::printf("]}\n");
        }
        bool refused = false;
        try {
            (void)eng.pac(params, B, sim.tran.tstep, sim.hb.f0, {}, sim.pac.nSide);   // no card to take the grid from
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        std::printf("{\"no_freqs_refused\": %s}\n", refused ? "true" : "false");
    } catch (const std::exception& e) {
        std::cerr << "csim_pac_demo: " << e.what() << "\n";
        return 2;
    }
    return 0;
}
