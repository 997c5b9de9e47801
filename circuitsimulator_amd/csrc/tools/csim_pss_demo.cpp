// csim_pss_demo -- the periodic steady state through the C++ batch API (api/analysis.hpp):
// parse -> index -> BatchEngine -> Monte-Carlo table -> BatchEngine::pss with the numbers of the netlist's .TRAN and .HB
// cards, which the caller hands over (a BatchEngine is built from a Circuit and has no cards of its own).
// Prints one JSON line per instance, then one line that says whether f0 = 0 was refused
// (used by tests/test_pss_gpu.py::test_cpp_batch_api_pss).
//
//   csim_pss_demo <netlist.sp> <B>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "../api/analysis.hpp"
#include "../api/parser.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) { std::cerr << "usage: csim_pss_demo <netlist.sp> <B>\n"; return 1; }
    const int B = std::atoi(argv[2]);
    Circuit ckt;
    SimulationConfig sim;
    if (!parseNetlist(argv[1], ckt, sim)) return 1;
    if (!sim.hb.enabled || !sim.tran.enabled) { std::cerr << "csim_pss_demo: the netlist needs .TRAN and .HB cards\n"; return 1; }
    ckt.assignEquationIndices();
    try {
        csim::BatchEngine eng(ckt, 0);
        const std::vector<double> params = eng.monteCarloParams(12345, 0.05, 0, B);
        const int N = eng.numUnknowns();
        const csim::BatchPssResult r = eng.pss(params, B, sim.tran.tstep, sim.hb.f0, sim.hb.nHarm);
        const size_t per = (size_t)(r.nHarm + 1) * r.nProbe;
        if (r.harm.size() != (size_t)B * per || r.x0.size() != (size_t)B * N) { std::cerr << "csim_pss_demo: bad result sizes\n"; return 3; }
        for (int b = 0; b < B; ++b) {
            std::printf("{\"b\": %d, \"rounds\": %d, \"status\": %u, \"n_harm\": %d, \"n_probe\": %d, \"x0\": [", b, r.rounds[b],
                        r.status[b], r.nHarm, r.nProbe);
            for (int i = 0; i < N; ++i) std::printf("%s%.17g", i ? ", " : "", r.x0[(size_t)b * N + i]);
            std::printf("], \"harm\": [");
            for (size_t e = 0; e < per; ++e)
                std::printf("%s[%.17g, %.17g]", e ? ", " : "", r.harm[b * per + e].real(), r.harm[b * per + e].imag());
            std::printf("]}\n");
        }
        bool refused = false;
        try {
            (void)eng.pss(params, B, sim.tran.tstep, 0.0, 0);       // no card to take f0 from: refused before anything is sized
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        std::printf("{\"f0_zero_refused\": %s}\n", refused ? "true" : "false");
    } catch (const std::exception& e) {
        std::cerr << "csim_pss_demo: " << e.what() << "\n";
        return 2;
    }
    return 0;
}
