// csim_pz_demo -- the pole analysis through the C++ batch API (api/analysis.hpp):
// parse -> index -> BatchEngine -> Monte-Carlo table -> BatchEngine::pz with the numbers of the netlist's .PZ card, which
// the caller hands over (a BatchEngine is built from a Circuit and has no cards of its own).
// Prints one JSON line per instance, then one line that says whether fmax = 0 was refused
// (used by tests/test_pz_gpu.py::test_cpp_batch_api_pz).
//
//   csim_pz_demo <netlist.sp> <B>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "../api/analysis.hpp"
#include "../api/parser.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) { std::cerr << "usage: csim_pz_demo <netlist.sp> <B>\n"; return 1; }
    const int B = std::atoi(argv[2]);
    Circuit ckt;
    SimulationConfig sim;
    if (!parseNetlist(argv[1], ckt, sim)) return 1;
    if (!sim.pz.enabled) { std::cerr << "csim_pz_demo: the netlist needs a .PZ card\n"; return 1; }
    ckt.assignEquationIndices();
    try {
        csim::BatchEngine eng(ckt, 0);
        const std::vector<double> params = eng.monteCarloParams(12345, 0.03, 0, B);
        const int N = eng.numUnknowns();
        const csim::BatchPzResult r = eng.pz(params, B, sim.pz.fmax, sim.pz.sigma0);
        if (r.poles.size() != (size_t)B * N || r.nPoles.size() != (size_t)B) { std::cerr << "csim_pz_demo: bad result sizes\n"; return 3; }
        for (int b = 0; b < B; ++b) {
            std::printf("{\"b\": %d, \"status\": %u, \"n_poles\": %d, \"n_rhp\": %d, \"max_re\": %.17g, \"poles\": [", b, r.status[b],
                        r.nPoles[b], r.nRhp[b], r.maxRe[b]);
            for (int k = 0; k < r.nPoles[b]; ++k)
                std::printf("%s[%.17g, %.17g]", k ? ", " : "", r.poles[(size_t)b * N + k].real(), r.poles[(size_t)b * N + k].imag());
            std::printf("]}\n");
        }
        bool refused = false;
        try {
            (void)eng.pz(params, B, 0.0);                           // no card to take fmax from
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        std::printf("{\"fmax_zero_refused\": %s}\n", refused ? "true" : "false");
    } catch (const std::exception& e) {
        std::cerr << "csim_pz_demo: " << e.what() << "\n";
        return 2;
    }
    return 0;
}
