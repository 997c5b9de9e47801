// netlist_internal.hpp -- what a csim_netlist handle holds (library-private).
#pragma once

#include <string>
#include <vector>

#include "csim.h"
#include "../api/circuit.hpp"
#include "../api/parser.hpp"
#include "../api/sim.hpp"

struct csim_netlist {
    Circuit ckt;
    SimulationConfig sim;
    csim::CircuitIR cir;
    std::vector<int> probeEq;      // .PLOTNV / .PRINT node-voltage probes
    std::string csvHeader;
    // .NOISE card resolved to indices: output equations (-1 ground, -2 unknown node), input source element (-1 none)
    int noiseOutP = -2, noiseOutM = -1, noiseSrcElem = -1;
};

namespace csim {
void setError(const std::string& msg);

// Noise generators of a circuit, in element order (include/csim.h "Noise analysis"): every resistor between its
// terminals, every MOSFET channel between drain and source.  Equations, -1 for ground.
struct NoiseSource { int32_t elem, a, b; };
inline std::vector<NoiseSource> noiseSources(const CircuitIR& c)
{
    std::vector<NoiseSource> out;
    for (std::size_t e = 0; e < c.kind.size(); ++e) {
        const int32_t* q = c.eq.data() + 4 * e;
        if (c.kind[e] == CSIM_R) out.push_back({static_cast<int32_t>(e), q[0], q[1]});
        else if (c.kind[e] == CSIM_NMOS || c.kind[e] == CSIM_PMOS) out.push_back({static_cast<int32_t>(e), q[0], q[2]});
    }
    return out;
}
}
