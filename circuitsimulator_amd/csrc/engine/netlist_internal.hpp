// netlist_internal.hpp -- what a csim_netlist handle holds (library-private).
#pragma once

#include <string>
#include <vector>

#include "csim.h"
#include "../api/circuit.hpp"
#include "../api/parser.hpp"
#include "../api/sim.hpp"

namespace csim {
struct Port { int32_t elem, branchEq; double z0; };     // a V source with PORTNUM k, its branch equation and Z0

// The analysis cards as the engine needs them: names resolved to indices, sweep words to the numbers of csim_ac_freqs.
// finishNetlist (netlist_capi.cpp) fills one per netlist, the csim_netlist_* getters report it, an engine keeps a copy
// and takes a call's defaults from it.  Without a card every field keeps its default.
struct SweepGrid {                                      // {DEC|OCT|LIN} n fstart fstop
    int enabled = 0, sweep = 0, points = 0;             // sweep: 0 DEC, 1 OCT, 2 LIN
    double fstart = 0.0, fstop = 0.0;
};
struct SidebandGrid : SweepGrid { int nSide = 1; };     // ... [nside]: sidebands -nSide .. nSide
struct OutputEqs {                                      // V(out[,ref]) [src]
    int outP = -2, outM = -1;                           // equations: -1 ground, -2 a node the netlist does not have
    int srcElem = -1;                                   // input source element, -1 none
};
struct Cards {
    SweepGrid ac, noise, sp, disto, imd, stb;
    SidebandGrid pac, pnoise;
    OutputEqs noiseOut, distoOut, imdOut, pnoiseOut;
    double imdF2overF1 = 0.0;                           // .IMD: the second tone stays at imdF2overF1 * fstart
    int stbElem = -2;                                   // the .STB probe's element, -2: a name the netlist does not have
    struct { int enabled = 0; double fmax = 0.0, sigma0 = 0.0; } pz;   // .PZ POL fmax [sigma0]
    bool spNoise = false;                               // .SP ... 1
    struct { int enabled = 0; double f0 = 0.0; int nHarm = 0; } hb;
    struct { int enabled = 0; double tstep = 0.0; } tran;
};
}

struct csim_netlist {
    Circuit ckt;
    SimulationConfig sim;
    csim::CircuitIR cir;
    std::vector<int> probeEq;      // .PLOTNV / .PRINT node-voltage probes
    std::string csvHeader;
    csim::Cards cards;             // the analysis cards, resolved
    // the ports (PORTNUM) in port order, or what is wrong with their numbering
    std::vector<csim::Port> ports;
    std::string portError;
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

// Non-linear devices of a circuit, in element order (include/csim.h "Distortion analysis"): every MOSFET with its
// drain, gate and source equations, -1 for ground.
struct DistoDevice { int32_t elem, d, g, s; };
inline std::vector<DistoDevice> distoDevices(const CircuitIR& c)
{
    std::vector<DistoDevice> out;
    for (std::size_t e = 0; e < c.kind.size(); ++e) {
        const int32_t* q = c.eq.data() + 4 * e;
        if (c.kind[e] == CSIM_NMOS || c.kind[e] == CSIM_PMOS) out.push_back({static_cast<int32_t>(e), q[0], q[1], q[2]});
    }
    return out;
}

// Ports of a circuit in port order (include/csim.h "S-parameter analysis"): V sources with PORTNUM 1 .. P.  Returns an
// empty string, or what is wrong with the numbering (then `out` is empty).
inline std::string portList(const CircuitIR& c, std::vector<Port>& out)
{
    out.clear();
    std::vector<Port> found;
    std::vector<int> num;
    for (std::size_t e = 0; e < c.portNum.size(); ++e)
        if (c.portNum[e] > 0) {
            found.push_back({static_cast<int32_t>(e), c.branchEq[e], c.portZ0[e]});
            num.push_back(c.portNum[e]);
        }
    const int P = static_cast<int>(found.size());
    if (P > 4) return "ports: at most 4 ports (PORTNUM 1 .. 4)";
    std::vector<Port> ordered(static_cast<std::size_t>(P));
    std::vector<bool> seen(static_cast<std::size_t>(P), false);
    for (int i = 0; i < P; ++i) {
        const int k = num[static_cast<std::size_t>(i)];
        if (k > P) return "ports: PORTNUM must run from 1 to the number of ports without a gap";
        if (seen[static_cast<std::size_t>(k - 1)]) return "ports: PORTNUM " + std::to_string(k) + " is given twice";
        seen[static_cast<std::size_t>(k - 1)] = true;
        ordered[static_cast<std::size_t>(k - 1)] = found[static_cast<std::size_t>(i)];
    }
    out = ordered;
    return std::string();
}
}
