// netlist_capi.cpp -- C-ABI over the C++ front-end: parse, index, flatten.
// Host only.  Replaces the parseNetlist() + assignEquationIndices() preamble
// every caller of the reference performs (src/main.cpp:29,34).
#include "netlist_internal.hpp"

#include <cmath>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "mc_draw.h"

namespace csim {

thread_local std::string g_lastError;

void setError(const std::string& msg) { g_lastError = msg; }

} // namespace csim

namespace {

csim::SweepGrid gridOf(const AcConfig& a)
{
    return {a.enabled ? 1 : 0, acSweepCode(a.sweepType), a.nPoints, a.fstart, a.fstop};
}

// V(out[,ref]) [src] of an enabled card; no source is -1
csim::OutputEqs outputOf(const Circuit& ckt, bool enabled, const OutputPair& o)
{
    if (!enabled) return {};
    return {csim::cardNodeEquation(ckt, o.outNode), csim::cardNodeEquation(ckt, o.refNode),
            o.srcName.empty() ? -1 : csim::elementIndex(ckt, o.srcName, -1)};
}

// the cards of the front-end -> what the getters report and an engine keeps
csim::Cards resolveCards(const Circuit& ckt, const SimulationConfig& sim)
{
    csim::Cards c;
    c.ac = gridOf(sim.ac);
    c.noise = gridOf(sim.noise);
    c.sp = gridOf(sim.sp);
    c.disto = gridOf(sim.disto);
    c.imd = gridOf(sim.imd);
    c.stb = gridOf(sim.stb);
    c.pac = {gridOf(sim.pac), sim.pac.nSide};
    c.pnoise = {gridOf(sim.pnoise), sim.pnoise.nSide};
    c.noiseOut = outputOf(ckt, sim.noise.enabled, sim.noise);
    c.distoOut = outputOf(ckt, sim.disto.enabled, sim.disto);
    c.imdOut = outputOf(ckt, sim.imd.enabled, sim.imd);
    c.imdF2overF1 = sim.imd.f2overf1;
    c.pnoiseOut = outputOf(ckt, sim.pnoise.enabled, sim.pnoise);
    if (sim.stb.enabled) c.stbElem = csim::elementIndex(ckt, sim.stb.probeName, -2);
    c.pz.enabled = sim.pz.enabled ? 1 : 0;
    c.pz.fmax = sim.pz.fmax;
    c.pz.sigma0 = sim.pz.sigma0;
    c.spNoise = sim.sp.enabled && sim.sp.doNoise;
    c.hb.enabled = sim.hb.enabled ? 1 : 0;
    c.hb.f0 = sim.hb.f0;
    c.hb.nHarm = sim.hb.nHarm;
    c.tran.enabled = sim.tran.enabled ? 1 : 0;
    c.tran.tstep = sim.tran.tstep;
    return c;
}

// what every card getter reports of a grid
void putGrid(const csim::SweepGrid& g, int32_t* enabled, int32_t* sweep, int32_t* n_points, double* fstart, double* fstop)
{
    if (enabled)  *enabled = g.enabled;
    if (sweep)    *sweep = g.sweep;
    if (n_points) *n_points = g.points;
    if (fstart)   *fstart = g.fstart;
    if (fstop)    *fstop = g.fstop;
}

void putOutput(const csim::OutputEqs& o, int32_t* out_p_eq, int32_t* out_m_eq, int32_t* src_elem)
{
    if (out_p_eq) *out_p_eq = o.outP;
    if (out_m_eq) *out_m_eq = o.outM;
    if (src_elem) *src_elem = o.srcElem;
}

int finishNetlist(csim_netlist* nl)
{
    nl->sim.ensureDefaultOp();
    nl->ckt.assignEquationIndices();
    nl->cir = csim::flatten(nl->ckt);
    nl->cir.view();

    // node-voltage probes named by .PLOTNV / .PRINT (first mention wins)
    for (const PrintCommand& pc : nl->sim.printCommands) {
        for (const ProbeSpec& p : pc.probes) {
            if (p.kind != ProbeKind::NodeVoltage || p.node1.empty()) continue;
            const int eq = csim::nodeEquation(nl->ckt, p.node1);
            if (eq < 0) continue;
            bool seen = false;
            for (int q : nl->probeEq) seen = seen || (q == eq);
            if (!seen) nl->probeEq.push_back(eq);
        }
    }

    nl->cards = resolveCards(nl->ckt, nl->sim);

    // PORTNUM tokens: the ports in port order
    nl->portError = csim::portList(nl->cir, nl->ports);
    if (!nl->portError.empty()) std::cerr << nl->portError << "\n";

    // reference CSV header: time, V(node) in node order, I(elem) for V sources
    // and inductors in element order (src/tanalisis.cpp:191-206) == equation order
    std::ostringstream h;
    h << "time";
    const csim_ir* ir = nl->cir.view();
    for (int eq = 0; eq < ir->n_unknowns; ++eq)
        h << (eq < ir->n_node_eq ? ",V(" : ",I(") << nl->cir.eqNames[static_cast<std::size_t>(eq)] << ")";
    nl->csvHeader = h.str();
    return CSIM_OK;
}

} // namespace

extern "C" {

const char* csim_last_error(void) { return csim::g_lastError.c_str(); }
const char* csim_version(void) { return "circuitsimulator_amd 0.1 (gfx950)"; }

int csim_netlist_parse_file(const char* path, csim_netlist** out)
{
    if (!path || !out) { csim::setError("csim_netlist_parse_file: null argument"); return CSIM_ERR_ARG; }
    *out = nullptr;
    auto* nl = new csim_netlist();
    NetlistParser parser(nl->ckt, nl->sim);
    if (!parser.parseFile(path)) {
        delete nl;
        csim::setError(std::string("cannot open netlist file ") + path);
        return CSIM_ERR_IO;
    }
    finishNetlist(nl);
    *out = nl;
    return CSIM_OK;
}

int csim_netlist_parse_text(const char* text, int64_t len, csim_netlist** out)
{
    if (!text || len < 0 || !out) { csim::setError("csim_netlist_parse_text: bad argument"); return CSIM_ERR_ARG; }
    *out = nullptr;
    auto* nl = new csim_netlist();
    std::istringstream in(std::string(text, static_cast<std::size_t>(len)));
    NetlistParser parser(nl->ckt, nl->sim);
    parser.parseStream(in, "<memory>");
    finishNetlist(nl);
    *out = nl;
    return CSIM_OK;
}

void csim_netlist_free(csim_netlist* nl) { delete nl; }

const csim_ir* csim_netlist_ir(const csim_netlist* nl) { return nl ? nl->cir.view() : nullptr; }

int csim_netlist_counts(const csim_netlist* nl, int32_t* n_nodes, int32_t* n_elems,
                        int32_t* n_unknowns, int32_t* n_node_eq, int32_t* n_branch_eq)
{
    if (!nl) return CSIM_ERR_ARG;
    if (n_nodes)     *n_nodes = static_cast<int32_t>(nl->ckt.nodes.size());
    if (n_elems)     *n_elems = static_cast<int32_t>(nl->ckt.elements.size());
    if (n_unknowns)  *n_unknowns = nl->ckt.numUnknowns();
    if (n_node_eq)   *n_node_eq = nl->ckt.numNodeEquations();
    if (n_branch_eq) *n_branch_eq = nl->ckt.numVoltageBranches();
    return CSIM_OK;
}

int csim_netlist_nominal_params(const csim_netlist* nl, double* out)
{
    if (!nl || !out) return CSIM_ERR_ARG;
    std::memcpy(out, nl->cir.nominal.data(), sizeof(double) * nl->cir.nominal.size());
    return CSIM_OK;
}

const char* csim_netlist_eq_name(const csim_netlist* nl, int32_t eq)
{
    if (!nl || eq < 0 || eq >= static_cast<int32_t>(nl->cir.eqNames.size())) return nullptr;
    return nl->cir.eqNames[static_cast<std::size_t>(eq)].c_str();
}

int csim_netlist_node_eq(const csim_netlist* nl, const char* node_name)
{
    return nl && node_name ? csim::nodeEquation(nl->ckt, node_name) : -2;
}

int csim_netlist_tran(const csim_netlist* nl, int32_t* enabled, double* tstep, double* tstop, double* tstart)
{
    if (!nl) return CSIM_ERR_ARG;
    if (enabled) *enabled = nl->sim.tran.enabled ? 1 : 0;
    if (tstep)   *tstep = nl->sim.tran.tstep;
    if (tstop)   *tstop = nl->sim.tran.tstop;
    if (tstart)  *tstart = nl->sim.tran.tstart;
    return CSIM_OK;
}

int csim_netlist_ac(const csim_netlist* nl, int32_t* enabled, int32_t* sweep, int32_t* n_points, double* fstart,
                    double* fstop)
{
    if (!nl) return CSIM_ERR_ARG;
    putGrid(nl->cards.ac, enabled, sweep, n_points, fstart, fstop);
    return CSIM_OK;
}

int csim_netlist_ac_source(const csim_netlist* nl, int32_t elem, double* mag, double* phase_deg)
{
    if (!nl || elem < 0 || elem >= nl->cir.ir.n_elems) { csim::setError("csim_netlist_ac_source: bad element index"); return CSIM_ERR_ARG; }
    if (mag) *mag = nl->cir.acMag[static_cast<std::size_t>(elem)];
    if (phase_deg) *phase_deg = nl->cir.acPhaseDeg[static_cast<std::size_t>(elem)];
    return CSIM_OK;
}

int csim_netlist_noise(const csim_netlist* nl, int32_t* enabled, int32_t* out_p_eq, int32_t* out_m_eq, int32_t* src_elem,
                       int32_t* sweep, int32_t* n_points, double* fstart, double* fstop)
{
    if (!nl) return CSIM_ERR_ARG;
    putGrid(nl->cards.noise, enabled, sweep, n_points, fstart, fstop);
    putOutput(nl->cards.noiseOut, out_p_eq, out_m_eq, src_elem);
    return CSIM_OK;
}

int csim_netlist_num_noise_sources(const csim_netlist* nl) { return nl ? static_cast<int>(csim::noiseSources(nl->cir).size()) : 0; }

int csim_netlist_noise_source(const csim_netlist* nl, int32_t i, int32_t* elem, int32_t* eq_a, int32_t* eq_b)
{
    if (!nl) return CSIM_ERR_ARG;
    const std::vector<csim::NoiseSource> src = csim::noiseSources(nl->cir);
    if (i < 0 || i >= static_cast<int32_t>(src.size())) { csim::setError("csim_netlist_noise_source: bad index"); return CSIM_ERR_ARG; }
    if (elem) *elem = src[static_cast<std::size_t>(i)].elem;
    if (eq_a) *eq_a = src[static_cast<std::size_t>(i)].a;
    if (eq_b) *eq_b = src[static_cast<std::size_t>(i)].b;
    return CSIM_OK;
}

int csim_netlist_disto(const csim_netlist* nl, int32_t* enabled, int32_t* out_p_eq, int32_t* out_m_eq, int32_t* sweep,
                       int32_t* n_points, double* fstart, double* fstop)
{
    if (!nl) return CSIM_ERR_ARG;
    putGrid(nl->cards.disto, enabled, sweep, n_points, fstart, fstop);
    putOutput(nl->cards.distoOut, out_p_eq, out_m_eq, nullptr);
    return CSIM_OK;
}

int csim_netlist_imd(const csim_netlist* nl, int32_t* enabled, int32_t* out_p_eq, int32_t* out_m_eq, int32_t* sweep,
                     int32_t* n_points, double* fstart, double* fstop, double* f2overf1)
{
    if (!nl) return CSIM_ERR_ARG;
    putGrid(nl->cards.imd, enabled, sweep, n_points, fstart, fstop);
    putOutput(nl->cards.imdOut, out_p_eq, out_m_eq, nullptr);
    if (f2overf1) *f2overf1 = nl->cards.imdF2overF1;
    return CSIM_OK;
}

int csim_netlist_num_disto_devices(const csim_netlist* nl) { return nl ? static_cast<int>(csim::distoDevices(nl->cir).size()) : 0; }

int csim_netlist_disto_device(const csim_netlist* nl, int32_t i, int32_t* elem, int32_t* eq_d, int32_t* eq_g, int32_t* eq_s)
{
    if (!nl) return CSIM_ERR_ARG;
    const std::vector<csim::DistoDevice> dev = csim::distoDevices(nl->cir);
    if (i < 0 || i >= static_cast<int32_t>(dev.size())) { csim::setError("csim_netlist_disto_device: bad index"); return CSIM_ERR_ARG; }
    if (elem) *elem = dev[static_cast<std::size_t>(i)].elem;
    if (eq_d) *eq_d = dev[static_cast<std::size_t>(i)].d;
    if (eq_g) *eq_g = dev[static_cast<std::size_t>(i)].g;
    if (eq_s) *eq_s = dev[static_cast<std::size_t>(i)].s;
    return CSIM_OK;
}

int csim_netlist_stb(const csim_netlist* nl, int32_t* enabled, int32_t* elem, int32_t* eq_p, int32_t* eq_m, int32_t* eq_br,
                     int32_t* sweep, int32_t* n_points, double* fstart, double* fstop)
{
    if (!nl) return CSIM_ERR_ARG;
    const int e = nl->cards.stbElem;
    const bool isV = e >= 0 && nl->cir.kind[static_cast<std::size_t>(e)] == CSIM_V;
    putGrid(nl->cards.stb, enabled, sweep, n_points, fstart, fstop);
    if (elem)     *elem = e;
    if (eq_p)     *eq_p = isV ? nl->cir.eq[4 * static_cast<std::size_t>(e) + 0] : -2;
    if (eq_m)     *eq_m = isV ? nl->cir.eq[4 * static_cast<std::size_t>(e) + 1] : -2;
    if (eq_br)    *eq_br = isV ? nl->cir.branchEq[static_cast<std::size_t>(e)] : -2;
    return CSIM_OK;
}

int csim_netlist_pz(const csim_netlist* nl, int32_t* enabled, double* fmax, double* sigma0)
{
    if (!nl) return CSIM_ERR_ARG;
    if (enabled) *enabled = nl->cards.pz.enabled;
    if (fmax)    *fmax = nl->cards.pz.fmax;
    if (sigma0)  *sigma0 = nl->cards.pz.sigma0;
    return CSIM_OK;
}

int csim_netlist_hb(const csim_netlist* nl, int32_t* enabled, double* f0, int32_t* n_harm)
{
    if (!nl) return CSIM_ERR_ARG;
    if (enabled) *enabled = nl->cards.hb.enabled;
    if (f0)      *f0 = nl->cards.hb.f0;
    if (n_harm)  *n_harm = nl->cards.hb.nHarm;
    return CSIM_OK;
}

int csim_netlist_pac(const csim_netlist* nl, int32_t* enabled, int32_t* sweep, int32_t* n_points, double* fstart,
                     double* fstop, int32_t* n_side)
{
    if (!nl) return CSIM_ERR_ARG;
    const csim::SidebandGrid& a = nl->cards.pac;
    putGrid(a, enabled, sweep, n_points, fstart, fstop);
    if (n_side) *n_side = a.enabled ? a.nSide : 0;
    return CSIM_OK;
}

int csim_netlist_pnoise(const csim_netlist* nl, int32_t* enabled, int32_t* out_p_eq, int32_t* out_m_eq, int32_t* src_elem,
                        int32_t* sweep, int32_t* n_points, double* fstart, double* fstop, int32_t* n_side)
{
    if (!nl) return CSIM_ERR_ARG;
    const csim::SidebandGrid& a = nl->cards.pnoise;
    putGrid(a, enabled, sweep, n_points, fstart, fstop);
    putOutput(nl->cards.pnoiseOut, out_p_eq, out_m_eq, src_elem);
    if (n_side) *n_side = a.enabled ? a.nSide : 0;
    return CSIM_OK;
}

int csim_netlist_num_ports(const csim_netlist* nl)
{
    if (!nl) return CSIM_ERR_ARG;
    if (!nl->portError.empty()) { csim::setError(nl->portError); return CSIM_ERR_CONFIG; }
    return static_cast<int>(nl->ports.size());
}

int csim_netlist_port(const csim_netlist* nl, int32_t i, int32_t* elem, int32_t* branch_eq, double* z0)
{
    if (!nl || i < 0 || i >= static_cast<int32_t>(nl->ports.size())) { csim::setError("csim_netlist_port: bad index"); return CSIM_ERR_ARG; }
    const csim::Port& p = nl->ports[static_cast<std::size_t>(i)];
    if (elem) *elem = p.elem;
    if (branch_eq) *branch_eq = p.branchEq;
    if (z0) *z0 = p.z0;
    return CSIM_OK;
}

int csim_netlist_sp(const csim_netlist* nl, int32_t* enabled, int32_t* sweep, int32_t* n_points, double* fstart, double* fstop)
{
    if (!nl) return CSIM_ERR_ARG;
    putGrid(nl->cards.sp, enabled, sweep, n_points, fstart, fstop);
    return CSIM_OK;
}

int csim_netlist_sp_noise(const csim_netlist* nl, int32_t* donoise)
{
    if (!nl) return CSIM_ERR_ARG;
    if (donoise) *donoise = nl->cards.spNoise ? 1 : 0;
    return CSIM_OK;
}

// SPICE frequency grid of an .AC card (DEC / OCT: n points per decade / octave from fstart, up to fstop;
// LIN: n points from fstart to fstop inclusive)
int64_t csim_ac_num_freqs(int32_t sweep, int32_t n_points, double fstart, double fstop)
{
    if (sweep < 0 || sweep > 2) { csim::setError("AC sweep must be 0 (DEC), 1 (OCT) or 2 (LIN)"); return CSIM_ERR_CONFIG; }
    if (n_points <= 0 || !std::isfinite(fstart) || !std::isfinite(fstop) || fstop < fstart || (sweep != 2 && fstart <= 0.0)) {
        csim::setError("invalid .AC numbers (need n > 0, fstop >= fstart, fstart > 0 for DEC/OCT)");
        return CSIM_ERR_CONFIG;
    }
    if (sweep == 2) return n_points;
    const double span = sweep == 0 ? std::log10(fstop / fstart) : std::log2(fstop / fstart);
    const double last = std::floor(static_cast<double>(n_points) * span + 1e-9);
    if (!(last >= 0.0) || last >= 2147483647.0) { csim::setError("invalid .AC numbers: too many points"); return CSIM_ERR_CONFIG; }
    return static_cast<int64_t>(last) + 1;
}

int csim_ac_freqs(int32_t sweep, int32_t n_points, double fstart, double fstop, double* f)
{
    const int64_t n = csim_ac_num_freqs(sweep, n_points, fstart, fstop);
    if (n < 0) return static_cast<int>(n);
    if (!f) { csim::setError("csim_ac_freqs: null output"); return CSIM_ERR_ARG; }
    if (sweep == 2) {
        for (int64_t k = 0; k < n; ++k)
            f[k] = n == 1 ? fstart : fstart + static_cast<double>(k) * (fstop - fstart) / static_cast<double>(n - 1);
    } else {
        const double base = sweep == 0 ? 10.0 : 2.0;
        for (int64_t k = 0; k < n; ++k) f[k] = fstart * std::pow(base, static_cast<double>(k) / n_points);
    }
    return CSIM_OK;
}

int csim_netlist_num_probes(const csim_netlist* nl) { return nl ? static_cast<int>(nl->probeEq.size()) : 0; }

int csim_netlist_probe_eq(const csim_netlist* nl, int32_t i)
{
    if (!nl || i < 0 || i >= static_cast<int32_t>(nl->probeEq.size())) return -2;
    return nl->probeEq[static_cast<std::size_t>(i)];
}

int csim_netlist_num_dc_sweeps(const csim_netlist* nl) { return nl ? static_cast<int>(nl->sim.dcSweeps.size()) : 0; }

int csim_netlist_dc_sweep(const csim_netlist* nl, int32_t i, int32_t* src_elem,
                          double* start, double* stop, double* step)
{
    if (!nl || i < 0 || i >= static_cast<int32_t>(nl->sim.dcSweeps.size())) return CSIM_ERR_ARG;
    const DCSweepConfig& dc = nl->sim.dcSweeps[static_cast<std::size_t>(i)];
    if (src_elem) *src_elem = csim::elementIndex(nl->ckt, dc.sourceName, -1);
    if (start) *start = dc.start;
    if (stop)  *stop = dc.stop;
    if (step)  *step = dc.step;
    return CSIM_OK;
}

static int sweepSource(const csim_netlist* nl, int32_t i, int* elem, double* a, double* b, double* st)
{
    int32_t e = -1;
    if (csim_netlist_dc_sweep(nl, i, &e, a, b, st) != CSIM_OK) return CSIM_ERR_ARG;
    if (e < 0) return CSIM_ERR_ARG;
    const int kind = nl->cir.kind[static_cast<std::size_t>(e)];
    if (kind != CSIM_V && kind != CSIM_I) return CSIM_ERR_ARG;
    *elem = e;
    return CSIM_OK;
}

int64_t csim_netlist_dc_sweep_points(const csim_netlist* nl, int32_t i)
{
    int e = -1;
    double a = 0, b = 0, st = 0;
    if (!nl || sweepSource(nl, i, &e, &a, &b, &st) != CSIM_OK) return 0;
    if (st == 0.0 || (b - a) / st < 0.0) return 0;
    return static_cast<int64_t>(std::floor((b - a) / st + 1e-9)) + 1;
}

int csim_netlist_dc_sweep_params(const csim_netlist* nl, int32_t i, int64_t n_points, double* params, double* values)
{
    int e = -1;
    double a = 0, b = 0, st = 0;
    if (!nl || !params || n_points < 0 || sweepSource(nl, i, &e, &a, &b, &st) != CSIM_OK) {
        csim::setError("csim_netlist_dc_sweep_params: bad sweep");
        return CSIM_ERR_ARG;
    }
    const csim::CircuitIR& c = nl->cir;
    const int P = static_cast<int>(c.nominal.size());
    const int slot = c.paramSlot[static_cast<std::size_t>(e)];      // SourceSpec::dcValue
    for (int p = 0; p < P; ++p)
        for (int64_t j = 0; j < n_points; ++j)
            params[static_cast<int64_t>(p) * n_points + j] = c.nominal[static_cast<std::size_t>(p)];
    for (int64_t j = 0; j < n_points; ++j) {
        const double v = a + static_cast<double>(j) * st;
        params[static_cast<int64_t>(slot) * n_points + j] = v;
        if (values) values[j] = v;
    }
    return CSIM_OK;
}

int csim_netlist_csv_header(const csim_netlist* nl, char* buf, int32_t cap)
{
    if (!nl) return CSIM_ERR_ARG;
    const int need = static_cast<int>(nl->csvHeader.size());
    if (buf && cap > 0) {
        const int n = need < cap - 1 ? need : cap - 1;
        std::memcpy(buf, nl->csvHeader.data(), static_cast<std::size_t>(n));
        buf[n] = '\0';
    }
    return need;
}

int csim_netlist_mc_kinds(const csim_netlist* nl, int32_t* kinds)
{
    if (!nl || !kinds) return CSIM_ERR_ARG;
    std::memcpy(kinds, nl->cir.mcKind.data(), sizeof(int32_t) * nl->cir.mcKind.size());
    return CSIM_OK;
}

int csim_mc_params_host(const csim_netlist* nl, uint64_t seed, double sigma, int64_t b_first,
                        int32_t B, double* params)
{
    if (!nl || !params || B < 0 || b_first < 0) { csim::setError("csim_mc_params_host: bad argument"); return CSIM_ERR_ARG; }
    const csim::CircuitIR& c = nl->cir;
    const int P = static_cast<int>(c.nominal.size());
    for (int p = 0; p < P; ++p) {
        for (int b = 0; b < B; ++b) {
            const uint64_t inst = static_cast<uint64_t>(b_first + b);
            const int kind = c.mcKind[static_cast<std::size_t>(p)];
            const double z = kind ? csim_mc::draw_z(seed, inst, static_cast<uint64_t>(p)) : 0.0;
            params[static_cast<int64_t>(p) * B + b] = csim_mc::perturb(
                kind, c.nominal[static_cast<std::size_t>(p)], c.mcMu[static_cast<std::size_t>(p)],
                c.mcCox[static_cast<std::size_t>(p)], c.mcW[static_cast<std::size_t>(p)],
                c.mcL[static_cast<std::size_t>(p)], sigma, z);
        }
    }
    return CSIM_OK;
}

} // extern "C"
