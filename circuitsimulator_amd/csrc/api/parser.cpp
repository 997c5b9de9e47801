// parser.cpp -- netlist dialect of the reference (src/parser.cpp), restated:
//   physical lines, trailing CR dropped; '$' starts an inline comment; a line
//   whose first non-blank is '*' or ';' is a comment; a leading '+' continues
//   the previous logical line; tokens split on blanks.
//   Devices by first letter (any case): R C L V I M.   Cards: .MODEL (read in
//   a first pass, so it may follow its users) .TRAN .OP .DC .AC .NOISE .SP .DISTO .IMD .STB .PZ .HB
//   .PAC .PNOISE .PRINT .PLOTNV .PLOTNC; anything else is reported and skipped.
#include "parser.hpp"

#include <algorithm>
#include <cctype>
#include <exception>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>

namespace {

std::string dropInlineComment(const std::string& s)
{
    const std::size_t at = s.find('$');
    return at == std::string::npos ? s : s.substr(0, at);
}

std::string clean(const std::string& s) { return rtrim(ltrim(dropInlineComment(s))); }

char upperHead(const std::string& tok)
{
    return static_cast<char>(std::toupper(static_cast<unsigned char>(tok[0])));
}

// position of the first '(' and of the last ')' in s, -1 when absent
void parenSpan(const std::string& s, int& open, int& close)
{
    open = close = -1;
    for (int i = 0; i < static_cast<int>(s.size()); ++i) {
        if (s[static_cast<std::size_t>(i)] == '(' && open < 0) open = i;
        if (s[static_cast<std::size_t>(i)] == ')') close = i;
    }
}

AnalysisType analysisFromToken(const std::string& tok)
{
    const std::string t = toLower(tok);
    if (t == "op")   return AnalysisType::OP;
    if (t == "dc")   return AnalysisType::DC;
    if (t == "ac")   return AnalysisType::AC;
    if (t == "tran") return AnalysisType::TRAN;
    if (t == "hb")   return AnalysisType::HB;
    return AnalysisType::NONE;
}

} // namespace

NetlistParser::NetlistParser(Circuit& circuit, SimulationConfig& simConfig) : ckt(circuit), sim(simConfig) {}

bool NetlistParser::parseFile(const std::string& filename)
{
    std::ifstream fin(filename);
    if (!fin) {
        std::cerr << "cannot open netlist file " << filename << "\n";
        return false;
    }
    return parseStream(fin, filename);
}

bool NetlistParser::parseStream(std::istream& in, const std::string& originName)
{
    sourceName = originName;
    lex(in);
    parseStatements();
    return true;
}

void NetlistParser::lex(std::istream& in)
{
    stmts.clear();
    std::string pending;       // logical line being assembled
    int pendingLine = 0;

    auto flush = [&]() {
        const std::string text = clean(pending);
        pending.clear();
        if (text.empty()) return;
        Statement st;
        st.lineNo = pendingLine;
        st.raw = text;
        std::istringstream split(text);
        for (std::string tok; split >> tok;) st.tokens.push_back(tok);
        if (!st.tokens.empty()) stmts.push_back(std::move(st));
    };

    std::string line;
    int lineNo = 0;
    while (std::getline(in, line)) {
        ++lineNo;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const std::string s = clean(line);
        if (s.empty()) continue;
        if (s[0] == '*' || s[0] == ';') continue;

        if (s[0] == '+') {
            const std::string rest = ltrim(s.substr(1));
            if (pending.empty()) {          // stray continuation opens a statement
                pendingLine = lineNo;
                pending = rest;
            } else {
                pending += " ";
                pending += rest;
            }
        } else {
            if (!pending.empty()) flush();
            pendingLine = lineNo;
            pending = s;
        }
    }
    if (!pending.empty()) flush();
}

void NetlistParser::parseStatements()
{
    // pass 1: models, so devices may precede their .MODEL card
    for (const Statement& st : stmts)
        if (toLower(st.tokens[0]) == ".model") modelCard(st);

    // pass 2: everything else, in netlist order (this order defines node and
    // element numbering)
    for (const Statement& st : stmts) {
        const std::string& head = st.tokens[0];
        if (head[0] == '.') {
            if (toLower(head) != ".model") dotCard(st);
        } else {
            // a leading title line is not special-cased: like the reference
            // it is handed to the device dispatcher, which reports it
            deviceStatement(st);
        }
    }
    sim.ensureDefaultOp();
}

void NetlistParser::deviceStatement(const Statement& st)
{
    // PORTNUM k [Z0 r] makes a V source a port of the S-parameter analysis; nothing else can be one
    if (upperHead(st.tokens[0]) != 'V')
        for (std::size_t i = 1; i < st.tokens.size(); ++i)
            if (toLower(st.tokens[i]) == "portnum") {
                std::cerr << "Line " << st.lineNo << ": PORTNUM needs a voltage source: " << st.raw << "\n";
                return;
            }
    switch (upperHead(st.tokens[0])) {
        case 'R': case 'C': case 'L': twoTerminal(st, upperHead(st.tokens[0])); break;
        case 'V': voltageSource(st); break;
        case 'I': currentSource(st); break;
        case 'M': mosfet(st); break;
        default:
            std::cerr << "Line " << st.lineNo << ": unsupported element or syntax: " << st.raw << "\n";
    }
}

// Rname n1 n2 value | Cname ... | Lname ...
void NetlistParser::twoTerminal(const Statement& st, char kind)
{
    const auto& t = st.tokens;
    const char* what = kind == 'R' ? "resistor" : (kind == 'C' ? "capacitor" : "inductor");
    if (t.size() < 4) {
        std::cerr << "Line " << st.lineNo << ": invalid " << what << ": " << st.raw << "\n";
        return;
    }
    double value = 0.0;
    try {
        value = parseSpiceNumber(t[3]);
    } catch (const std::exception& e) {
        std::cerr << "Line " << st.lineNo << ": cannot parse " << kind << " value: " << e.what()
                  << " in '" << st.raw << "'\n";
        return;
    }
    if (kind == 'R')      ckt.addResistor(t[0], t[1], t[2], value);
    else if (kind == 'C') ckt.addCapacitor(t[0], t[1], t[2], value);
    else                  ckt.addInductor(t[0], t[1], t[2], value);
}

// PULSE / PWL waveforms.  The reference's netlist dialect has no syntax for them (its parser
// rejects the statement, src/parser.cpp:330-345) although its solver evaluates them
// (include/sim.hpp:80-138) for circuits built through the C++ API.  Accepted here as a superset:
//   PULSE v1 v2 [td [tr [tf [ton [per]]]]]      PWL t0 v0 t1 v1 ...
// with optional SPICE-style parentheses and commas.  Returns true when a waveform keyword was
// consumed (valid or not).
namespace {
bool startsWithKeyword(const std::string& token, const char* kw)
{
    const std::string low = toLower(token);
    const std::string k(kw);
    return low.compare(0, k.size(), k) == 0 && (low.size() == k.size() || low[k.size()] == '(');
}

bool parsePulseOrPwl(const std::vector<std::string>& t, std::size_t next, int lineNo, const std::string& raw,
                     SourceSpec& spec)
{
    if (next >= t.size()) return false;
    const bool pulse = startsWithKeyword(t[next], "pulse");
    const bool pwl = startsWithKeyword(t[next], "pwl");
    if (!pulse && !pwl) return false;

    std::string rest;
    for (std::size_t i = next; i < t.size(); ++i) rest += t[i] + " ";
    rest = rest.substr(pulse ? 5 : 3);
    for (char& c : rest) if (c == '(' || c == ')' || c == ',') c = ' ';
    std::vector<double> vals;
    try {
        std::istringstream is(rest);
        std::string tok;
        while (is >> tok) vals.push_back(parseSpiceNumber(tok));
    } catch (const std::exception& e) {
        std::cerr << "Line " << lineNo << ": cannot parse " << (pulse ? "PULSE" : "PWL") << " parameters: "
                  << e.what() << " in '" << raw << "'\n";
        return true;
    }
    if (pulse) {
        if (vals.size() < 2 || vals.size() > 7) {
            std::cerr << "Line " << lineNo << ": PULSE needs 2 to 7 parameters (v1 v2 td tr tf ton per): " << raw << "\n";
            return true;
        }
        vals.resize(7, 0.0);
        PulseSpec p;
        p.v1 = vals[0]; p.v2 = vals[1]; p.td = vals[2]; p.tr = vals[3]; p.tf = vals[4]; p.ton = vals[5]; p.per = vals[6];
        spec.tran.type = WaveformType::PULSE;
        spec.tran.pulse = p;
    } else {
        if (vals.size() < 2 || vals.size() % 2 != 0) {
            std::cerr << "Line " << lineNo << ": PWL needs (time value) pairs: " << raw << "\n";
            return true;
        }
        PwlSpec w;
        for (std::size_t i = 0; i < vals.size(); i += 2) { w.t.push_back(vals[i]); w.v.push_back(vals[i + 1]); }
        spec.tran.type = WaveformType::PWL;
        spec.tran.pwl = w;
    }
    return true;
}
// `AC mag [phase_deg]`: the small-signal excitation of a source (SourceSpec::acMag / acPhaseDeg,
// include/sim.hpp:146-149, stamped by VoltageSource/CurrentSource::stampAC, src/element.cpp:68-81,125-151).
// The reference's parser has no syntax for it either; accepted as a superset after the DC value or in its
// place, before an optional SIN / PULSE / PWL waveform.  `next` moves past the tokens consumed; false (with a
// message) when the numbers do not parse.
bool isWaveKeyword(const std::string& token)
{
    return toLower(token) == "sin" || toLower(token) == "dc" || startsWithKeyword(token, "pulse") ||
           startsWithKeyword(token, "pwl") || startsWithKeyword(token, "sin");
}

// `PORTNUM k [Z0 r]` (ngspice's spelling) anywhere after the nodes of a V line: taken out of the token list, so the
// DC / AC / waveform tokens parse as they do without it.  False (with a message) when k or r is not acceptable.
bool takePortSpec(std::vector<std::string>& t, int lineNo, const std::string& raw, SourceSpec& spec)
{
    std::size_t at = 3;
    while (at < t.size() && toLower(t[at]) != "portnum") ++at;
    if (at >= t.size()) return true;
    std::size_t end = at + 2;
    bool ok = at + 1 < t.size();
    double k = 0.0, z0 = 50.0;
    try {
        if (ok) k = parseSpiceNumber(t[at + 1]);
        if (ok && end < t.size() && toLower(t[end]) == "z0") {
            ok = end + 1 < t.size();
            if (ok) z0 = parseSpiceNumber(t[end + 1]);
            end += 2;
        }
    } catch (const std::exception&) {
        ok = false;
    }
    ok = ok && k >= 1.0 && k <= 1e6 && k == static_cast<double>(static_cast<int>(k)) && z0 > 0.0 && z0 <= 1.7e308;
    for (std::size_t i = std::min(end, t.size()); ok && i < t.size(); ++i) ok = toLower(t[i]) != "portnum";
    if (!ok) {
        std::cerr << "Line " << lineNo << ": PORTNUM needs a port number >= 1 and, after Z0, a finite resistance > 0: "
                  << raw << "\n";
        return false;
    }
    spec.portNum = static_cast<int>(k);
    spec.portZ0 = z0;
    t.erase(t.begin() + static_cast<std::ptrdiff_t>(at), t.begin() + static_cast<std::ptrdiff_t>(end));
    return true;
}

bool parseAcSpec(const std::vector<std::string>& t, std::size_t& next, int lineNo, const std::string& raw, SourceSpec& spec)
{
    if (next >= t.size() || toLower(t[next]) != "ac") return true;
    if (next + 1 >= t.size()) {
        std::cerr << "Line " << lineNo << ": AC needs a magnitude: " << raw << "\n";
        return false;
    }
    try {
        spec.acMag = parseSpiceNumber(t[next + 1]);
        next += 2;
        if (next < t.size() && !isWaveKeyword(t[next])) {
            spec.acPhaseDeg = parseSpiceNumber(t[next]);
            next += 1;
        }
    } catch (const std::exception& e) {
        std::cerr << "Line " << lineNo << ": cannot parse AC parameters: " << e.what() << " in '" << raw << "'\n";
        return false;
    }
    return true;
}
} // namespace

// Vname np nm <value> [AC mag [phase]] [SIN ...] | Vname np nm DC <value> [AC ...] [SIN ...] |
// Vname np nm [AC mag [phase]] SIN v0 va freq [td [phi]]
// each with `PORTNUM k [Z0 r]` anywhere after the nodes (usually last): port k of the .SP analysis
void NetlistParser::voltageSource(const Statement& st)
{
    std::vector<std::string> t = st.tokens;
    SourceSpec spec;
    if (!takePortSpec(t, st.lineNo, st.raw, spec)) return;
    if (t.size() < 4) {
        std::cerr << "Line " << st.lineNo << ": invalid voltage source: " << st.raw << "\n";
        return;
    }

    std::size_t next = 3;      // token where a waveform keyword may start
    try {
        if (t.size() >= 5 && toLower(t[3]) == "dc") {
            spec.dcValue = parseSpiceNumber(t[4]);
            next = 5;
        } else if (toLower(t[3]) == "ac" || toLower(t[3]) == "sin" || startsWithKeyword(t[3], "pulse") || startsWithKeyword(t[3], "pwl")) {
            spec.dcValue = 0.0;
            next = 3;
        } else {
            spec.dcValue = parseSpiceNumber(t[3]);
            next = 4;
        }
    } catch (const std::exception& e) {
        std::cerr << "Line " << st.lineNo << ": cannot parse V DC value: " << e.what()
                  << " in '" << st.raw << "'\n";
        return;
    }
    if (!parseAcSpec(t, next, st.lineNo, st.raw, spec)) return;

    if (parsePulseOrPwl(t, next, st.lineNo, st.raw, spec)) {
        // superset of the reference dialect, see above
    } else if (next < t.size() && toLower(t[next]) == "sin") {
        // SIN v0 va freq [td [phi]] -- td in seconds, phi in radians
        if (t.size() < next + 4) {
            std::cerr << "Line " << st.lineNo << ": SIN needs at least 3 parameters (v0 va freq): "
                      << st.raw << "\n";
        } else {
            try {
                SinSpec s;
                s.v0   = parseSpiceNumber(t[next + 1]);
                s.va   = parseSpiceNumber(t[next + 2]);
                s.freq = parseSpiceNumber(t[next + 3]);
                if (t.size() > next + 4) s.td  = parseSpiceNumber(t[next + 4]);
                if (t.size() > next + 5) s.phi = parseSpiceNumber(t[next + 5]);
                spec.tran.type = WaveformType::SIN;
                spec.tran.sine = s;
            } catch (const std::exception& e) {
                std::cerr << "Line " << st.lineNo << ": cannot parse SIN parameters: " << e.what()
                          << " in '" << st.raw << "'\n";
            }
        }
    }
    ckt.addVoltageSource(t[0], t[1], t[2], spec);
}

// Iname np nm [DC] value [AC mag [phase]]   (+ optional PULSE / PWL waveform: superset, see above)
// Iname np nm AC mag [phase]                 (no DC value: 0)
void NetlistParser::currentSource(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 4) {
        std::cerr << "Line " << st.lineNo << ": invalid current source: " << st.raw << "\n";
        return;
    }
    SourceSpec spec;
    try {
        const bool dcForm = t.size() >= 5 && toLower(t[3]) == "dc";
        if (startsWithKeyword(t[3], "pulse") || startsWithKeyword(t[3], "pwl")) {
            parsePulseOrPwl(t, 3, st.lineNo, st.raw, spec);
        } else {
            std::size_t next = 3;
            if (toLower(t[3]) != "ac") {
                spec.dcValue = parseSpiceNumber(dcForm ? t[4] : t[3]);
                next = dcForm ? 5 : 4;
            }
            if (!parseAcSpec(t, next, st.lineNo, st.raw, spec)) return;
            parsePulseOrPwl(t, next, st.lineNo, st.raw, spec);
        }
    } catch (const std::exception& e) {
        std::cerr << "Line " << st.lineNo << ": cannot parse I value: " << e.what()
                  << " in '" << st.raw << "'\n";
        return;
    }
    ckt.addCurrentSource(t[0], t[1], t[2], spec);
}

// Mname nd ng ns model W L            (7 tokens)
// Mname nd ng ns <p|n> W L modelId    (8 tokens; the type letter is ignored)
void NetlistParser::mosfet(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() != 7 && t.size() != 8) {
        std::cerr << "Line " << st.lineNo << ": invalid MOSFET: " << st.raw << "\n";
        return;
    }
    const std::string modelId = (t.size() == 7) ? t[4] : t.back();
    double W = 0.0, L = 0.0;
    try {
        W = parseSpiceNumber(t[5]);
        L = parseSpiceNumber(t[6]);
    } catch (const std::exception& e) {
        std::cerr << "Line " << st.lineNo << ": cannot parse MOS W/L: " << e.what()
                  << " in '" << st.raw << "'\n";
        return;
    }
    ckt.addMosfet(t[0], t[1], t[2], t[3], modelId, W, L);
}

void NetlistParser::dotCard(const Statement& st)
{
    const std::string head = toLower(st.tokens[0]);
    if      (head == ".op")     sim.doOp = true;
    else if (head == ".dc")     dcCard(st);
    else if (head == ".tran")   tranCard(st);
    else if (head == ".ac")     acCard(st);
    else if (head == ".noise")  noiseCard(st);
    else if (head == ".sp")     spCard(st);
    else if (head == ".disto")  distoCard(st);
    else if (head == ".imd")    imdCard(st);
    else if (head == ".stb")    stbCard(st);
    else if (head == ".pz")     pzCard(st);
    else if (head == ".print")  printCard(st);
    else if (head == ".model")  modelCard(st);
    else if (head == ".hb")     hbCard(st);
    else if (head == ".pac")    pacCard(st);
    else if (head == ".pnoise") pnoiseCard(st);
    else if (head == ".plotnv") plotNvCard(st);
    else if (head == ".plotnc") plotNcCard(st);
    else std::cerr << "Line " << st.lineNo << ": unsupported control card: " << st.raw << "\n";
}

// .DC src start stop step   (recorded; executed by the batch API as a sweep axis)
void NetlistParser::dcCard(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 5) {
        std::cerr << "Line " << st.lineNo << ": invalid .DC syntax: " << st.raw << "\n";
        return;
    }
    DCSweepConfig dc;
    dc.sourceName = t[1];
    try {
        dc.start = parseSpiceNumber(t[2]);
        dc.stop  = parseSpiceNumber(t[3]);
        dc.step  = parseSpiceNumber(t[4]);
    } catch (const std::exception& e) {
        std::cerr << "Line " << st.lineNo << ": cannot parse .DC numbers: " << e.what()
                  << " in '" << st.raw << "'\n";
        return;
    }
    sim.dcSweeps.push_back(dc);
}

// .TRAN tstep tstop [tstart]
void NetlistParser::tranCard(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 3) {
        std::cerr << "Line " << st.lineNo << ": invalid .TRAN syntax: " << st.raw << "\n";
        return;
    }
    TranConfig cfg;
    try {
        cfg.tstep  = parseSpiceNumber(t[1]);
        cfg.tstop  = parseSpiceNumber(t[2]);
        cfg.tstart = t.size() >= 4 ? parseSpiceNumber(t[3]) : 0.0;
    } catch (const std::exception& e) {
        std::cerr << "Line " << st.lineNo << ": cannot parse .TRAN numbers: " << e.what()
                  << " in '" << st.raw << "'\n";
        return;
    }
    cfg.enabled = true;
    sim.tran = cfg;
}

// ---- what the sweep cards share: each rule is written once ---------------------

void NetlistParser::invalidSyntax(const Statement& st, const char* card)
{
    std::cerr << "Line " << st.lineNo << ": invalid " << card << " syntax: " << st.raw << "\n";
}

bool NetlistParser::cannotParse(const Statement& st, const char* card, const char* what)
{
    std::cerr << "Line " << st.lineNo << ": cannot parse " << card << " arguments: " << what << " in '" << st.raw << "'\n";
    return false;
}

// LIN | OCT | DEC in either case -> out.  Any other word is DEC; strict: and false (the reference's .AC takes any word
// for DEC, src/parser.cpp:435-439; the cards added here refuse it)
bool NetlistParser::sweepWord(const std::string& token, bool strict, AcSweepType& out)
{
    const std::string w = toLower(token);
    out = w == "lin" ? AcSweepType::LIN : (w == "oct" ? AcSweepType::OCT : AcSweepType::DEC);
    return !strict || w == "lin" || w == "oct" || w == "dec";
}

// npoints fstart fstop at t[at .. at + 2] -> the grid, enabled.  A trailing tail of the point count is accepted (stoi).
bool NetlistParser::sweepGrid(const Statement& st, const std::vector<std::string>& t, std::size_t at, const char* card,
                              AcConfig& grid)
{
    try {
        grid.nPoints = std::stoi(t[at]);
        grid.fstart  = parseSpiceNumber(t[at + 1]);
        grid.fstop   = parseSpiceNumber(t[at + 2]);
    } catch (const std::exception& e) {
        return cannotParse(st, card, e.what());
    }
    grid.enabled = true;
    return true;
}

// nside: a whole number >= 0, nothing after it; reported as the grid's numbers are
bool NetlistParser::sideCount(const Statement& st, const std::string& token, const char* card, int& nSide)
{
    try {
        std::size_t used = 0;
        nSide = std::stoi(token, &used);
        if (used != token.size() || nSide < 0) throw std::invalid_argument("nside must be a whole number >= 0");
    } catch (const std::exception& e) {
        return cannotParse(st, card, e.what());
    }
    return true;
}

// the output may be written with blanks inside its parentheses: the tokens with t[1] joined up to the closing one
std::vector<std::string> NetlistParser::joinOutput(const std::vector<std::string>& tokens)
{
    std::vector<std::string> t;
    for (std::size_t i = 0; i < tokens.size(); ++i) {
        if (i >= 2 && t.size() == 2 && t[1].find('(') != std::string::npos && t[1].find(')') == std::string::npos)
            t[1] += tokens[i];
        else
            t.push_back(tokens[i]);
    }
    return t;
}

// where the sweep word of V(out[,ref]) [src] {sweep} ... stands: at 2 when the source is left out, else 3
std::size_t NetlistParser::sweepAfterOutput(const std::vector<std::string>& t)
{
    AcSweepType word;
    return t.size() > 2 && sweepWord(t[2], true, word) ? 2 : 3;
}

// t[1] = V(node) | V(node,ref), and t[2] the source when the sweep word stands at 3
bool NetlistParser::outputPair(const Statement& st, const std::vector<std::string>& t, std::size_t at, const char* card,
                               OutputPair& out)
{
    const ProbeSpec p = probeFromToken(t[1]);
    if ((p.kind != ProbeKind::NodeVoltage && p.kind != ProbeKind::DiffVoltage) || p.node1.empty()) {
        std::cerr << "Line " << st.lineNo << ": " << card << " output must be V(node) or V(node,ref): " << st.raw << "\n";
        return false;
    }
    out.outNode = p.node1;
    out.refNode = p.node2;
    if (at == 3) out.srcName = t[2];
    return true;
}

// ---- the cards: token count and sweep word, then the output, then the numbers; a card that fails changes nothing ----

// .AC {LIN|DEC|OCT} npoints fstart fstop   (further tokens are ignored)
void NetlistParser::acCard(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 5) return invalidSyntax(st, ".AC");
    AcConfig cfg;
    sweepWord(t[1], false, cfg.sweepType);
    if (sweepGrid(st, t, 2, ".AC", cfg)) sim.ac = cfg;
}

// .SP {LIN|DEC|OCT} npoints fstart fstop [0|1]   (a sixth token 1: noise too; anything else is ignored)
void NetlistParser::spCard(const Statement& st)
{
    const auto& t = st.tokens;
    SpConfig cfg;
    if (t.size() < 5 || !sweepWord(t[1], true, cfg.sweepType)) return invalidSyntax(st, ".SP");
    if (!sweepGrid(st, t, 2, ".SP", cfg)) return;
    cfg.doNoise = t.size() > 5 && t[5] == "1";
    sim.sp = cfg;
}

// .NOISE V(out[,ref]) [src] {LIN|DEC|OCT} npoints fstart fstop   (further tokens are ignored)
void NetlistParser::noiseCard(const Statement& st)
{
    const std::vector<std::string> t = joinOutput(st.tokens);
    const std::size_t at = sweepAfterOutput(t);
    NoiseConfig cfg;
    if (t.size() < at + 4 || !sweepWord(t[at], true, cfg.sweepType)) return invalidSyntax(st, ".NOISE");
    if (outputPair(st, t, at, ".NOISE", cfg) && sweepGrid(st, t, at + 1, ".NOISE", cfg)) sim.noise = cfg;
}

// .DISTO V(out[,ref]) {LIN|DEC|OCT} npoints fstart fstop   (single tone: a further token, ngspice's f2overf1, is an error)
void NetlistParser::distoCard(const Statement& st)
{
    const std::vector<std::string> t = joinOutput(st.tokens);
    DistoConfig cfg;
    if (t.size() != 6 || !sweepWord(t[2], true, cfg.sweepType)) return invalidSyntax(st, ".DISTO");
    if (outputPair(st, t, 2, ".DISTO", cfg) && sweepGrid(st, t, 3, ".DISTO", cfg)) sim.disto = cfg;
}

// .IMD V(out[,ref]) {LIN|DEC|OCT} npoints fstart fstop f2overf1   (two tones: f1 sweeps the grid, f2 = f2overf1 * fstart;
// 0 < f2overf1 < 1; any other token count is an error)
void NetlistParser::imdCard(const Statement& st)
{
    const std::vector<std::string> t = joinOutput(st.tokens);
    ImdConfig cfg;
    if (t.size() != 7 || !sweepWord(t[2], true, cfg.sweepType)) return invalidSyntax(st, ".IMD");
    if (!outputPair(st, t, 2, ".IMD", cfg) || !sweepGrid(st, t, 3, ".IMD", cfg)) return;
    try {
        cfg.f2overf1 = parseSpiceNumber(t[6]);
        if (!(cfg.f2overf1 > 0.0 && cfg.f2overf1 < 1.0)) throw std::invalid_argument("f2overf1 must lie between 0 and 1");
    } catch (const std::exception& e) {
        cannotParse(st, ".IMD", e.what());
        return;
    }
    sim.imd = cfg;
}

// .STB Vprobe {LIN|DEC|OCT} npoints fstart fstop   (any other token count is an error)
void NetlistParser::stbCard(const Statement& st)
{
    const auto& t = st.tokens;
    StbConfig cfg;
    if (t.size() != 6 || !sweepWord(t[2], true, cfg.sweepType)) return invalidSyntax(st, ".STB");
    cfg.probeName = t[1];
    if (sweepGrid(st, t, 3, ".STB", cfg)) sim.stb = cfg;
}

// .PZ POL fmax [sigma0]   (poles only: ZER and PZ are refused by name; any other token count is an error)
void NetlistParser::pzCard(const Statement& st)
{
    const auto& t = st.tokens;
    const std::string what = t.size() > 1 ? toLower(t[1]) : std::string();
    if (what == "zer" || what == "pz") {
        std::cerr << "Line " << st.lineNo << ": .PZ supports POL only: " << st.raw << "\n";
        return;
    }
    if ((t.size() != 3 && t.size() != 4) || what != "pol") return invalidSyntax(st, ".PZ");
    PzConfig cfg;
    try {
        cfg.fmax = parseSpiceNumber(t[2]);
        if (t.size() == 4) cfg.sigma0 = parseSpiceNumber(t[3]);
    } catch (const std::exception& e) {
        cannotParse(st, ".PZ", e.what());
        return;
    }
    cfg.enabled = true;
    sim.pz = cfg;
}

// .HB f0 nharm
void NetlistParser::hbCard(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 3) {
        std::cerr << "Line " << st.lineNo << ": invalid .hb syntax: " << st.raw << "\n";
        return;
    }
    HbConfig cfg;
    try {
        cfg.f0 = parseSpiceNumber(t[1]);
        cfg.nHarm = std::stoi(t[2]);
    } catch (const std::exception& e) {
        std::cerr << "Line " << st.lineNo << ": cannot parse .hb arguments: " << e.what()
                  << " in '" << st.raw << "'\n";
        return;
    }
    cfg.enabled = true;
    sim.hb = cfg;
}

// .PAC {LIN|DEC|OCT} npoints fstart fstop [nside]   (nside defaults to 1; any other token count is an error)
void NetlistParser::pacCard(const Statement& st)
{
    const auto& t = st.tokens;
    PacConfig cfg;
    if ((t.size() != 5 && t.size() != 6) || !sweepWord(t[1], true, cfg.sweepType)) return invalidSyntax(st, ".PAC");
    if (!sweepGrid(st, t, 2, ".PAC", cfg)) return;
    if (t.size() == 6 && !sideCount(st, t[5], ".PAC", cfg.nSide)) return;
    sim.pac = cfg;
}

// .PNOISE V(out[,ref]) [src] {LIN|DEC|OCT} npoints fstart fstop [nside]: the output and source of .NOISE, the grid and
// nside of .PAC (nside defaults to 1; any other token count is an error)
void NetlistParser::pnoiseCard(const Statement& st)
{
    const std::vector<std::string> t = joinOutput(st.tokens);
    const std::size_t at = sweepAfterOutput(t);
    PnoiseConfig cfg;
    if ((t.size() != at + 4 && t.size() != at + 5) || !sweepWord(t[at], true, cfg.sweepType)) return invalidSyntax(st, ".PNOISE");
    if (!outputPair(st, t, at, ".PNOISE", cfg) || !sweepGrid(st, t, at + 1, ".PNOISE", cfg)) return;
    if (t.size() == at + 5 && !sideCount(st, t[at + 4], ".PNOISE", cfg.nSide)) return;
    sim.pnoise = cfg;
}

// V(n) | V(n1,n2) | I(elem)
ProbeSpec NetlistParser::probeFromToken(const std::string& token)
{
    ProbeSpec p;
    p.expr = token;
    if (token.empty()) return p;

    int open = -1, close = -1;
    parenSpan(token, open, close);
    const bool hasArg = open >= 0 && close > open + 1;
    const std::string inside = hasArg
        ? token.substr(static_cast<std::size_t>(open + 1), static_cast<std::size_t>(close - open - 1))
        : std::string();

    const char head = upperHead(token);
    if (head == 'V') {
        p.kind = ProbeKind::NodeVoltage;
        if (hasArg) {
            const std::size_t comma = inside.find(',');
            if (comma == std::string::npos) {
                p.node1 = rtrim(ltrim(inside));
            } else {
                p.node1 = rtrim(ltrim(inside.substr(0, comma)));
                p.node2 = rtrim(ltrim(inside.substr(comma + 1)));
                p.kind = ProbeKind::DiffVoltage;
            }
        }
    } else if (head == 'I') {
        p.kind = ProbeKind::BranchCurrent;
        if (hasArg) p.eleName = rtrim(ltrim(inside));
    }
    return p;
}

// .PRINT <analysis> probe...
void NetlistParser::printCard(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 3) {
        std::cerr << "Line " << st.lineNo << ": invalid .PRINT: " << st.raw << "\n";
        return;
    }
    PrintCommand pc;
    pc.analysis = analysisFromToken(t[1]);
    if (pc.analysis == AnalysisType::NONE) {
        std::cerr << "Line " << st.lineNo << ": unknown analysis type in .PRINT: " << t[1]
                  << " in '" << st.raw << "'\n";
        return;
    }
    for (std::size_t i = 2; i < t.size(); ++i) pc.probes.push_back(probeFromToken(t[i]));
    sim.printCommands.push_back(std::move(pc));
}

// .PLOTNV node...   (node voltages, not tied to an analysis)
void NetlistParser::plotNvCard(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 2) {
        std::cerr << "Line " << st.lineNo << ": invalid .PLOTNV: " << st.raw << "\n";
        return;
    }
    PrintCommand pc;
    pc.analysis = AnalysisType::NONE;
    for (std::size_t i = 1; i < t.size(); ++i)
        if (!t[i].empty()) pc.probes.push_back(probeFromToken("V(" + t[i] + ")"));
    if (!pc.probes.empty()) sim.printCommands.push_back(std::move(pc));
}

// .PLOTNC elem | elem(port) ...   (branch currents)
void NetlistParser::plotNcCard(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 2) {
        std::cerr << "Line " << st.lineNo << ": invalid .PLOTNC: " << st.raw << "\n";
        return;
    }
    PrintCommand pc;
    pc.analysis = AnalysisType::NONE;
    for (std::size_t i = 1; i < t.size(); ++i) {
        const std::string& tok = t[i];
        if (tok.empty()) continue;
        ProbeSpec p;
        p.kind = ProbeKind::BranchCurrent;
        p.expr = tok;
        int open = -1, close = -1;
        parenSpan(tok, open, close);
        if (open < 0) {
            p.eleName = tok;
        } else {
            p.eleName = rtrim(ltrim(tok.substr(0, static_cast<std::size_t>(open))));
            p.elePort = rtrim(ltrim(tok.substr(static_cast<std::size_t>(open + 1),
                                               static_cast<std::size_t>(close - open - 1))));
        }
        pc.probes.push_back(std::move(p));
    }
    if (!pc.probes.empty()) sim.printCommands.push_back(std::move(pc));
}

// .MODEL id {VT|MU|COX|LAMBDA|CJ0|CJO value}...   sign of VT selects PMOS
void NetlistParser::modelCard(const Statement& st)
{
    const auto& t = st.tokens;
    if (t.size() < 4) {
        std::cerr << "Line " << st.lineNo << ": invalid .MODEL: " << st.raw << "\n";
        return;
    }
    MosModel m;
    m.name = t[1];
    for (std::size_t i = 2; i + 1 < t.size(); i += 2) {
        const std::string key = toLower(t[i]);
        double val = 0.0;
        try {
            val = parseSpiceNumber(t[i + 1]);
        } catch (const std::exception& e) {
            std::cerr << "Line " << st.lineNo << ": cannot parse .MODEL param " << t[i] << " = "
                      << t[i + 1] << " : " << e.what() << "\n";
            return;
        }
        if      (key == "vt")     m.VT = val;
        else if (key == "mu")     m.MU = val;
        else if (key == "cox")    m.COX = val;
        else if (key == "lambda") m.LAMBDA = val;
        else if (key == "cj0" || key == "cjo") m.CJO = val;
    }
    m.isP = m.VT < 0.0;
    if (m.isP) m.VT = -m.VT;
    ckt.addMosModel(m);
}
