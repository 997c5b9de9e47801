// codegen_sym.hpp -- internal to the kernel generators (codegen.cpp, codegen_linear.cpp, codegen_group.cpp).
// Symbolic values over {structural zero, exact constant, run-time value}, the emitter that folds them into
// straight-line code, the lazily assembled matrix [G | I] and the analysis of the reference's pivot rule.
#pragma once

#include "codegen.hpp"

#include <cmath>
#include <cstdio>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

namespace csim {

inline std::size_t sz(int v) { return static_cast<std::size_t>(v); }

// an exact double literal
inline std::string lit(double x)
{
    char buf[64];
    std::snprintf(buf, sizeof buf, "%a", x);
    return std::string("(") + buf + ")";
}

inline std::string intArray(const std::string& name, const std::vector<int32_t>& v)
{
    std::ostringstream o;
    o << "static __device__ const int " << name << "[" << (v.empty() ? 1 : v.size()) << "] = {";
    if (v.empty()) o << "0";
    for (std::size_t i = 0; i < v.size(); ++i) o << (i ? "," : "") << ((i % 32 == 31) ? "\n    " : "") << v[i];
    o << "};\n";
    return o.str();
}

// TRAN source value of element e into `target`: SourceSpec::evalTran with TranWaveform::eval (reference
// include/sim.hpp:75-143,160-162).  P(o) = expression of parameter slot o.
inline void emitTranSourceValue(std::ostream& src, const std::string& i2, const csim_ir& ir, int e,
                                const std::function<std::string(int)>& P, const std::string& target)
{
    const csim_consts& K = ir.k;
    if (ir.wave[e] == CSIM_WAVE_SIN) {
        src << i2 << "if (tNow < " << P(4) << ") " << target << " = " << P(0) << " + " << P(1) << ";\n"
            << i2 << "else " << target << " = " << P(0) << " + (" << P(1) << " + " << P(2)
            << " * sin((2.0 * " << lit(K.pi) << " * " << P(3) << ") * (tNow - " << P(4) << ") + " << P(5) << "));\n";
    } else if (ir.wave[e] == CSIM_WAVE_PULSE) {
        src << i2 << "{\n"
            << i2 << "    const double v1 = " << P(1) << ", v2 = " << P(2) << ", td = " << P(3) << ", tr = " << P(4)
            << ", tf = " << P(5) << ", ton = " << P(6) << ", per = " << P(7) << ";\n"
            << i2 << "    double w;\n"
            << i2 << "    if (per <= 0.0) {\n"
            << i2 << "        const double tau = tNow - td;\n"
            << i2 << "        if (tau <= 0.0) w = v1;\n"
            << i2 << "        else if (tau < tr) w = v1 + clamp01_cg(tau / tr) * (v2 - v1);\n"
            << i2 << "        else if (tau < tr + ton) w = v2;\n"
            << i2 << "        else w = v2 + clamp01_cg((tau - (tr + ton)) / tf) * (v1 - v2);\n"
            << i2 << "    } else if (tNow < td) {\n"
            << i2 << "        w = v1;\n"
            << i2 << "    } else {\n"
            << i2 << "        double tau = fmod(tNow - td, per);\n"
            << i2 << "        if (tau < 0.0) tau += per;\n"
            << i2 << "        if (tau < tr) w = v1 + (v2 - v1) * clamp01_cg(tau / tr);\n"
            << i2 << "        else if (tau < tr + ton) w = v2;\n"
            << i2 << "        else if (tau < tr + ton + tf) w = v2 + (v1 - v2) * clamp01_cg((tau - (tr + ton)) / tf);\n"
            << i2 << "        else w = v1;\n"
            << i2 << "    }\n"
            << i2 << "    " << target << " = " << P(0) << " + w;\n"
            << i2 << "}\n";
    } else if (ir.wave[e] == CSIM_WAVE_PWL) {
        const int n = ir.wave_n[e];
        auto PT = [&](int i) { return P(1 + i); };
        auto PV = [&](int i) { return P(1 + n + i); };
        src << i2 << "{\n" << i2 << "    double w;\n";
        if (n <= 0) {
            src << i2 << "    w = 0.0;\n";
        } else {
            src << i2 << "    if (tNow <= " << PT(0) << ") w = " << PV(0) << ";\n"
                << i2 << "    else if (tNow >= " << PT(n - 1) << ") w = " << PV(n - 1) << ";\n";
            for (int i = 0; i + 1 < n; ++i)
                src << i2 << "    else if (tNow > " << PT(i) << " && tNow <= " << PT(i + 1) << ") { const double ta = " << PT(i)
                    << ", tb = " << PT(i + 1) << ", va = " << PV(i) << ", vb = " << PV(i + 1)
                    << "; w = va + (vb - va) * ((tNow - ta) / (tb - ta)); }\n";
            src << i2 << "    else w = " << PV(n - 1) << ";\n";
        }
        src << i2 << "    " << target << " = " << P(0) << " + w;\n" << i2 << "}\n";
    } else {
        src << i2 << target << " = " << P(0) << " + 0.0;\n";
    }
}

// abstract value: structural zero, exact constant, or an expression evaluated at run time
struct Sym {
    enum Kind { ZERO, CONST, DYN } kind = ZERO;
    double c = 0.0;          // CONST
    std::string e;           // DYN: a variable name or an expression
    bool neg = false;        // DYN: the value is -(e)
    static Sym konst(double x) { Sym a; if (x == 0.0) return a; a.kind = CONST; a.c = x; return a; }
    static Sym dyn(const std::string& s, bool n = false) { Sym a; a.kind = DYN; a.e = s; a.neg = n; return a; }
    bool isZero() const { return kind == ZERO; }
};

// Emits one `const double <prefix><n> = ...;` per operation that is not folded: a - 0*b == a, a factor of
// exactly +-1 multiplies by a sign, constants fold.  Operation counts go to `stats` when it is set.
struct SymGen {
    std::ostringstream out;
    std::string ind, prefix;
    CodegenStats* stats = nullptr;
    int tmp = 0;

    SymGen(const std::string& indent, const std::string& tempPrefix, CodegenStats* st = nullptr)
        : ind(indent), prefix(tempPrefix), stats(st) {}
    void count(int CodegenStats::*field) { if (stats) ++(stats->*field); }
    std::string ref(const Sym& a) const
    {
        if (a.kind == Sym::CONST) return lit(a.c);
        if (a.kind == Sym::DYN) return a.neg ? "(-" + a.e + ")" : a.e;
        return "0.0";
    }
    Sym emit(const std::string& expr)
    {
        const std::string n = prefix + std::to_string(tmp++);
        out << ind << "const double " << n << " = " << expr << ";\n";
        return Sym::dyn(n);
    }
    static Sym negate(Sym a)
    {
        if (a.kind == Sym::CONST) a.c = -a.c;
        else if (a.kind == Sym::DYN) a.neg = !a.neg;
        return a;
    }
    Sym mul(const Sym& a, const Sym& b)                   // a * b
    {
        if (a.isZero() || b.isZero()) return Sym();
        if (a.kind == Sym::CONST && b.kind == Sym::CONST) return Sym::konst(a.c * b.c);
        if (a.kind == Sym::CONST || b.kind == Sym::CONST) {
            const Sym& k = a.kind == Sym::CONST ? a : b;
            const Sym& d = a.kind == Sym::CONST ? b : a;
            if (k.c == 1.0) return d;
            if (k.c == -1.0) return negate(d);
            count(&CodegenStats::nMul);
            return emit(lit(k.c) + " * " + ref(d));
        }
        count(&CodegenStats::nMul);
        Sym r = emit(a.e + " * " + b.e);
        r.neg = a.neg != b.neg;
        return r;
    }
    Sym div(const Sym& a, const Sym& b)                   // a / b, a true division (solver.hpp:71 and :126)
    {
        if (a.isZero()) return Sym();
        if (a.kind == Sym::CONST && b.kind == Sym::CONST) return Sym::konst(a.c / b.c);
        if (b.kind == Sym::CONST) {
            if (b.c == 1.0) return a;
            if (b.c == -1.0) return negate(a);
            return emit(ref(a) + " / " + lit(b.c));
        }
        Sym r = emit((a.kind == Sym::CONST ? lit(a.c) : a.e) + " / " + b.e);
        r.neg = (a.kind == Sym::DYN && a.neg) != b.neg;
        return r;
    }
    Sym fnma(const Sym& a, const Sym& f, const Sym& u)    // a - f*u
    {
        if (f.isZero() || u.isZero()) return a;
        if (a.isZero()) return negate(mul(f, u));
        if (f.kind == Sym::CONST && u.kind == Sym::CONST) {
            const double p = f.c * u.c;
            if (a.kind == Sym::CONST) return Sym::konst(a.c - p);
            count(&CodegenStats::nAddSub);
            return emit(ref(a) + " - " + lit(p));
        }
        // fold exact +-1 factors into an add/sub
        const bool f1 = f.kind == Sym::CONST && std::fabs(f.c) == 1.0, u1 = u.kind == Sym::CONST && std::fabs(u.c) == 1.0;
        if (f1 || u1) {
            Sym w = f1 ? u : f;
            if ((f1 ? f.c : u.c) < 0) w = negate(w);
            count(&CodegenStats::nAddSub);
            return emit(ref(a) + " - " + ref(w));
        }
        count(&CodegenStats::nFma);
        return emit(ref(a) + " - " + ref(f) + " * " + ref(u));
    }
    Sym orderedSum(const std::vector<Sym>& terms)         // signed terms in the reference's accumulation order
    {
        bool allConst = true;
        for (const Sym& t : terms) allConst = allConst && t.kind != Sym::DYN;
        if (allConst) {
            double acc = 0.0;
            for (const Sym& t : terms) acc = acc + (t.kind == Sym::CONST ? t.c : 0.0);
            return Sym::konst(acc);
        }
        std::vector<Sym> nz;
        for (const Sym& t : terms) if (!t.isZero()) nz.push_back(t);
        if (nz.size() == 1) return nz[0];
        std::string e;
        for (std::size_t i = 0; i < nz.size(); ++i) {
            const Sym& t = nz[i];
            if (i == 0) { e = ref(t); continue; }
            if (t.kind == Sym::DYN) e = "(" + e + (t.neg ? " - " : " + ") + t.e + ")";
            else e = "(" + e + " + " + lit(t.c) + ")";
            count(&CodegenStats::nAddSub);
        }
        return emit(e);
    }
};

// A matrix assembled symbolically from a gather plan (plan.cpp, the reference's stamping order), the right-hand side
// (if any) in the last column.  All-constant entries are resolved at once (they cost no code and decide the zero
// pattern); any other entry is only RECORDED and its code is emitted when the elimination first reads it (shortens
// live ranges: every entry would otherwise be live at once).  A recorded entry reads as a non-zero marker in cell().
struct LazyMatrix {
    SymGen& g;
    std::vector<std::vector<Sym>> M;
    std::vector<std::vector<std::vector<Sym>>> pend;

    LazyMatrix(SymGen& gen, int rows, int cols)
        : g(gen), M(sz(rows), std::vector<Sym>(sz(cols))), pend(sz(rows), std::vector<std::vector<Sym>>(sz(cols))) {}
    // G entries (withG) and / or I entries (withI, into the last column); term[t] = value of term t
    void assemble(const GatherPlan& gp, int LD, const std::vector<Sym>& term, bool withG, bool withI)
    {
        auto terms = [&](const std::vector<int32_t>& ptr, const std::vector<int32_t>& con, int n) {
            std::vector<Sym> t;
            for (int c = ptr[sz(n)]; c < ptr[sz(n + 1)]; ++c)
                t.push_back((con[sz(c)] & 1) ? SymGen::negate(term[sz(con[sz(c)] >> 1)]) : term[sz(con[sz(c)] >> 1)]);
            return t;
        };
        for (int n = 0; withG && n < gp.nnzG(); ++n) record(gp.gPos[sz(n)] / LD, gp.gPos[sz(n)] % LD, terms(gp.gPtr, gp.gCon, n));
        for (int n = 0; withI && n < gp.nnzI(); ++n) record(gp.iRow[sz(n)], static_cast<int>(M[0].size()) - 1, terms(gp.iPtr, gp.iCon, n));
    }
    void record(int r, int c, const std::vector<Sym>& terms)
    {
        bool allConst = true;
        for (const Sym& t : terms) allConst = allConst && t.kind != Sym::DYN;
        if (allConst) cell(r, c) = g.orderedSum(terms);
        else { pend[sz(r)][sz(c)] = terms; cell(r, c) = Sym::dyn("?"); }
    }
    Sym& cell(int r, int c) { return M[sz(r)][sz(c)]; }      // without materialising
    Sym& at(int r, int c)                                     // materialised on first read
    {
        std::vector<Sym>& p = pend[sz(r)][sz(c)];
        if (!p.empty()) { cell(r, c) = g.orderedSum(p); p.clear(); }
        return cell(r, c);
    }
    void swapRows(int a, int b) { std::swap(M[sz(a)], M[sz(b)]); std::swap(pend[sz(a)], pend[sz(b)]); }
};

// The reference's pivot rule (solver.hpp:48-61): the FIRST row attaining the column maximum -- strictly greater than
// every row before the scheduled one, at least as large as every row after it -- and at least lu_eps.  For column k
// with scheduled row p (pivot non-zero): the rows that exact constants decide already, and the run-time tests left.
struct PivotRule {
    bool contradiction = false;     // the schedule contradicts exact constants: it can never hold
    std::string absP;               // |pivot| as an expression
    std::string maxBefore, maxAfter;// running maxima (fmax) of the candidates' magnitudes before / after row p ("" = none)
    std::vector<std::string> conds; // every run-time test in row order, lu_eps first for a run-time pivot
};

inline PivotRule analysePivot(LazyMatrix& A, int k, int p, double luEps)
{
    PivotRule r;
    const Sym pv = A.at(p, k);
    auto absOf = [](const Sym& v) { return v.kind == Sym::CONST ? lit(std::fabs(v.c)) : "fabs(" + v.e + ")"; };
    r.absP = absOf(pv);
    if (pv.kind == Sym::DYN) r.conds.push_back("(" + r.absP + " >= " + lit(luEps) + ")");
    else if (std::fabs(pv.c) < luEps) r.contradiction = true;
    for (int i = k; i < static_cast<int>(A.M.size()); ++i) {
        if (i == p) continue;
        const Sym& ai = A.at(i, k);
        if (ai.isZero()) continue;
        const bool before = i < p;
        if (ai.kind == Sym::CONST && pv.kind == Sym::CONST) {
            if (!(before ? std::fabs(pv.c) > std::fabs(ai.c) : std::fabs(pv.c) >= std::fabs(ai.c))) r.contradiction = true;
            continue;
        }
        const std::string absI = absOf(ai);
        r.conds.push_back("(" + r.absP + (before ? " > " : " >= ") + absI + ")");
        std::string& m = before ? r.maxBefore : r.maxAfter;
        m = m.empty() ? absI : "fmax(" + m + ", " + absI + ")";
    }
    return r;
}

} // namespace csim
