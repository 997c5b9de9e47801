"""Two-port noise analysis, GPU-free parts: the arithmetic of engine/ac_port_noise.hpp compiled for the host against
tests/spnoise_reference.py bit for bit, the physics of the definition against closed forms (Nyquist / Twiss on passive
networks, NF of an attenuator, the F(Ys) identity against a brute-force noise analysis), the .SP card's noise token, and
the register budget of the kernels.

The physics tests, test_case_set_coverage and test_cy_diagonal_is_the_noise_analysis run the numpy reference alone: they
pin the reference (and with it the definition), not the engine.  The engine is held to that reference bit for bit by
test_host_equals_reference_bitwise here and by the GPU test files."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ac_cases as cs
import noise_reference as nref
import spnoise_cases as spc
import spnoise_reference as spnref
from conftest import ROOT, has_gpu, netlist_path

ENGINE_DIR = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")

HOST_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ac_port_noise.hpp"
// binary records on stdin -- int32 n, P, S, F; G [n][n], C [n][n] row-major; omega [F]; port_eq [P] int32; z0 [P];
// src_a [S], src_b [S] int32; psd [S]
// one line per frequency: flags, x [P][n] (re im), y [P][P], cy [P][P], and with P == 2 nf fmin rn yopt.re yopt.im
int main()
{
    int32_t hd[4];
    while (std::fread(hd, sizeof(int32_t), 4, stdin) == 4) {
        const int n = hd[0], P = hd[1], S = hd[2], F = hd[3], ld = n + P;
        std::vector<double> G(n * n), C(n * n), om(F), z0(P), psd(S), ar(n * ld), ai(n * ld), xr(P * n), xi(P * n);
        std::vector<double> yr(P * P), yi(P * P), cr(P * P), ci(P * P);
        std::vector<int32_t> pe(P), sa(S), sb(S);
        if (std::fread(G.data(), sizeof(double), G.size(), stdin) != G.size()) return 1;
        if (std::fread(C.data(), sizeof(double), C.size(), stdin) != C.size()) return 1;
        if (std::fread(om.data(), sizeof(double), om.size(), stdin) != om.size()) return 1;
        if (std::fread(pe.data(), sizeof(int32_t), pe.size(), stdin) != pe.size()) return 1;
        if (std::fread(z0.data(), sizeof(double), z0.size(), stdin) != z0.size()) return 1;
        if (std::fread(sa.data(), sizeof(int32_t), sa.size(), stdin) != sa.size()) return 1;
        if (std::fread(sb.data(), sizeof(int32_t), sb.size(), stdin) != sb.size()) return 1;
        if (std::fread(psd.data(), sizeof(double), psd.size(), stdin) != psd.size()) return 1;
        const double kT40 = 4.0 * 1.380649e-23 * 290.0, gs = 1.0 / z0[0];
        for (int f = 0; f < F; ++f) {
            csim::TwoPortNoise tp{};
            const unsigned fl = csim::ac_spnoise_solve(n, G.data(), C.data(), om[f], P, pe.data(), S, sa.data(), sb.data(),
                                                       psd.data(), kT40, gs, 1e-15, ld, ar.data(), ai.data(), xr.data(),
                                                       xi.data(), yr.data(), yi.data(), cr.data(), ci.data(), &tp);
            std::printf("%u", fl);
            for (int e = 0; e < P * n; ++e) std::printf(" %a %a", xr[e], xi[e]);
            for (int e = 0; e < P * P; ++e) std::printf(" %a %a", yr[e], yi[e]);
            for (int e = 0; e < P * P; ++e) std::printf(" %a %a", cr[e], ci[e]);
            if (P == 2) std::printf(" %a %a %a %a %a", tp.nf, tp.fmin, tp.rn, tp.yoptRe, tp.yoptIm);
            std::printf("\n");
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_spn(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("acportnoise")
    exe = d / "drv"
    p = subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-w", "-I" + ENGINE_DIR,
                        "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-", "-o", str(exe)], input=HOST_DRIVER,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def run(systems, omega):
        """systems: list of (G, C, port_eq, z0, src_a, src_b, psd [S]) -> per system dict(per_f, x, y, cy[, nf ...])"""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        blob = []
        for G, Cm, pe, z0, sa, sb, psd in systems:
            blob.append(np.array([G.shape[0], len(pe), len(sa), len(omega)], dtype=np.int32).tobytes()
                        + np.ascontiguousarray(G, dtype=np.float64).tobytes()
                        + np.ascontiguousarray(Cm, dtype=np.float64).tobytes() + omega.tobytes()
                        + np.asarray(pe, dtype=np.int32).tobytes() + np.asarray(z0, dtype=np.float64).tobytes()
                        + np.asarray(sa, dtype=np.int32).tobytes() + np.asarray(sb, dtype=np.int32).tobytes()
                        + np.asarray(psd, dtype=np.float64).tobytes())
        out = subprocess.run([str(exe)], input=b"".join(blob), capture_output=True, check=True).stdout.decode()
        lines = out.splitlines()
        F = len(omega)
        assert len(lines) == len(systems) * F
        res = []
        for k, sy in enumerate(systems):
            n, P = sy[0].shape[0], len(sy[2])
            r = dict(per_f=[], x=np.zeros((F, P, n), dtype=complex), y=np.zeros((F, P, P), dtype=complex),
                     cy=np.zeros((F, P, P), dtype=complex), nf=np.zeros(F), fmin=np.zeros(F), rn=np.zeros(F),
                     yopt=np.zeros(F, dtype=complex))
            for f in range(F):
                tok = lines[k * F + f].split()
                v = np.array([float.fromhex(t) for t in tok[1:]])
                r["per_f"].append(int(tok[0]))
                cut = [0, 2 * P * n, 2 * P * n + 2 * P * P, 2 * P * n + 4 * P * P]
                for key, a, b in (("x", cut[0], cut[1]), ("y", cut[1], cut[2]), ("cy", cut[2], cut[3])):
                    r[key][f].real = v[a:b:2].reshape(r[key][f].shape)       # parts set separately: keeps a -0.0
                    r[key][f].imag = v[a + 1:b:2].reshape(r[key][f].shape)
                if P == 2:
                    r["nf"][f], r["fmin"][f], r["rn"][f] = v[cut[3]:cut[3] + 3]
                    r["yopt"][f:f + 1].real, r["yopt"][f:f + 1].imag = v[cut[3] + 3], v[cut[3] + 4]
            res.append(r)
        return res
    return run


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(x, ref, nan_expected, where):
    """bitwise equality; where NaNs are expected: equal NaN masks, bitwise equality elsewhere"""
    x, ref = np.ascontiguousarray(x), np.ascontiguousarray(ref)
    if not nan_expected:
        assert not np.isnan(ref.view(np.float64)).any(), where
        assert np.array_equal(_bits(x), _bits(ref)), where
        return
    nx, nr = np.isnan(x.view(np.float64)), np.isnan(ref.view(np.float64))
    assert np.array_equal(nx, nr), where
    assert np.array_equal(np.where(nx, 0, _bits(x)), np.where(nr, 0, _bits(ref))), where


# ---- ac_port_noise.hpp, compiled for the host
def test_host_equals_reference_bitwise(host_spn):
    """ac_spnoise_solve() against the reference on every case of tests/spnoise_cases.py: flags, adjoint solutions, Y, Cy
    and the noise parameters bit for bit; a failed frequency is all +0.0"""
    n_sys = n_flagged = 0
    for c in spc.all_cases():
        n, kind, P = c["n"], c["kind"], c["P"]
        ref = spc.reference(c)
        host = host_spn([(c["G"][s], c["C"][s], c["port_eq"], c["z0"], c["src_a"], c["src_b"], c["psd"][s])
                         for s in range(cs.NSYS)], cs.OMEGA)
        for s in range(cs.NSYS):
            where = (kind, n, P, c["S"], s)
            assert host[s]["per_f"] == ref[s]["per_f"], where
            for key in spc.keys(P):                             # Y21 == 0 gets IEEE's answer: NaN parameters from finite data
                _same(host[s][key], ref[s][key], kind in cs.HAS_NAN or key in spc.KEYS2, where + (key,))
            n_sys += 1
            n_flagged += int(ref[s]["flags"] != 0)
            for f, fl in enumerate(ref[s]["per_f"]):
                if fl:
                    for key in spc.keys(P):
                        v = np.ascontiguousarray(host[s][key][f]).view(np.float64)
                        assert np.all(v == 0) and not np.signbit(v).any(), where + (f, key)
    print("%d systems, %d flagged" % (n_sys, n_flagged))
    assert n_flagged > 0


def test_case_set_coverage():
    """what the case set exercises, by the reference alone: per size class row exchanges, ties and skipped zero
    multipliers (ac_cases.Coverage); a system that fails at one frequency only; the Cvv-not-positive branch on finite
    data and the regular branch; every (P, S) combination, and the generator counts around each kernel's lane chunk on
    sizes both kernels cover"""
    cov = cs.Coverage()
    one_freq = cvv_branch = regular = 0
    combos, packed_s = set(), set()
    for c in spc.all_cases():
        ref = spc.reference(c)
        combos.add((c["P"], c["S"]))
        if c["n"] <= 32:
            packed_s.add(c["S"])
        for s in range(cs.NSYS):
            cov.add(c["n"], ref[s]["logs"])
            one_freq += int(0 < sum(1 for fl in ref[s]["per_f"] if fl) < len(cs.OMEGA))
            if c["P"] == 2 and c["kind"] not in cs.HAS_NAN:
                cvv_branch += sum(1 for v in ref[s]["cvv_positive"] if v is False)
                regular += sum(1 for v in ref[s]["cvv_positive"] if v is True)
    cov.check()
    print("%s; one-frequency failures %d, Cvv <= 0 %d, regular %d" % (cov, one_freq, cvv_branch, regular))
    assert one_freq > 0 and cvv_branch > 0 and regular > 0
    assert combos == {(P, S) for P in spc.PORTS for S in spc.S_VALUES}
    assert packed_s == set(spc.S_VALUES)


@pytest.mark.parametrize("n", spc.SIZES)
def test_cy_diagonal_is_the_noise_analysis(n):
    """(d) diag(Cy).re equals, bit for bit, the onoise of the reference of "Noise analysis" taken with the output at the
    port's branch equation; the diagonal's imaginary part is +0.0"""
    for c in spc.all_cases(sizes=(n,)):
        ref = spc.reference(c)
        for s in range(cs.NSYS):
            for i, k in enumerate(c["port_eq"]):
                on = nref.solve_sweep(c["G"][s], c["C"][s], cs.OMEGA, (k, -1), c["src_a"], c["src_b"], c["psd"][s])
                where = (c["kind"], n, s, i)
                assert on["per_f"] == ref[s]["per_f"], where
                _same(ref[s]["cy"][:, i, i].real, on["onoise"], c["kind"] in cs.HAS_NAN, where)
                im = np.ascontiguousarray(ref[s]["cy"][:, i, i].imag)
                assert np.all(im == 0) and not np.signbit(im).any(), where


# ---- physics: the float64 reference against closed forms
LD = np.longdouble
CLD = np.clongdouble
# The small-signal values of M1 in the hand-stamped systems.  They are chosen here, not read from the netlists: the
# operating point takes a DC solve, which is the engine's.  Every R and C value comes from the files.
GM, GDS = 2.0e-3, 1.0e-4


def _stamp(nl, elems):
    """G, C and the generator table of a netlist stamped by hand (no gmin: the definition is the subject, not the
    assembly).  elems: (kind, name, plus, minus, value); "M" is (d, g) with the source at ground: gm from g to d, gds
    at d, the channel generator between d and ground.  -> (G, C, [(name, a, b, conductance)])"""
    n = nl.n_unknowns
    G, C = np.zeros((n, n)), np.zeros((n, n))
    names = nl.eq_names
    gens = []

    def eq(node):
        return -1 if node == "0" else nl.node_eq(node)

    def two(M, a, b, v):
        for r, c, sg in ((a, a, 1), (b, b, 1), (a, b, -1), (b, a, -1)):
            if r >= 0 and c >= 0:
                M[r, c] += sg * v

    for kind, name, p, m, val in elems:
        a, b = eq(p), eq(m)
        if kind == "R":
            two(G, a, b, 1.0 / val)
            gens.append((name, a, b, 1.0 / val))
        elif kind == "C":
            two(C, a, b, val)
        elif kind == "M":                                       # p = drain, m = gate
            G[a, b] += GM
            G[a, a] += GDS
            gens.append((name, a, -1, (2.0 / 3.0) * GM))
        else:                                                   # V or L: a branch equation
            k = nl.n_node_eq + names[nl.n_node_eq:].index(name)
            for node, sg in ((a, 1.0), (b, -1.0)):
                if node >= 0:
                    G[k, node] += sg
                    G[node, k] += sg
            if kind == "L":
                C[k, k] -= val
    return G, C, gens


def _fixture(name, rs=None):
    """-> (netlist, G, C, gens) of a golden circuit; element values as the parser read them"""
    from circuitsimulator_amd import Netlist
    nl = Netlist.from_file(netlist_path(name))
    v = [float(x) for x in nl.nominal_params if x != 0.0]
    if name == "sp_pi_pad.sp":
        assert v == [150.0, 39.0, 220.0]
        el = [("V", "V1", "in", "0", 0), ("V", "V2", "out", "0", 0), ("R", "R1", "in", "0", v[0]),
              ("R", "R2", "in", "out", v[1]), ("R", "R3", "out", "0", v[2])]
    elif name == "sp_rlc_twoport.sp":
        assert np.allclose(v, [2.0, 100e-9, 20e-12, 2e3], rtol=1e-15, atol=0)
        el = [("V", "V1", "p1", "0", 0), ("V", "V2", "p2", "0", 0), ("R", "RS", "p1", "m", v[0]), ("L", "L1", "m", "p2", v[1]),
              ("C", "C1", "p2", "0", v[2]), ("R", "RP", "p2", "0", v[3])]
    else:
        # nominal parameters in element order: VIN's DC, [RS], VDD's DC, [RL], RD, CL, CGD, then M1's model values
        if name == "spn_cs_amp.sp":
            assert v[:2] == [0.9, 3.0]
            rd, cl, cgd = v[2:5]
            el = [("V", "VIN", "g", "0", 0), ("V", "VDD", "vdd", "0", 0)]
        else:
            assert name == "spn_cs_amp_rs.sp" and v[0] == 0.9 and v[2] == 3.0 and v[1] == FYS_RS[0]
            rl, rd, cl, cgd = v[3:7]
            el = [("V", "VIN", "s", "0", 0), ("R", "RS", "s", "g", rs), ("V", "VDD", "vs", "0", 0),
                  ("R", "RL", "vs", "vdd", rl)]
        assert np.allclose([rd, cl, cgd], [5e3, 1e-12, 20e-15], rtol=1e-15, atol=0)
        el += [("R", "RD", "vdd", "d", rd), ("C", "CL", "d", "0", cl), ("C", "CGD", "g", "d", cgd), ("M", "M1", "d", "g", 0)]
    return (nl,) + _stamp(nl, el)


def _table(gens, temp):
    kt4 = spnref.kt4(temp)
    return ([g[1] for g in gens], [g[2] for g in gens], np.array([kt4 * np.float64(g[3]) for g in gens]))


def _solve_ld(A, B):
    """A X = B in numpy.clongdouble by Gaussian elimination with partial pivoting (the systems are small)"""
    A, B = A.astype(CLD).copy(), B.astype(CLD).copy()
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]], B[[k, p]] = A[[p, k]], B[[p, k]]
        for i in range(k + 1, n):
            m = A[i, k] / A[k, k]
            A[i, k:] -= m * A[k, k:]
            B[i] -= m * B[k]
    X = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - A[i, i + 1:] @ X[i + 1:]) / A[i, i]
    return X


def _y_ld(G, C, w, pe):
    """Y of the ports in longdouble: Y(i,j) = -x(j)[k_i] with A x(j) = e_{k_j}"""
    n = G.shape[0]
    A = G.astype(CLD) + 1j * LD(w) * C.astype(CLD)
    E = np.zeros((n, len(pe)), dtype=CLD)
    for j, k in enumerate(pe):
        E[k, j] = 1
    X = _solve_ld(A, E)
    return -X[pe, :]


# Worst relative deviation of the float64 reference from the same quantity in numpy.longdouble, measured once on the
# circuits below; each bound is 16 x that, rounded up to a power of two.  A wrong sign or factor shows up at 1e-1.
NYQUIST_BOUND = 2.0 ** -44        # measured 3.42e-15 (x 16 = 5.5e-14)
PAD_NF_BOUND = 2.0 ** -51         # measured 1.92e-17 (x 16 = 3.1e-16): NF of the pad is within half an ulp of its loss
FYS_BOUND = 2.0 ** -46            # measured 6.88e-16 (x 16 = 1.1e-14)


def measure_nyquist():
    """-> worst |Cy - kT4 Re(Y)| / |kT4 Re(Y)| over the passive circuits, entries and frequencies; also checks (c)"""
    worst = 0.0
    for name in ("sp_pi_pad.sp", "sp_rlc_twoport.sp"):
        nl, G, C, gens = _fixture(name)
        pe, z0 = [p[1] for p in nl.ports], [p[2] for p in nl.ports]
        omega = 2.0 * np.pi * nl.sp_freqs()
        for temp in (290.0, 300.15):
            sa, sb, psd = _table(gens, temp)
            r = spnref.sweep(G, C, omega, pe, z0, sa, sb, psd)
            assert r["per_f"] == [0] * len(omega), name
            assert np.all(r["fmin"] >= 1.0) and np.all(r["fmin"] <= r["nf"]), name
            for f, w in enumerate(omega):
                want = LD(4.0) * LD(1.380649e-23) * LD(temp) * _y_ld(G, C, w, pe).real
                for i in range(2):
                    for j in range(2):
                        worst = max(worst, float(np.abs(CLD(r["cy"][f][i, j]) - want[i, j]) / np.abs(want[i, j])))
    return worst


def measure_pad_nf():
    """-> worst relative deviation of NF at Z0 from 1 / (available gain) on the pad at 290 K"""
    nl, G, C, gens = _fixture("sp_pi_pad.sp")
    pe, z0 = [p[1] for p in nl.ports], [p[2] for p in nl.ports]
    omega = 2.0 * np.pi * nl.sp_freqs()
    sa, sb, psd = _table(gens, 290.0)
    r = spnref.sweep(G, C, omega, pe, z0, sa, sb, psd)
    worst = 0.0
    for f, w in enumerate(omega):
        Y = _y_ld(G, C, w, pe)
        ys = 1 / LD(z0[0])
        yout = Y[1, 1] - Y[0, 1] * Y[1, 0] / (Y[0, 0] + ys)
        ga = np.abs(Y[1, 0]) ** 2 * ys / (yout.real * np.abs(Y[0, 0] + ys) ** 2)
        worst = max(worst, float(np.abs(LD(r["nf"][f]) - 1 / ga) * ga))
    return worst


FYS_RS = (50.0, 200.0, 1000.0)


def measure_fys():
    """(b) the stage of spn_cs_amp.sp driven from RS and loaded by RL (spn_cs_amp_rs.sp): F = (output noise but RL's) /
    (RS's share), by the reference of "Noise analysis" in float64 and by a longdouble solve of the same system, against
    Fmin + (Rn / Gs) |Ys - Yopt|^2 from the two-port parameters, Ys = 1 / RS.  -> worst relative deviation of either
    float64 figure from the longdouble one"""
    nl2, G2, C2, gens2 = _fixture("spn_cs_amp.sp")
    pe, z0 = [p[1] for p in nl2.ports], [p[2] for p in nl2.ports]
    omega = 2.0 * np.pi * nl2.sp_freqs()
    sa, sb, psd = _table(gens2, 290.0)
    tp = spnref.sweep(G2, C2, omega, pe, z0, sa, sb, psd)
    assert tp["per_f"] == [0] * len(omega) and np.all(tp["fmin"] <= tp["nf"]) and np.all(tp["fmin"] >= 1.0)
    worst = 0.0
    for rs in FYS_RS:
        nl, G, C, gens = _fixture("spn_cs_amp_rs.sp", rs)
        names = [g[0] for g in gens]
        a, b, p = _table(gens, 290.0)
        out = nl.node_eq("vdd")
        on = nref.solve_sweep(G, C, omega, (out, -1), a, b, p)
        assert on["per_f"] == [0] * len(omega)
        keep = [s for s, nm in enumerate(names) if nm != "RL"]
        ys = np.float64(1.0) / np.float64(rs)
        for f, w in enumerate(omega):
            brute = on["contrib"][f][keep].sum() / on["contrib"][f][names.index("RS")]
            d = ys - tp["yopt"][f]
            params = tp["fmin"][f] + (tp["rn"][f] / ys) * (d.real * d.real + d.imag * d.imag)
            A = G.astype(CLD) + 1j * LD(w) * C.astype(CLD)
            e = np.zeros((G.shape[0], 1), dtype=CLD)
            e[out, 0] = 1
            lam = _solve_ld(A.T, e)[:, 0]
            z = np.array([(lam[x] if x >= 0 else 0) - (lam[y] if y >= 0 else 0) for x, y in zip(a, b)])
            con = np.abs(z) ** 2 * np.array([LD(v) for v in p])
            exact = con[keep].sum() / con[names.index("RS")]
            for got in (brute, params):
                worst = max(worst, float(np.abs(LD(got) - exact) / exact))
            if rs == z0[0]:                                     # NF itself is F at Ys = 1 / Z0 of port 1
                worst = max(worst, float(np.abs(LD(tp["nf"][f]) - exact) / exact))
    return worst


def test_passive_networks_obey_nyquist():
    """(a) Cy = kT4 Re(Y) entrywise on the pi pad and the RLC two-port at 290 K and 300.15 K (Twiss); (c) 1 <= Fmin <= NF"""
    worst = measure_nyquist()
    print("worst relative deviation %.3g (bound %.3g)" % (worst, NYQUIST_BOUND))
    assert worst <= NYQUIST_BOUND


def test_pad_noise_figure_is_its_loss():
    """(a) at 290 K the NF of the attenuator at Z0 is 1 / (available gain), from Y in numpy.longdouble"""
    worst = measure_pad_nf()
    print("worst relative deviation %.3g (bound %.3g)" % (worst, PAD_NF_BOUND))
    assert worst <= PAD_NF_BOUND


def test_f_of_ys_identity():
    """(b) F(Ys) = Fmin + (Rn / Gs) |Ys - Yopt|^2 equals the brute-force noise factor at RS = 50, 200, 1000 ohm"""
    worst = measure_fys()
    print("worst relative deviation %.3g (bound %.3g)" % (worst, FYS_BOUND))
    assert worst <= FYS_BOUND


# ---- card, ports, arguments
BASE = "* ports\nR1 a b 100\nR2 b 0 50\nC1 b 0 1p\nV1 a 0 DC 0 PORTNUM 1\nV2 b 0 DC 0 PORTNUM 2\n"


def _nl(text):
    from circuitsimulator_amd import Netlist
    return Netlist.from_text(text)


@pytest.mark.parametrize("card,want", [(".SP DEC 3 1 1k 1", True), (".SP DEC 3 1 1k", False), (".SP DEC 3 1 1k 0", False),
                                       (".sp lin 3 1 1k 1", True), (".SP DEC 3 1 1k 2", False),
                                       (".SP DEC 3 1 1k noise", False), (".SP DEC 3 1 1k 1 7", True), ("", False)])
def test_sp_card_noise_token(card, want):
    """a sixth token `1` sets sp_noise; nothing else about the card or the netlist changes"""
    nl = _nl(BASE + card + "\n")
    assert nl.sp_noise is want
    assert nl.sp == (("dec" if "DEC" in card else "lin", 3, 1.0, 1000.0) if card else None)
    assert len(nl.ports) == 2


def test_golden_netlists():
    from circuitsimulator_amd import Netlist
    a, b = Netlist.from_file(netlist_path("spn_cs_amp.sp")), Netlist.from_file(netlist_path("sp_cs_amp.sp"))
    assert a.sp_noise and not b.sp_noise and a.sp == b.sp and a.ports == b.ports
    assert np.array_equal(a.nominal_params, b.nominal_params) and a.eq_names == b.eq_names
    rs = Netlist.from_file(netlist_path("spn_cs_amp_rs.sp"))
    assert rs.ports == [] and rs.noise is not None and rs.noise[0] == rs.node_eq("vdd")
    assert len(rs.noise_sources) == len(a.noise_sources) + 2


@pytest.mark.parametrize("P", [1, 3, 4])
def test_noise_parameters_need_two_ports(P):
    """asking for NF, Fmin, Rn, Yopt with P != 2 is a ValueError before any call into the library"""
    from circuitsimulator_amd import sp_noise_solve_batch
    c = cs.case("dense", 5)
    with pytest.raises(ValueError):
        sp_noise_solve_batch(c["G"], c["C"], list(range(P)), [50.0] * P, [0], [1], np.ones((cs.NSYS, 1)), cs.OMEGA,
                             noise_params=True)


@pytest.mark.skipif(has_gpu(), reason="the machine has a GPU")
def test_without_a_gpu_there_is_no_device():
    from circuitsimulator_amd import CsimError, capi, sp_noise_solve_batch
    c = spc.case("dense", 9)
    with pytest.raises(CsimError) as e:
        sp_noise_solve_batch(c["G"], c["C"], c["port_eq"], c["z0"], c["src_a"], c["src_b"], c["psd"], cs.OMEGA)
    assert e.value.code == capi.CSIM_ERR_NO_DEVICE


# ---- register budget
def test_spnoise_kernel_registers(tmp_path):
    """Tripwire: the register-resident kernel keeps its rows and its correlation sums in registers -- no scratch, no
    spills, in any of its eight instantiations; the two LDS kernels likewise."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "spn.s"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + ENGINE_DIR, "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "api"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ENGINE_DIR, "kernels_spnoise.hip"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    meta, name = {}, None
    for line in asm.read_text().splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.(private_segment_fixed_size|vgpr_spill_count|vgpr_count):\s+(\d+)", line)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    packed = {k: v for k, v in meta.items() if "spn_sweep_packed_kernel" in k}
    wave = {k: v for k, v in meta.items() if "spn_sweep_wave_kernel" in k}
    assert len(packed) == 8 and len(wave) == 2, sorted(meta)
    for k, v in list(packed.items()) + list(wave.items()):
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
    print("VGPRs:", {k[-28:]: v["vgpr_count"] for k, v in list(packed.items()) + list(wave.items())})
