"""Noise analysis, GPU-free parts: the .NOISE card and the generator list, the arithmetic of engine/ac_noise.hpp
compiled for the host against tests/noise_reference.py bit for bit, the accuracy of the definition itself against
an evaluation in numpy.longdouble, and the register budget of the register-resident noise kernel."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ac_cases as cs
import ac_reference
import noise_reference as nref
from conftest import ROOT, netlist_path

ENGINE_DIR = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")
DIVIDER = "* divider\nV1 in 0 DC 1 AC 1\nR1 in out 10k\nR2 out 0 30k\nI1 0 out DC 0\n"


def _nl(text):
    from circuitsimulator_amd import Netlist
    return Netlist.from_text(text)


# ---- the card
@pytest.mark.parametrize("card,out_m,src,grid", [
    (".NOISE V(out) V1 DEC 10 1 1k", None, 0, ("dec", 10, 1.0, 1e3)),
    (".NOISE V(out,in) V1 OCT 3 10 1k", "in", 0, ("oct", 3, 10.0, 1e3)),
    (".NOISE V(out,0) V1 LIN 5 1meg 2meg", None, 0, ("lin", 5, 1e6, 2e6)),
    (".NOISE V(out, in) I1 DEC 2 1 10", "in", 3, ("dec", 2, 1.0, 10.0)),
    (".noise v(out) v1 dec 10 1 1k", None, 0, ("dec", 10, 1.0, 1e3)),
    (".Noise V(out) i1 Lin 3 0 10", None, 3, ("lin", 3, 0.0, 10.0)),
    (".NOISE V(out) DEC 10 1 1k", None, -1, ("dec", 10, 1.0, 1e3)),          # no source named
    (".NOISE V(out) VX DEC 10 1 1k", None, -1, ("dec", 10, 1.0, 1e3)),       # a source the netlist does not have
])
def test_noise_card_forms(card, out_m, src, grid):
    from circuitsimulator_amd.engine import ac_freqs
    nl = _nl(DIVIDER + card + "\n")
    assert nl.n_elems == 4
    want_m = -1 if out_m is None else nl.node_eq(out_m)
    assert nl.noise == (nl.node_eq("out"), want_m, src) + grid
    assert nl.node_eq("out") >= 0 and (out_m is None or want_m >= 0)
    assert np.array_equal(nl.noise_freqs(), ac_freqs(*grid))
    assert nl.ac is None


def test_noise_card_absent_invalid_and_beside_ac():
    from circuitsimulator_amd import capi
    nl = _nl(DIVIDER)
    assert nl.noise is None
    with pytest.raises(capi.CsimError) as e:
        nl.noise_freqs()
    assert e.value.code == capi.CSIM_ERR_CONFIG
    for bad in (".NOISE", ".NOISE V(out) V1 DEC 10 1", ".NOISE I(V1) V1 DEC 10 1 1k", ".NOISE V(out) V1 V2 DEC 10 1 1k",
                ".NOISE V(out) V1 DEC ten 1 1k"):
        assert _nl(DIVIDER + bad + "\n").noise is None, bad
    both = _nl(DIVIDER + ".AC OCT 4 10 1k\n.NOISE V(out) V1 DEC 10 1 1k\n")
    assert both.ac == ("oct", 4, 10.0, 1000.0) and both.noise[3:] == ("dec", 10, 1.0, 1000.0)
    # an output node the netlist does not have: the card is kept, the equation is -2 (refused when used)
    assert _nl(DIVIDER + ".NOISE V(nowhere) V1 DEC 10 1 1k\n").noise[0] == -2


def _expected_sources(text, nl):
    """resistors between their terminals and MOSFETs drain - source, in element order, from the netlist text"""
    out, elem = [], 0
    for line in text.splitlines():
        line = line.split("$")[0].strip()
        if not line or line[0] in "*;.+":
            continue
        tok = line.split()
        head = tok[0][0].upper()
        if head not in "RCLVIM":
            continue
        if head == "R":
            out.append((elem, nl.node_eq(tok[1]), nl.node_eq(tok[2])))
        elif head == "M":
            out.append((elem, nl.node_eq(tok[1]), nl.node_eq(tok[3])))
        elem += 1
    return out, elem


@pytest.mark.parametrize("name,n_r,n_m", [("buffer.sp", 3, 4), ("dbmixer.sp", 9, 6), ("noise_cs_amp.sp", 1, 1),
                                          ("noise_divider.sp", 2, 0), ("noise_rc_lowpass.sp", 1, 0)])
def test_generator_list(name, n_r, n_m):
    from circuitsimulator_amd import Netlist
    text = open(netlist_path(name)).read()
    nl = Netlist.from_file(netlist_path(name))
    want, n_elems = _expected_sources(text, nl)
    assert n_elems == nl.n_elems
    src = nl.noise_sources
    assert src == want
    assert len(src) == n_r + n_m
    assert all(-1 <= a < nl.n_unknowns and -1 <= b < nl.n_unknowns for _, a, b in src)
    assert [e for e, _, _ in src] == sorted(e for e, _, _ in src)


@pytest.mark.parametrize("name,card", [("buffer.sp", ".NOISE V(118) Vin DEC 10 1k 1g"),
                                       ("dbmixer.sp", ".NOISE V(102,103) Vrf1+ DEC 5 1meg 10g")])
def test_shipped_netlists_unchanged_by_noise_card(name, card):
    """A .NOISE card changes neither P, nor the nominal parameters, the equation names, the CSV header, the probes
    or the generator list."""
    from circuitsimulator_amd import Netlist
    text = open(netlist_path(name)).read()
    ref = Netlist.from_text(text)
    assert ref.noise is None
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.strip().lower().startswith(".tran"))
    nz = Netlist.from_text("\n".join(lines[:at] + [card] + lines[at:]) + "\n")
    assert nz.noise is not None and nz.noise[0] >= 0 and nz.noise[2] >= 0
    assert nz.n_params == ref.n_params and nz.n_unknowns == ref.n_unknowns and nz.n_elems == ref.n_elems
    assert np.array_equal(nz.nominal_params, ref.nominal_params)
    assert nz.eq_names == ref.eq_names
    assert nz.csv_header == ref.csv_header
    assert nz.probes == ref.probes
    assert np.array_equal(nz.mc_kinds, ref.mc_kinds)
    assert (nz.tran_enabled, nz.tstep, nz.tstop, nz.tstart) == (ref.tran_enabled, ref.tstep, ref.tstop, ref.tstart)
    assert nz.noise_sources == ref.noise_sources
    if name == "buffer.sp":
        assert nz.n_params == 36


def test_golden_netlists_carry_a_card():
    from circuitsimulator_amd import Netlist
    for name, out, src_name in (("noise_divider.sp", "out", "V1"), ("noise_rc_lowpass.sp", "out", "V1"),
                                ("noise_cs_amp.sp", "d", "VIN")):
        nl = Netlist.from_file(netlist_path(name))
        card = nl.noise
        assert card is not None and card[0] == nl.node_eq(out) and card[1] == -1, name
        assert nl.eq_names[nl.n_node_eq:].count(src_name) == 1 and card[2] >= 0, name
        assert len(nl.noise_freqs()) > 1


# ---- ac_noise_solve(), compiled for the host
HOST_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ac_noise.hpp"
// binary records on stdin -- int32 n, F, S, out_p, out_m, in_kind, in_a, in_b; G [n][n], C [n][n] row-major;
// src_a [S], src_b [S] int32; psd [S]; omega [F] -- one line per frequency: flags, onoise, gain, contrib [S], y [n]
int main()
{
    int32_t hd[8];
    while (std::fread(hd, sizeof(int32_t), 8, stdin) == 8) {
        const int n = hd[0], F = hd[1], S = hd[2], ld = n + 1;
        std::vector<double> G(n * n), C(n * n), psd(S), om(F), ar(n * ld), ai(n * ld), yr(n), yi(n), con(S);
        std::vector<int32_t> sa(S), sb(S);
        if (std::fread(G.data(), sizeof(double), G.size(), stdin) != G.size()) return 1;
        if (std::fread(C.data(), sizeof(double), C.size(), stdin) != C.size()) return 1;
        if (std::fread(sa.data(), sizeof(int32_t), sa.size(), stdin) != sa.size()) return 1;
        if (std::fread(sb.data(), sizeof(int32_t), sb.size(), stdin) != sb.size()) return 1;
        if (std::fread(psd.data(), sizeof(double), psd.size(), stdin) != psd.size()) return 1;
        if (std::fread(om.data(), sizeof(double), om.size(), stdin) != om.size()) return 1;
        for (int f = 0; f < F; ++f) {
            double onoise = -1.0;
            csim::cpx gain = {-1.0, -1.0};
            const unsigned fl = csim::ac_noise_solve(n, G.data(), C.data(), om[f], hd[3], hd[4], S, sa.data(), sb.data(),
                                                     psd.data(), hd[5], hd[6], hd[7], 1e-15, ld, ar.data(), ai.data(),
                                                     yr.data(), yi.data(), con.data(), &onoise, &gain);
            std::printf("%u %a %a %a", fl, onoise, gain.re, gain.im);
            for (int s = 0; s < S; ++s) std::printf(" %a", con[s]);
            for (int i = 0; i < n; ++i) std::printf(" %a %a", yr[i], yi[i]);
            std::printf("\n");
        }
    }
    return 0;
}
"""


def _gain_ints(gain_in):
    if gain_in is None:
        return 0, -1, -1
    return (1, gain_in[1], -1) if gain_in[0] == "v" else (2, gain_in[1], gain_in[2])


@pytest.fixture(scope="module")
def host_noise(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("acnoise")
    cpp, exe = d / "drv.cpp", d / "drv"
    cpp.write_text(HOST_DRIVER)
    p = subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-w", "-I" + ENGINE_DIR,
                        "-I" + os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def run(systems, omega):
        """systems: list of (G, C, setup dict, psd [S]) -> per system dict(per_f, onoise [F], gain [F], contrib [F][S],
        y [F][n]), values exactly as printed (%a)"""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        blob = []
        for G, Cm, st, psd in systems:
            n, S = G.shape[0], len(st["src_a"])
            hd = [n, len(omega), S, st["out"][0], st["out"][1], *_gain_ints(st["gain_in"])]
            blob.append(np.array(hd, dtype=np.int32).tobytes()
                        + np.ascontiguousarray(G, dtype=np.float64).tobytes()
                        + np.ascontiguousarray(Cm, dtype=np.float64).tobytes()
                        + np.ascontiguousarray(st["src_a"], dtype=np.int32).tobytes()
                        + np.ascontiguousarray(st["src_b"], dtype=np.int32).tobytes()
                        + np.ascontiguousarray(psd, dtype=np.float64).tobytes() + omega.tobytes())
        out = subprocess.run([str(exe)], input=b"".join(blob), capture_output=True, check=True).stdout.decode()
        lines = out.splitlines()
        F = len(omega)
        assert len(lines) == len(systems) * F
        res = []
        for k, (G, _, st, _) in enumerate(systems):
            n, S = G.shape[0], len(st["src_a"])
            r = dict(per_f=[], onoise=np.zeros(F), gain=np.zeros(F, dtype=complex), contrib=np.zeros((F, S)),
                     y=np.zeros((F, n), dtype=complex))
            for f in range(F):
                tok = lines[k * F + f].split()
                v = np.array([float.fromhex(t) for t in tok[1:]])
                r["per_f"].append(int(tok[0]))
                r["onoise"][f] = v[0]
                r["gain"][f] = complex(v[1], v[2])
                r["contrib"][f] = v[3:3 + S]
                r["y"][f].real, r["y"][f].imag = v[3 + S::2], v[4 + S::2]
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


def test_host_noise_solve_equals_reference_bitwise(host_noise):
    """ac_noise_solve() against tests/noise_reference.py on the systems of tests/ac_cases.py, transposed so that the
    factored matrix carries each kind's feature (noise_reference.adjoint_case; every n from 1 to 63, every kind, OMEGA) with seeded generator tables of 0 .. 3n generators (ground terminals and a == b among them):
    flags, onoise, contrib, gain and y equal bit for bit (equal NaN masks where the inputs carry a NaN)."""
    seen_S, n_solves, n_failed = set(), 0, 0
    cov = cs.Coverage()
    for n in cs.SIZES:
        cases = [nref.adjoint_case(c) for c in cs.all_cases(sizes=(n,))]
        setups = [nref.setup(cs.KINDS.index(c["kind"]), n) for c in cases]
        host = host_noise([(c["G"][s], c["C"][s], st, st["psd"][s]) for c, st in zip(cases, setups)
                           for s in range(cs.NSYS)], cs.OMEGA)
        for ci, (c, st) in enumerate(zip(cases, setups)):
            S = len(st["src_a"])
            seen_S.add("none" if S == 0 else ("3n" if S == 3 * n else "between"))
            for s in range(cs.NSYS):
                h = host[ci * cs.NSYS + s]
                r = nref.solve_sweep(c["G"][s], c["C"][s], cs.OMEGA, st["out"], st["src_a"], st["src_b"], st["psd"][s],
                                     st["gain_in"])
                where = (c["kind"], n, s)
                assert h["per_f"] == r["per_f"], where
                cov.add(n, r["logs"])
                nan = c["kind"] in cs.HAS_NAN
                for key in ("onoise", "contrib", "gain", "y"):
                    _same(h[key], r[key], nan, where + (key,))
                for f, fl in enumerate(r["per_f"]):
                    n_solves += 1
                    if fl:
                        n_failed += 1
                        for key in ("onoise", "contrib", "gain", "y"):
                            v = np.ascontiguousarray(h[key][f]).view(np.float64)
                            assert np.all(v == 0) and not np.signbit(v).any(), where + (key, f)
    assert seen_S == {"none", "between", "3n"}
    cov.check()
    print("ac_noise_solve() == reference on %d solves, %d of them failed factorisations" % (n_solves, n_failed))
    assert n_failed > 0


# ---- accuracy of the definition
def _inverse_longdouble(A):
    """A^-1 by Gauss-Jordan elimination with partial pivoting, every operation in numpy.clongdouble"""
    n = A.shape[0]
    M = np.zeros((n, 2 * n), dtype=np.clongdouble)
    M[:, :n] = A
    M[:, n:] = np.eye(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        rows = np.arange(n) != k
        M[rows] = M[rows] - M[rows, k][:, None] * M[k][None, :]
    return M[:, n:]


ACCURACY_KINDS = ("dense", "mna", "reversed", "shift_up", "shift_down")      # dense, MNA-like and the dominant ones
ACCURACY_SEED = 20250117


def _accuracy_setup(kind, n):
    """noise_reference.setup() with the gain input a current into the output node, so that the gain is the
    driving-point impedance of the output, and for an MNA-like system the output at one of the nodes n // 4 ..
    n - n // 4 - 1 of ac_cases._mna, which no source ties to ground.

    The bound is normwise: it speaks for the components of y that are of the size of its norm.  A seeded pair of
    equations may land on a node that a source pins, or on two parts that sources isolate from each other (a
    transfer that is zero but for gmin and rounding), or on an off-diagonal entry of the inverse of a dominant
    matrix, 1e-6 of the diagonal ones: none of these has a relative accuracy under a normwise bound."""
    st = nref.setup(cs.KINDS.index(kind), n, seed=ACCURACY_SEED)
    if kind == "mna":
        rng = np.random.default_rng([ACCURACY_SEED, n])
        nb = n // 4
        st["out"] = (nb + int(rng.integers(0, n - 2 * nb)), -1)
    st["gain_in"] = ("i", st["out"][0], -1)
    return st


def test_definition_against_longdouble():
    """The float64 reference's onoise and gain against d^T A^-1 evaluated in numpy.longdouble from an explicit inverse
    of A (no transposition): relative deviation within 8 n 2^-52 cond_inf(A(w)), the forward-error bound of a
    backward-stable solve, cond computed here for every system and frequency.  The same bound for the adjoint
    identity: the gain read off y against d^T x of the forward solve (ac_reference.solve_sweep) with the unit
    excitation of the input."""
    worst = {"onoise": (0.0, None), "gain": (0.0, None), "adjoint": (0.0, None)}
    n_checked = 0
    for n in cs.SIZES:
        for kind in ACCURACY_KINDS:
            c = cs.case(kind, n)
            st = _accuracy_setup(kind, n)
            out_p, out_m = st["out"]
            gin = st["gain_in"]
            J = np.zeros(n, dtype=complex)                       # the unit excitation whose response the gain is
            if gin[0] == "v":
                J[gin[1]] = 1.0
            else:
                if gin[1] >= 0:
                    J[gin[1]] += 1.0
                if gin[2] >= 0:
                    J[gin[2]] -= 1.0
            for s in range(cs.NSYS):
                r = nref.solve_sweep(c["G"][s], c["C"][s], cs.OMEGA, st["out"], st["src_a"], st["src_b"], st["psd"][s], gin)
                assert r["per_f"] == [0, 0, 0], (kind, n, s)
                _, xf, _, _ = ac_reference.solve_sweep(c["G"][s], c["C"][s], J, cs.OMEGA)
                for f, w in enumerate(cs.OMEGA):
                    A = np.empty((n, n), dtype=np.clongdouble)
                    A.real, A.imag = c["G"][s], np.float64(w) * c["C"][s]
                    Ainv = _inverse_longdouble(A)
                    cond = float(np.max(np.sum(np.abs(A), axis=1)) * np.max(np.sum(np.abs(Ainv), axis=1)))
                    bound = 8.0 * n * 2.0 ** -52 * cond
                    t = Ainv[out_p] - (Ainv[out_m] if out_m >= 0 else 0)      # d^T A^-1
                    tz = np.concatenate([t, np.zeros(1, dtype=np.clongdouble)])   # index -1: ground
                    z = tz[st["src_a"]] - tz[st["src_b"]]
                    on = np.sum((z.real * z.real + z.imag * z.imag) * st["psd"][s].astype(np.longdouble))
                    g = tz[gin[1]] if gin[0] == "v" else tz[gin[1]] - tz[gin[2]]
                    dTx = xf[f][out_p] - (xf[f][out_m] if out_m >= 0 else 0.0)
                    where = (kind, n, s, f)
                    for key, got, want in (("onoise", np.longdouble(r["onoise"][f]), on),
                                           ("gain", np.clongdouble(r["gain"][f]), g),
                                           ("adjoint", np.clongdouble(r["gain"][f]), np.clongdouble(dTx))):
                        err, ref_abs = float(np.abs(got - want)), float(np.abs(want))
                        rel = err / (bound * ref_abs) if ref_abs > 0 else (0.0 if err == 0 else np.inf)
                        if rel > worst[key][0]:
                            worst[key] = (rel, where)
                        assert err <= bound * ref_abs, (key, where, err, bound * ref_abs, cond)
                    n_checked += 1
    print("definition against longdouble on %d (system, frequency) pairs; largest deviation as a fraction of the bound: "
          "onoise %.3g at %s, gain %.3g at %s, adjoint identity %.3g at %s"
          % (n_checked, *worst["onoise"], *worst["gain"], *worst["adjoint"]))


# ---- register budget
def test_packed_noise_kernel_registers(tmp_path):
    """Tripwire: the register-resident noise kernel keeps its matrix in registers -- no scratch, no spills, at any
    size (NP = 32 is the one at risk)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "noise.s"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + ENGINE_DIR, "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "api"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ENGINE_DIR, "kernels_noise.hip"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    meta, name = {}, None
    for line in asm.read_text().splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", line)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    packed = {k: v for k, v in meta.items() if "ac_noise_packed_kernel" in k}
    assert len(packed) == 4, sorted(meta)
    assert any("ILi32E" in k for k in packed)
    for k, v in packed.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
    wave = [v for k, v in meta.items() if "ac_noise_wave_kernel" in k]
    assert wave and wave[0]["private_segment_fixed_size"] == 0 and wave[0]["vgpr_spill_count"] == 0
    print("ac_noise_packed_kernel VGPRs:", {k[-30:]: v["vgpr_count"] for k, v in packed.items()})
