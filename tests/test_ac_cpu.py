"""AC small-signal analysis, GPU-free parts: the `AC mag [phase]` source syntax and the .AC card, the SPICE
frequency grid, the complex LU core of engine/ac_lu.hpp compiled for the host, and the register budget of the
register-resident AC kernel."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, netlist_path

ENGINE_DIR = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")


def _nl(text):
    from circuitsimulator_amd import Netlist
    return Netlist.from_text(text)


@pytest.mark.parametrize("line,mag,phase,dc", [
    ("V1 a 0 DC 0.9 AC 1", 1.0, 0.0, 0.9),
    ("V1 a 0 0.9 AC 1 90", 1.0, 90.0, 0.9),
    ("V1 a 0 AC 1", 1.0, 0.0, 0.0),
    ("V1 a 0 AC 2.5 -45", 2.5, -45.0, 0.0),
    ("V1 a 0 DC 0.5 AC 1m 30 SIN 0 0.1 1meg", 1e-3, 30.0, 0.5),
    ("V1 a 0 AC 1 SIN 0.9 1m 1meg 0", 1.0, 0.0, 0.0),
    ("V1 a 0 0.2 AC 1 PULSE 0 1 1n 1n 1n 5n 20n", 1.0, 0.0, 0.2),
    ("V1 a 0 AC 3 10 PWL 0 0 1n 1", 3.0, 10.0, 0.0),
    ("I1 a 0 DC 1m AC 1", 1.0, 0.0, 1e-3),
    ("I1 a 0 AC 0.5 180", 0.5, 180.0, 0.0),
    ("I1 a 0 2m AC 1 PULSE 0 1m 1n", 1.0, 0.0, 2e-3),
])
def test_ac_source_forms(line, mag, phase, dc):
    text = "* ac source\n%s\nR1 a 0 1k\n" % line
    nl = _nl(text)
    assert nl.n_elems == 2
    m, p = nl.ac_source(0)
    assert (m, p) == pytest.approx((mag, phase), rel=0, abs=0)
    assert nl.nominal_params[0] == dc
    assert nl.ac_source(1) == (0.0, 0.0)


def test_ac_source_waveform_kept():
    plain = _nl("* w\nV1 a 0 DC 0.5 SIN 0 0.1 1meg\nR1 a 0 1k\n")
    ac = _nl("* w\nV1 a 0 DC 0.5 AC 1 SIN 0 0.1 1meg\nR1 a 0 1k\n")
    assert ac.n_params == plain.n_params
    assert np.array_equal(ac.nominal_params, plain.nominal_params)


def test_ac_card_round_trip():
    from circuitsimulator_amd.engine import ac_freqs
    nl = _nl("* card\nV1 a 0 AC 1\nR1 a 0 1k\n.AC OCT 4 10 1k\n")
    assert nl.ac == ("oct", 4, 10.0, 1000.0)
    assert np.array_equal(nl.ac_freqs(), ac_freqs("oct", 4, 10.0, 1000.0))
    assert _nl("* none\nV1 a 0 AC 1\nR1 a 0 1k\n").ac is None
    assert _nl("* lin\nV1 a 0 AC 1\nR1 a 0 1k\n.ac lin 5 1meg 2meg\n").ac == ("lin", 5, 1e6, 2e6)


@pytest.mark.parametrize("name,src", [("buffer.sp", "Vin 101 0 SIN"), ("dbmixer.sp", "Vrf1+ 112 212 SIN")])
def test_shipped_netlists_unchanged_by_ac_token(name, src):
    """Adding `AC 1` to the input source changes neither P, nor the nominal parameters, the equation names or the
    CSV header: the AC values live beside the parameter vector."""
    from circuitsimulator_amd import Netlist
    text = open(netlist_path(name)).read()
    assert src in text
    ref = Netlist.from_text(text)
    ac = Netlist.from_text(text.replace(src, src.replace(" SIN", " AC 1 SIN"), 1))
    assert ac.n_params == ref.n_params
    assert np.array_equal(ac.nominal_params, ref.nominal_params)
    assert ac.eq_names == ref.eq_names
    assert ac.csv_header == ref.csv_header
    assert np.array_equal(ac.mc_kinds, ref.mc_kinds)
    mags = [ac.ac_source(e)[0] for e in range(ac.n_elems)]
    assert sorted(mags) == [0.0] * (ac.n_elems - 1) + [1.0]
    assert all(ref.ac_source(e) == (0.0, 0.0) for e in range(ref.n_elems))
    if name == "buffer.sp":
        assert ac.n_params == 36


# ---- frequency grid
def _grid(*a):
    from circuitsimulator_amd.engine import ac_freqs
    return ac_freqs(*a)


def test_grid_dec_oct_points():
    f = _grid("dec", 10, 1e3, 1e10)
    assert len(f) == 71
    assert f[0] == 1e3
    assert np.allclose(f, 1e3 * 10.0 ** (np.arange(71) / 10), rtol=1e-15, atol=0)
    assert [1e3 * math.pow(10.0, k / 10) for k in range(71)] == list(f)
    # fstop just past a grid point: the point below it is the last
    assert len(_grid("dec", 10, 1e3, 1e4 * 1.01)) == 11
    assert len(_grid("dec", 10, 1e3, 1e4 * 0.99)) == 10
    # OCT: 2^(k/n)
    g = _grid("oct", 3, 100.0, 800.0)
    assert len(g) == 10
    assert [100.0 * math.pow(2.0, k / 3) for k in range(10)] == list(g)
    assert list(_grid("dec", 1, 5.0, 5.0)) == [5.0]


def test_grid_lin():
    assert list(_grid("lin", 1, 7.0, 9.0)) == [7.0]
    f = _grid("lin", 5, 1e6, 2e6)
    assert list(f) == [1e6 + k * (2e6 - 1e6) / 4 for k in range(5)]
    assert f[-1] == 2e6
    assert list(_grid("lin", 3, 0.0, 10.0)) == [0.0, 5.0, 10.0]


@pytest.mark.parametrize("args", [("dec", 0, 1.0, 10.0), ("oct", -1, 1.0, 10.0), ("dec", 10, 0.0, 10.0),
                                  ("oct", 10, -1.0, 10.0), ("lin", 5, 10.0, 1.0), ("dec", 10, 10.0, 1.0),
                                  ("lin", 0, 1.0, 2.0)])
def test_grid_errors(args):
    from circuitsimulator_amd import capi
    sw = ("dec", "oct", "lin").index(args[0])
    assert capi.lib().csim_ac_num_freqs(sw, *args[1:]) == capi.CSIM_ERR_CONFIG
    with pytest.raises(capi.CsimError) as e:
        _grid(*args)
    assert e.value.code == capi.CSIM_ERR_CONFIG


# ---- the complex LU core, compiled for the host
HOST_DRIVER = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "ac_lu.hpp"
// "sweep": binary records on stdin -- int32 n, F; G [n][n], C [n][n] row-major; J re [n], J im [n]; omega [F] --
// solved at every omega as (G + j w C) x = J; one line of flags and %a values per frequency
static int sweep()
{
    int32_t hd[2];
    while (std::fread(hd, sizeof(int32_t), 2, stdin) == 2) {
        const int n = hd[0], F = hd[1], ld = n + 1;
        std::vector<double> G(n * n), C(n * n), J(2 * n), om(F), ar(n * ld), ai(n * ld), xr(n), xi(n);
        if (std::fread(G.data(), sizeof(double), G.size(), stdin) != G.size()) return 1;
        if (std::fread(C.data(), sizeof(double), C.size(), stdin) != C.size()) return 1;
        if (std::fread(J.data(), sizeof(double), J.size(), stdin) != J.size()) return 1;
        if (std::fread(om.data(), sizeof(double), om.size(), stdin) != om.size()) return 1;
        for (int f = 0; f < F; ++f) {
            for (int i = 0; i < n; ++i) {
                for (int j = 0; j < n; ++j) { ar[i * ld + j] = G[i * n + j]; ai[i * ld + j] = om[f] * C[i * n + j]; }
                ar[i * ld + n] = J[i];
                ai[i * ld + n] = J[n + i];
            }
            const unsigned fl = csim::ac_lu_solve(n, ld, ar.data(), ai.data(), 1e-15, xr.data(), xi.data());
            std::printf("%u", fl);
            for (int i = 0; i < n; ++i) std::printf(" %a %a", xr[i], xi[i]);
            std::printf("\n");
        }
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "sweep") return sweep();
    int n;
    while (std::scanf("%d", &n) == 1) {
        const int ld = n + 1;
        std::vector<double> ar(n * ld), ai(n * ld), xr(n), xi(n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= n; ++j) std::scanf("%lf %lf", &ar[i * ld + j], &ai[i * ld + j]);
        const unsigned fl = csim::ac_lu_solve(n, ld, ar.data(), ai.data(), 1e-15, xr.data(), xi.data());
        std::printf("%u", fl);
        for (int i = 0; i < n; ++i) std::printf(" %a %a", xr[i], xi[i]);
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_lu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("aclu")
    cpp, exe = d / "drv.cpp", d / "drv"
    cpp.write_text(HOST_DRIVER)
    p = subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-w", "-I" + ENGINE_DIR,
                        "-I" + os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def run(systems):
        """systems: list of (A complex [n][n], b complex [n]) -> list of (flags, x complex [n])"""
        lines = []
        for A, b in systems:
            n = len(b)
            aug = np.concatenate([A, b[:, None]], axis=1)
            lines.append("%d %s" % (n, " ".join("%r %r" % (float(z.real), float(z.imag)) for z in aug.reshape(-1))))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        res = []
        for ln in out.splitlines():
            tok = ln.split()
            v = np.array([float.fromhex(t) for t in tok[1:]])
            res.append((int(tok[0]), v[0::2] + 1j * v[1::2]))
        return res

    def sweep(systems, omega):
        """systems: list of (G [n][n], C [n][n], J complex [n]) -> per system (flags [F], x complex [F][n]),
        values exactly as printed (%a)"""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        blob = b"".join(np.array([len(J), len(omega)], dtype=np.int32).tobytes()
                        + np.ascontiguousarray(G, dtype=np.float64).tobytes()
                        + np.ascontiguousarray(Cm, dtype=np.float64).tobytes()
                        + np.ascontiguousarray(J.real).tobytes() + np.ascontiguousarray(J.imag).tobytes()
                        + omega.tobytes() for G, Cm, J in systems)
        out = subprocess.run([str(exe), "sweep"], input=blob, capture_output=True, check=True).stdout.decode()
        lines = out.splitlines()
        assert len(lines) == len(systems) * len(omega)
        res = []
        for s, (_, _, J) in enumerate(systems):
            fl, x = [], np.zeros((len(omega), len(J)), dtype=complex)
            for f in range(len(omega)):
                tok = lines[s * len(omega) + f].split()
                v = np.array([float.fromhex(t) for t in tok[1:]])
                fl.append(int(tok[0]))
                x[f].real, x[f].imag = v[0::2], v[1::2]
            res.append((fl, x))
        return res
    run.sweep = sweep
    return run


def test_host_lu_against_numpy(host_lu):
    rng = np.random.default_rng(7)
    systems = []
    for n in range(1, 64):
        A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) + n * np.eye(n)
        b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        systems.append((A, b))
    for (A, b), (fl, x) in zip(systems, host_lu(systems)):
        assert fl == 0
        ref = np.linalg.solve(A, b)
        assert np.max(np.abs(x - ref)) / np.max(np.abs(ref)) <= 1e-12, len(b)


def test_host_lu_pivoting_rules(host_lu):
    # ties: the first row with the largest |.|^2 wins (rows 1 and 2 tie in column 0; row 1 is taken)
    A = np.array([[0.5, 1, 0], [1j, 2, 1], [-1, 0, 3]], dtype=complex)
    b = np.array([1, 2, 3], dtype=complex)
    (fl, x), = host_lu([(A, b)])
    assert fl == 0 and np.allclose(x, np.linalg.solve(A, b), rtol=1e-13)
    # singular: zero vector + flag
    S = np.array([[1, 2], [2, 4]], dtype=complex)
    (fl, x), = host_lu([(S, np.array([1, 1], dtype=complex))])
    assert fl == 0x4 and np.all(x == 0)
    # zero-diagonal MNA pattern of a voltage source: V(a) = 1, R = 1k to ground, C = 1n
    w = 2 * math.pi * 1e6
    A = np.array([[1e-3 + 1e-6 + 1j * w * 1e-9, 1], [1, 0]], dtype=complex)
    (fl, x), = host_lu([(A, np.array([0, 1], dtype=complex))])
    assert fl == 0 and x[0] == 1 and abs(x[1] + (1e-3 + 1e-6 + 1j * w * 1e-9)) < 1e-18


def test_reference_equals_host_lu_on_kernel_inputs(host_lu):
    """tests/ac_reference.py (the specification restated in numpy) against ac_lu_solve() on every input of the GPU
    kernel tests (tests/ac_cases.py): flags equal, x equal bit for bit (NaN masks equal where NaNs are expected).

    And a condition on the inputs: on every solve that is neither flagged nor fed a NaN, the reference's normwise
    backward error, evaluated in numpy.longdouble, stays below 8 n 2^-53.  Random inputs sit near 0.3 n 2^-53;
    the bound leaves the structured inputs about 25 times that.  An input that misses it is to be replaced, the
    bound stays.  The structured kinds are also checked to do what they are named after."""
    import ac_cases as cs
    import ac_reference as ref
    cov = cs.Coverage()
    worst = (0.0, None)
    n_solves = n_swaps = 0
    for n in cs.SIZES:
        cases = list(cs.all_cases(sizes=(n,)))
        assert {c["kind"] for c in cases} >= set(cs.KINDS) - ({"tie_diag", "nan_below"} if n < 2 else set()) \
            - ({"tie_rows"} if n < 3 else set())
        host = host_lu.sweep([(c["G"][s], c["C"][s], c["J"][s]) for c in cases for s in range(cs.NSYS)], cs.OMEGA)
        for ci, c in enumerate(cases):
            kind = c["kind"]
            flags, x, per_f, logs = cs.reference(c)
            for s in range(cs.NSYS):
                hfl, hx = host[ci * cs.NSYS + s]
                where = (kind, n, s)
                assert hfl == per_f[s], where
                nan = np.isnan(x[s].view(np.float64))
                assert np.array_equal(nan, np.isnan(hx.view(np.float64))), where
                assert nan.any() == (kind in cs.HAS_NAN), where
                assert np.array_equal(np.where(nan, 0, x[s].view(np.uint64)), np.where(nan, 0, hx.view(np.uint64))), where
                cov.add(n, logs[s])
                n_swaps += sum(g.swaps for g in logs[s])
                # the kinds do what they say
                if kind in cs.SINGULAR:
                    assert per_f[s] == [4, 4, 4] and np.all(x[s] == 0), where
                    at = {"sing_first": 0, "sing_mid": n // 2, "sing_last": n - 1}.get(kind)
                    assert at is None or [g.failed_at for g in logs[s]] == [at] * 3, where
                elif kind in ("sing_dc_only", "thr_both"):
                    assert per_f[s] == [0, 4, 0] and int(flags[s]) == 4, where
                    assert np.all(x[s, 1] == 0) and np.all(x[s, 0] != 0) and np.all(x[s, 2] != 0), where
                else:
                    assert per_f[s] == [0, 0, 0], where
                if kind in ("tie_diag", "tie_rows"):
                    assert logs[s][0].ties >= 1, where
                if kind == "mna" and n >= 8:
                    assert np.mean(c["G"][s] == 0) >= 0.6 and np.mean(c["C"][s] == 0) >= 0.6, where
                    assert logs[s][0].skips > 0, where
                if kind in cs.HAS_NAN:
                    continue
                for f, w in enumerate(cs.OMEGA):
                    if per_f[s][f]:
                        continue
                    A = np.empty((n, n), dtype=complex)
                    A.real, A.imag = c["G"][s], w * c["C"][s]
                    be = ref.backward_error(A, x[s, f], c["J"][s]) / (n * 2.0 ** -53)
                    n_solves += 1
                    if be > worst[0]:
                        worst = (be, where + (f,))
                    assert be < 8.0, (be, where, f)
    print("reference == ac_lu_solve() on %d unflagged NaN-free solves, %d row swaps; worst backward error "
          "%.3f n 2^-53 at %s" % (n_solves, n_swaps, worst[0], worst[1]))
    print("coverage:", cov)
    cov.check()


def test_packed_ac_kernel_registers(tmp_path):
    """Tripwire: the register-resident AC kernel keeps its matrix in registers -- no scratch at any size."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "ac.s"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + ENGINE_DIR, "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "api"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ENGINE_DIR, "kernels_ac.hip"), "-o", str(asm)],
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
    packed = {k: v for k, v in meta.items() if "ac_sweep_packed_kernel" in k}
    assert len(packed) == 4, sorted(meta)
    for k, v in packed.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)
    wave = [v for k, v in meta.items() if "ac_sweep_wave_kernel" in k]
    assert wave and wave[0]["private_segment_fixed_size"] == 0
