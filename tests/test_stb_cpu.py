"""Loop-gain analysis without a GPU: tests/stb_reference.py (include/csim.h "Loop-gain analysis" restated in numpy)
against what a loop gain is (the determinant identity 1 + T = det A / det A|gm=0, the closed forms of three equal
poles), the meaning of the probe's orientation, the host-compiled ac_stb.hpp against the reference on every input of
the GPU kernel tests, the golden loops' crossings, the argument refusals of csim_stb_solve_batch, and the register
budget of the kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stb_cases as sc
import stb_reference as sref
from circuitsimulator_amd import capi
from conftest import ROOT, has_gpu, netlist_path

ENGINE_DIR = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")

# Relative bound on |(1 + T) det A0 - det A| / |det A|, both determinants by numpy's LU in complex128.  Measured on the
# CPU over the three chain instances x 41 frequencies and 200 random unilateral loops: largest 5.3e-15; the bound is
# ten times that.
DET_BOUND = 5.3e-14


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. the reference against what a loop gain is ------------------------------------------------------------------

def _det_identity_error(G, C, w, probe, loop_entry):
    """|(1 + T) det A|gm=0 - det A| / |det A| with the loop opened by zeroing the transconductor at loop_entry"""
    fl, T, _, _ = sref.solve(G, C, w, probe)
    assert fl == 0
    A = G + 1j * w * C
    A0 = A.copy()
    A0[loop_entry] = 0.0
    dA, dA0 = np.linalg.det(A), np.linalg.det(A0)
    return abs((1.0 + T) * dA0 - dA) / abs(dA)


def test_reference_satisfies_the_determinant_identity_on_unilateral_loops():
    """1 + T = det A / det A|gm=0: the return difference of the loop's one transconductor.  Measured largest relative
    error 5.3e-15 (see DET_BOUND)."""
    worst = 0.0
    c, omega, _ = sc.inputs("chain")
    for b in range(len(c["G"])):
        for w in omega:
            worst = max(worst, _det_identity_error(c["G"][b], c["C"][b], w, c["probe"], (0, 3)))
    rng = np.random.default_rng(20261019)
    for _ in range(200):                                      # rows x, y, k: Yb and the current gm vy on x, Ya on y
        ya, yb, gm, ca, cb = rng.uniform(0.1, 2.0, 5)
        G = np.array([[yb, gm, 1.0], [0.0, ya, -1.0], [1.0, -1.0, 0.0]])
        C = np.diag([cb, ca, 0.0])
        w = rng.uniform(0.0, 3.0)
        worst = max(worst, _det_identity_error(G, C, w, (0, 1, 2), (0, 1)))
        _, T, _, _ = sref.solve(G, C, w, (0, 1, 2))
        want = gm / (ya + yb + 1j * w * (ca + cb))            # the unilateral loop: gm / (Ya + Yb)
        assert abs(T - want) <= 1e-13 * abs(want)
    print("determinant identity: largest relative error %.3e" % worst)
    assert worst <= DET_BOUND


# The interpolation error of the margins against the closed forms of A0 / (1 + s / p)^3, measured on the CPU at 10, 40
# and 160 points per decade, largest over the three instances:
#    10: PM 0.56 degrees,    fc 5.9e-3 relative,  GM 0.12 dB,    f180 3.2e-3 relative
#    40: PM 0.028 degrees,   fc 2.7e-4 relative,  GM 8.0e-3 dB,  f180 2.1e-4 relative
#   160: PM 0.0020 degrees,  fc 3.6e-5 relative,  GM 2.9e-4 dB,  f180 7.3e-6 relative
# Linear interpolation of smooth curves: second order in the spacing, times u (1 - u) of where in its interval the
# crossing falls, so a fourfold density gains between 7 and 30 here, not exactly 16.  Bounds: ten times the largest
# at 10 per decade, scaled by (10 / density)^2; and every figure must fall at least fourfold per fourfold density.
CLOSED_FORM_BOUND_AT_10 = dict(pm=5.6, fc=5.9e-2, gm=1.2, f180=3.2e-2)


def _closed_form_errors(per_decade):
    f = sc.chain_freqs(per_decade)
    c = sc.chain()
    err = dict(pm=0.0, fc=0.0, gm=0.0, f180=0.0)
    for b, gain in enumerate(sc.CHAIN_GAIN):
        r = sref.solve_sweep(c["G"][b], c["C"][b], 2.0 * np.pi * f, c["probe"])
        assert r["flags"] == 0
        # positive real at low frequency: at p / 100 the three poles have turned it by 0.03 rad
        assert abs(r["t"][0] - gain ** 3) < 0.04 * gain ** 3 and r["t"][0].real > 0
        m, found = sref.margins(f, r["t"])
        assert found == 3
        pm, fc, gm, f180 = sc.chain_closed_form(gain)
        assert f[0] < fc < f[-1] and f[0] < f180 < f[-1] and pm > 0 and gm > 0
        err["pm"] = max(err["pm"], abs(m[0] - pm))
        err["fc"] = max(err["fc"], abs(m[1] - fc) / fc)
        err["gm"] = max(err["gm"], abs(m[2] - gm))
        err["f180"] = max(err["f180"], abs(m[3] - f180) / f180)
    return err


def test_reference_margins_against_three_equal_poles():
    """f180 = sqrt(3) p / 2 pi, GM = 20 log10(8 / A0), PM from (1 + u^2)^(3/2) = A0: the reference's margins are these up
    to the interpolation error of the grid, which falls with its density (figures above)."""
    errs = {d: _closed_form_errors(d) for d in (10, 40, 160)}
    for d, e in errs.items():
        print("%3d points per decade: PM %.3e deg, fc %.3e, GM %.3e dB, f180 %.3e" % (d, e["pm"], e["fc"], e["gm"], e["f180"]))
        for k, bound in CLOSED_FORM_BOUND_AT_10.items():
            assert e[k] <= bound * (10.0 / d) ** 2, (d, k, e[k])
    for k in CLOSED_FORM_BOUND_AT_10:
        assert errs[160][k] < errs[40][k] / 4 and errs[40][k] < errs[10][k] / 4, k


def test_reversing_the_probe_changes_t_on_a_bilateral_loop():
    """with a conductance from the receiving node back into the chain the loop transmits both ways: T at the reversed
    probe (+ and - exchanged, the branch current negated) is another number, so the orientation is part of the
    definition; on the unilateral chain the reversed probe is simply wrong (1 / T-like), which is why + must drive"""
    c = sc.chain(reverse=2e-4)
    G, C = c["G"][0], c["C"][0]
    Gr = G.copy()
    Gr[:, 4] = -Gr[:, 4]
    Gr[4, :] = -Gr[4, :]
    w = 0.5 * sc.CHAIN_G / sc.CHAIN_C
    _, T, _, _ = sref.solve(G, C, w, (2, 3, 4))
    _, Tr, _, _ = sref.solve(Gr, C, w, (3, 2, 4))
    _, Tu, _, _ = sref.solve(sc.chain()["G"][0], C, w, (2, 3, 4))
    print("T %s, reversed %s, unilateral %s" % (T, Tr, Tu))
    assert abs(T - Tr) > 0.05 * abs(T)
    assert abs(T - Tu) > 0.01 * abs(Tu)                       # the reverse path does change the loop


@pytest.mark.parametrize("name", ["stb_cs_loop.sp", "stb_cs_loop_p.sp"])
def test_golden_loops_have_both_crossings_inside_the_grid(name):
    """the reference on the nominal instance (operating point and G from the CPU oracle, C from the IR) finds the unity
    and the phase crossing strictly inside the card's grid, so no test of these netlists passes by finding nothing"""
    import stb_netlist_system as sn
    from circuitsimulator_amd import Netlist
    nl = Netlist.from_file(netlist_path(name))
    G, C, x = sn.nominal_system(nl)
    el, ep, em, eb = nl.stb[:4]
    assert (ep, em) == (nl.node_eq("d"), nl.node_eq("fb")) and eb == nl.n_unknowns - 1
    assert abs(x[nl.node_eq("g")] - x[nl.node_eq("d")]) < 0.02           # self-biased: the gate sits at the drain
    f = nl.stb_freqs()
    r = sref.solve_sweep(G, C, 2.0 * np.pi * f, (ep, em, eb))
    m, found = sref.margins(f, r["t"])
    print("%s: T(1 kHz) %s, PM %.2f deg at %.4g Hz, GM %.2f dB at %.4g Hz" % (name, r["t"][0], m[0], m[1], m[2], m[3]))
    assert r["flags"] == 0 and found == 3
    assert r["t"][0].real > 1.0 and abs(r["t"][0].imag) < 0.01 * r["t"][0].real     # negative feedback: positive real
    assert f[1] < m[1] < f[-2] and f[1] < m[3] < f[-2] and m[1] < m[3]
    assert 0 < m[0] < 90 and m[2] > 0


# ---- 2. the host-compiled ac_stb.hpp against the reference --------------------------------------------------------

# binary records on stdin -- int32 n, F, x, y, k; G [n][n], C [n][n] row-major; omega [F]; freqs [F]; one line per
# frequency: flags, T, X0, X1 (re im pairs) as %a; then one line: PM, fc, GM, f180 as %a and found
HOST_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ac_stb.hpp"
int main()
{
    int32_t hd[5];
    while (std::fread(hd, sizeof(int32_t), 5, stdin) == 5) {
        const int n = hd[0], F = hd[1], ld = n + 2;
        std::vector<double> G((size_t)n * n), C((size_t)n * n), om(F), fr(F), ar((size_t)n * ld), ai((size_t)n * ld), xr(2 * n),
            xi(2 * n), T(2 * (size_t)F);
        if (std::fread(G.data(), sizeof(double), G.size(), stdin) != G.size()) return 1;
        if (std::fread(C.data(), sizeof(double), C.size(), stdin) != C.size()) return 1;
        if (std::fread(om.data(), sizeof(double), om.size(), stdin) != om.size()) return 1;
        if (std::fread(fr.data(), sizeof(double), fr.size(), stdin) != fr.size()) return 1;
        for (int f = 0; f < F; ++f) {
            const unsigned fl = csim::ac_stb_solve(n, G.data(), C.data(), om[f], hd[2], hd[3], hd[4], 1e-15, ld, ar.data(),
                                                   ai.data(), xr.data(), xi.data(), &T[2 * (size_t)f]);
            std::printf("%u %a %a", fl, T[2 * (size_t)f], T[2 * (size_t)f + 1]);
            for (int i = 0; i < 2 * n; ++i) std::printf(" %a %a", xr[i], xi[i]);
            std::printf("\n");
        }
        const csim::StbMargins m = csim::stb_margins(F, fr.data(), T.data(), 1);
        std::printf("%a %a %a %a %d\n", m.pm, m.fc, m.gm, m.f180, m.found);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_sweep(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("stb")
    cpp, exe = d / "drv.cpp", d / "drv"
    cpp.write_text(HOST_DRIVER)
    p = subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-w", "-I" + ENGINE_DIR,
                        "-I" + os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def sweep(c, omega, fhz):
        """-> per system (flags [F], t complex [F], x complex [F][2][n], margins [4], found), values as printed (%a)"""
        n, F = c["n"], len(omega)
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
        i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).tobytes()       # noqa: E731
        blob = b"".join(i4([n, F] + list(c["probe"])) + f8(c["G"][b]) + f8(c["C"][b]) + f8(omega) + f8(fhz)
                        for b in range(len(c["G"])))
        lines = subprocess.run([str(exe)], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
        assert len(lines) == len(c["G"]) * (F + 1)
        res = []
        for b in range(len(c["G"])):
            fl, t, x = [], np.zeros(F, dtype=complex), np.zeros((F, 2, n), dtype=complex)
            for f in range(F):
                tok = lines[b * (F + 1) + f].split()
                v = np.array([float.fromhex(s) for s in tok[1:]])
                fl.append(int(tok[0]))
                t.real[f], t.imag[f] = v[0], v[1]
                x[f].real, x[f].imag = v[2::2].reshape(2, n), v[3::2].reshape(2, n)
            tok = lines[b * (F + 1) + F].split()
            res.append((fl, t, x, np.array([float.fromhex(s) for s in tok[:4]]), int(tok[4])))
        return res
    return sweep


KEYS = list(sc.SIZES) + ["chain", "tank", "zero_den"]


@pytest.mark.parametrize("key", KEYS, ids=[str(k) for k in KEYS])
def test_reference_equals_host_compiled_header(host_sweep, key):
    c, omega, fhz = sc.inputs(key)
    ref = sc.reference(key)
    worst = 0.0
    for b, (fl, t, x, m, found) in enumerate(host_sweep(c, omega, fhz)):
        assert fl == ref[b]["per_f"], (key, b)
        assert not np.isnan(ref[b]["x"].view(np.float64)).any()
        assert np.array_equal(_bits(t), _bits(ref[b]["t"])), (key, b)
        assert np.array_equal(_bits(x), _bits(ref[b]["x"])), (key, b)
        assert found == ref[b]["found"], (key, b)
        worst = max(worst, sc.margins_close(m, ref[b]["margins"]))
        if isinstance(key, int):
            assert ref[b]["flags"] == 0 and np.all(ref[b]["t"] != 0)
    print("%s: margins of the host-compiled header against numpy: largest deviation %.3e" % (key, worst))
    if isinstance(key, int):
        assert len(set(c["probe"])) == 3 and any(log.swaps > 0 for r in ref for logs in r["logs"] for log in logs)
    if key == "chain":
        assert all(r["found"] == 3 for r in ref)


def test_singular_and_zero_den_cases_zero_t_and_flag_it(host_sweep):
    """the LC tank fails its pivot test at w == 1.0 alone; the resistive loop has den == 0.0 at every frequency while
    its factorisation succeeds: T is +0.0 + 0.0j and the flag is set in both, and the margins' walk ends there"""
    ref, = sc.reference("tank")
    assert [bool(f) for f in ref["per_f"]] == list(sc.TANK_FAILS) and ref["flags"] == 4
    for f, fails in enumerate(sc.TANK_FAILS):
        v = ref["t"][f:f + 1].view(np.float64)
        assert (np.all(v == 0) and not np.signbit(v).any() and np.all(ref["x"][f] == 0)) if fails else ref["t"][f] != 0
    assert ref["found"] == 0 and np.isnan(ref["margins"]).all()
    ref, = sc.reference("zero_den")
    assert ref["per_f"] == [4] * len(sc.OMEGA)
    v = ref["t"].view(np.float64)
    assert np.all(v == 0) and not np.signbit(v).any()
    assert np.all(ref["x"][:, 0, :2] == [1.5, 0.5]) and np.all(ref["x"][:, 1, 2] == 0.5)     # solved, and exactly so
    assert all(log.failed_at < 0 for logs in ref["logs"] for log in logs)
    # the walk ends at the first zero: a crossing before it stays, one after it is not looked for
    f = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    m, found = sref.margins(f, np.array([2.0, 0.5, 0.0, -2.0, -0.5]))
    assert found == 1 and 1.0 < m[1] < 2.0 and abs(m[0] - 180.0) < 1e-12 and np.isnan(m[2:]).all()
    m, found = sref.margins(f, np.array([2.0, np.inf, 0.5, 0.25, 0.125]))
    assert found == 0 and np.isnan(m).all()


# ---- 3. refusals without a GPU --------------------------------------------------------------------------------------

ORDER = "device n B G Cm eq_p eq_m eq_br omega F kernel T x flags freqs_hz margins found".split()


def _call(**change):
    a = dict(device=0, n=3, B=1, G=np.eye(3)[None].copy(), Cm=np.zeros((1, 3, 3)), eq_p=0, eq_m=1, eq_br=2, omega=np.ones(2),
             F=2, kernel=0, T=np.zeros((1, 2, 2)), x=np.zeros((1, 2, 2, 3, 2)), flags=np.zeros(1, dtype=np.uint32),
             freqs_hz=np.array([1.0, 2.0]), margins=np.zeros((1, 4)), found=np.zeros(1, dtype=np.int32))
    for k, v in change.items():
        assert k in a, k
        a[k] = np.asarray(v, dtype=a[k].dtype) if isinstance(a[k], np.ndarray) and v is not None else v
    keep = [v for v in a.values() if isinstance(v, np.ndarray)]
    rc = capi.lib().csim_stb_solve_batch(*[a[k].ctypes.data if isinstance(a[k], np.ndarray) else a[k] for k in ORDER])
    del keep
    return rc


ARG_CASES = [dict(n=-1), dict(B=-1), dict(F=-1), dict(kernel=3), dict(kernel=5), dict(kernel=-1),
             dict(G=None), dict(Cm=None), dict(omega=None), dict(T=None), dict(freqs_hz=None), dict(margins=None),
             dict(eq_p=3), dict(eq_p=-1), dict(eq_m=3), dict(eq_m=-1), dict(eq_br=3), dict(eq_br=-1),
             dict(eq_p=1), dict(eq_br=0), dict(eq_m=2),
             dict(freqs_hz=[0.0, 1.0]), dict(freqs_hz=[2.0, 2.0]), dict(freqs_hz=[2.0, 1.0]), dict(freqs_hz=[-1.0, 1.0]),
             dict(freqs_hz=[1.0, np.nan]), dict(freqs_hz=[1.0, np.inf]),
             dict(kernel=3, n=64)]


@pytest.mark.parametrize("change", ARG_CASES, ids=lambda c: "-".join("%s=%s" % (k, "null" if v is None else v) for k, v in c.items()))
def test_refused_at_the_argument_stage(change):
    assert _call(**change) == capi.CSIM_ERR_ARG, capi.lib().csim_last_error()


def test_empty_calls_and_calls_without_margins_pass_the_argument_stage():
    after = capi.CSIM_OK if has_gpu() else capi.CSIM_ERR_NO_DEVICE
    nulls = dict(G=None, Cm=None, omega=None, T=None, freqs_hz=None)
    assert _call(F=0, **nulls) == after and _call(B=0, **nulls) == after
    assert _call(x=None, flags=None, freqs_hz=None, margins=None, found=None) == after
    assert _call(found=None) == after
    assert _call(freqs_hz=[0.0, 0.0], margins=None, found=None) == after         # without margins the grid is not looked at


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_need_a_device():
    """the device check comes after the argument checks and before the refusal of the block kernel and of the sizes"""
    assert _call() == capi.CSIM_ERR_NO_DEVICE
    assert _call(kernel=4) == capi.CSIM_ERR_NO_DEVICE
    for n, kernel in ((64, 0), (33, 2)):
        assert _call(n=n, kernel=kernel, G=np.eye(n)[None], Cm=np.zeros((1, n, n)),
                     x=np.zeros((1, 2, 2, n, 2))) == capi.CSIM_ERR_NO_DEVICE


# ---- 4. registers ---------------------------------------------------------------------------------------------------

def test_stb_kernel_registers(tmp_path):
    """Tripwire: no kernel of kernels_stb.hip uses scratch or spills a vector register, at any packed size (NP = 32 is
    the one at risk).  Scalar registers parked in lanes of a vector register (sgpr_spill_count; the unrolled columns of
    ac_sweep.hpp's acp_column do that in every packed sweep kernel) never reach memory and are only printed."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "stb.s"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + ENGINE_DIR, "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "api"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ENGINE_DIR, "kernels_stb.hip"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    meta, name = {}, None
    for line in asm.read_text().splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|agpr_count):\s+(\d+)", line)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    packed = {k: v for k, v in meta.items() if "stb_sweep_packed_kernel" in k}
    assert len(packed) == 4 and any("ILi32E" in k for k in packed), sorted(meta)
    assert len([k for k in meta if "stb_sweep_wave_kernel" in k]) == 1 and len([k for k in meta if "stb_margins_kernel" in k]) == 1
    assert len(meta) == 6, sorted(meta)
    for k, v in meta.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
    print("kernels_stb.hip VGPRs (+AGPRs, SGPRs held in VGPR lanes):",
          {k[-40:]: (v["vgpr_count"], v.get("agpr_count", 0), v["sgpr_spill_count"]) for k, v in meta.items()})
