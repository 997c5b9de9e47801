"""Distortion analysis without a GPU: tests/disto_reference.py (include/csim.h "Distortion analysis" restated in numpy)
against physics (a time-domain solve of a one-MOSFET stage), its coefficients against the current they expand, the
host-compiled ac_disto.hpp against it bit for bit on every input of the GPU kernel tests, the argument refusals of
csim_disto_solve_batch, and the register budget of the kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import disto_cases as dc
import disto_reference as dref
import disto_timedomain as td
from circuitsimulator_amd import capi
from conftest import ROOT, has_gpu

ENGINE_DIR = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")

# ---- 1. the reference against physics ---------------------------------------------------------------------------

VTH, K, LAM = 0.5, 1.8e-3, 0.05
AMP, PHYSICS_BOUND = td.AMP, td.PHYSICS_BOUND


def _stage_reference(isP, rd, rs, vg0, xop, amp=AMP):
    """the stage of tests/disto_timedomain.py through disto_reference: unknowns (vd, vg, vs, i of the gate source)"""
    vd0, vs0 = xop
    _, gg, gd = dref.mos_current(isP, VTH, K, LAM, vd0, vg0, vs0)
    G = np.zeros((4, 4))
    G[0, 0] += 1.0 / rd
    G[2, 2] += 1.0 / rs
    for row, sign in ((0, 1.0), (2, -1.0)):                   # the drain current leaves d and enters s
        G[row, 0] += sign * gd
        G[row, 1] += sign * gg
        G[row, 2] -= sign * (gd + gg)
    G[1, 3] = G[3, 1] = 1.0
    J = np.array([0, 0, 0, amp], dtype=complex)
    c = dref.coef(isP, VTH, K, LAM, vd0, vg0, vs0)
    fl, _, x, hd, _ = dref.solve(G, np.zeros((4, 4)), J, 1.0, [0], [1], [2], c[None], (0, -1))
    assert fl == 0
    return x[:, [0, 2]], hd


STAGES = {                                                    # isP, VDD, RD, RS, VG
    "nmos-sat": (False, 3.0, 2e3, 200.0, 1.2),
    "nmos-triode": (False, 3.0, 20e3, 200.0, 1.5),
    "pmos-sat": (True, -3.0, 2e3, 200.0, -1.2),
    "pmos-triode": (True, -3.0, 20e3, 200.0, -1.5),
}


@pytest.mark.parametrize("name", list(STAGES))
def test_reference_against_time_domain(name):
    """x1, x2, x3 of the reference equal the first three harmonics of the statically stepped stage at 1 mV.  The two
    differ by the next term of the series, O((a / Vov)^2) relative.  Measured largest relative disagreement over the
    three orders and the two nodes: nmos-sat 1.41e-7, nmos-triode 1.99e-6, pmos-sat 1.41e-7, pmos-triode 1.99e-6 (the
    third order in triode, where a / Vov is largest); the bound is ten times the largest."""
    isP, vdd, rd, rs, vg0 = STAGES[name]
    vd0, vs0, _ = td.dc_point(isP, VTH, K, LAM, vdd, rd, rs, vg0)
    xop = (float(vd0), float(vs0))
    ph, region = td.harmonics(isP, VTH, K, LAM, rd, rs, (xop[0], vg0, xop[1]))
    assert region == ("sat" if "sat" in name else "triode")
    x, hd = _stage_reference(isP, rd, rs, vg0, xop)
    rel = np.abs(x - ph) / np.abs(ph)
    print("%s: x_op %s, |x1| %s, |x2| %s, |x3| %s, relative disagreement per order %s, HD2 %.3e HD3 %.3e"
          % (name, xop, np.abs(ph[0]), np.abs(ph[1]), np.abs(ph[2]), rel.max(axis=1), hd[0], hd[1]))
    assert np.all(np.abs(ph[1]) > 0) and np.all(np.abs(ph[2]) > 0)
    assert rel.max() < PHYSICS_BOUND, rel
    assert np.isclose(hd[0], abs(ph[1, 0]) / abs(ph[0, 0]), rtol=PHYSICS_BOUND)
    assert np.isclose(hd[1], abs(ph[2, 0]) / abs(ph[0, 0]), rtol=PHYSICS_BOUND)


# ---- 2. the coefficients are the Taylor coefficients of the current -----------------------------------------------

@pytest.mark.parametrize("isP", [False, True], ids=["nmos", "pmos"])
@pytest.mark.parametrize("region", ["sat", "triode"])
def test_coefficients_are_exact_taylor_coefficients(isP, region):
    """Inside a region the current is a cubic in (Ug, Ud): the third-order Taylor sum from the first derivatives and the
    seven coefficients equals the current at the displaced point within 64 ulp of the sum of the absolute terms (fewer
    than 32 roundings in either evaluation).  Operating points keep Vov >= 0.2 Vgs, so the rounding of the terminal
    differences, amplified by Vgs / Vov, stays inside that margin."""
    rng = np.random.default_rng([20260119, int(isP), region == "sat"])
    p = -1.0 if isP else 1.0
    worst, n = 0.0, 0
    while n < 400:
        vth, k, lam = rng.uniform(0.3, 0.7), rng.uniform(1e-4, 1e-2), rng.uniform(0.0, 0.1)
        vs = rng.uniform(-0.5, 0.5)
        vgs, vds = rng.uniform(1.0, 3.0), rng.uniform(0.05, 3.0)
        dg, dd = rng.uniform(-0.2, 0.2, 2)
        here = dref.mos_region(isP, vth, k, lam, vs + p * vds, vs + p * vgs, vs)
        there = dref.mos_region(isP, vth, k, lam, vs + p * vds + dd, vs + p * vgs + dg, vs)
        if here[5] != region or there[5] != region or here[3] < 0.2 * vgs:
            continue
        n += 1
        vd, vg = np.float64(vs + p * vds), np.float64(vs + p * vgs)
        i0, gg, gd = dref.mos_current(isP, vth, k, lam, vd, vg, vs)
        c = dref.coef(isP, vth, k, lam, vd, vg, vs)
        ug, ud = (vg + dg) - vg, (vd + dd) - vd              # the displacement as the displaced point sees it
        terms = [i0, gg * ug, gd * ud, 0.5 * c[dref.GG] * ug * ug, c[dref.GD] * ug * ud, 0.5 * c[dref.DD] * ud * ud,
                 c[dref.GGG] / 6.0 * ug ** 3, 0.5 * c[dref.GGD] * ug * ug * ud, 0.5 * c[dref.GDD] * ug * ud * ud,
                 c[dref.DDD] / 6.0 * ud ** 3]
        want, _, _ = dref.mos_current(isP, vth, k, lam, vd + dd, vg + dg, vs)
        scale = np.sum(np.abs(terms))
        dev = abs(float(np.sum(terms)) - float(want)) / float(np.spacing(scale))
        worst = max(worst, dev)
        assert dev <= 64, (isP, region, vth, k, lam, vs, vgs, vds, dg, dd, dev)
    print("%s %s: %d points, largest deviation %.1f ulp of the sum of the absolute terms" % ("pmos" if isP else "nmos", region, n, worst))


def test_coefficients_off_and_clamped_are_zero():
    assert np.all(dref.coef(False, 0.5, 1e-3, 0.05, 1.0, 0.4, 0.0) == 0)          # Vgs <= Vth
    assert np.all(dref.coef(False, 0.5, 1e-3, 0.05, -0.1, 1.0, 0.0) == 0)         # Vds < 0
    assert np.all(dref.coef(True, 0.5, 1e-3, 0.05, -1.0, -0.4, 0.0) == 0)
    assert np.all(dref.coef(False, 0.5, 1e-3, -2.0, 1.0, 3.0, 0.0) == 0)          # factor = 1 - 2 < 0: clamped
    c = dref.coef(True, 0.5, 1e-3, 0.05, -2.0, -1.0, 0.0)                         # PMOS in saturation: p on second order
    assert c[dref.GG] < 0 and c[dref.GD] < 0 and c[dref.GGD] > 0 and np.signbit(c[dref.DD])


# ---- 3. the host-compiled ac_disto.hpp against the reference ------------------------------------------------------

# binary records on stdin -- int32 n, F, M, out_p, out_m; G [n][n], C [n][n] row-major; J re [n], J im [n]; omega [F];
# dev_d, dev_g, dev_s [M] int32; coef [M][7]; one line per frequency: flags, x1, x2, x3 (re im pairs), HD2, HD3 as %a
HOST_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ac_disto.hpp"
int main()
{
    int32_t hd[5];
    while (std::fread(hd, sizeof(int32_t), 5, stdin) == 5) {
        const int n = hd[0], F = hd[1], M = hd[2], ld = n + 1;
        std::vector<double> G((size_t)n * n), C((size_t)n * n), J(2 * n), om(F), coef((size_t)M * 7 + 1), ar((size_t)n * ld),
            ai((size_t)n * ld), xr(3 * n), xi(3 * n);
        std::vector<int32_t> dev(3 * (size_t)M + 1);
        if (std::fread(G.data(), sizeof(double), G.size(), stdin) != G.size()) return 1;
        if (std::fread(C.data(), sizeof(double), C.size(), stdin) != C.size()) return 1;
        if (std::fread(J.data(), sizeof(double), J.size(), stdin) != J.size()) return 1;
        if (std::fread(om.data(), sizeof(double), om.size(), stdin) != om.size()) return 1;
        if (std::fread(dev.data(), sizeof(int32_t), 3 * (size_t)M, stdin) != 3 * (size_t)M) return 1;
        if (std::fread(coef.data(), sizeof(double), (size_t)M * 7, stdin) != (size_t)M * 7) return 1;
        for (int f = 0; f < F; ++f) {
            double h2[2];
            const unsigned fl = csim::ac_disto_solve(n, G.data(), C.data(), J.data(), J.data() + n, om[f], M, dev.data(),
                                                     dev.data() + M, dev.data() + 2 * M, coef.data(), hd[3], hd[4], 1e-15, ld,
                                                     ar.data(), ai.data(), xr.data(), xi.data(), h2);
            std::printf("%u", fl);
            for (int i = 0; i < 3 * n; ++i) std::printf(" %a %a", xr[i], xi[i]);
            std::printf(" %a %a\n", h2[0], h2[1]);
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_sweep(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("disto")
    cpp, exe = d / "drv.cpp", d / "drv"
    cpp.write_text(HOST_DRIVER)
    p = subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-w", "-I" + ENGINE_DIR,
                        "-I" + os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def sweep(c, omega):
        """-> per system (flags [F], h complex [F][3][n], hd [F][2]), values exactly as printed (%a)"""
        n, M, F = c["n"], c["M"], len(omega)
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
        i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).tobytes()       # noqa: E731
        blob = b"".join(i4([n, F, M, c["out"][0], c["out"][1]]) + f8(c["G"][b]) + f8(c["C"][b]) + f8(c["J"][b].real)
                        + f8(c["J"][b].imag) + f8(omega) + i4(c["dev_d"]) + i4(c["dev_g"]) + i4(c["dev_s"])
                        + f8(c["coef"][b]) for b in range(len(c["G"])))
        lines = subprocess.run([str(exe)], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
        assert len(lines) == len(c["G"]) * F
        res = []
        for b in range(len(c["G"])):
            fl, h, hd = [], np.zeros((F, 3, n), dtype=complex), np.zeros((F, 2))
            for f in range(F):
                tok = lines[b * F + f].split()
                v = np.array([float.fromhex(t) for t in tok[1:]])
                fl.append(int(tok[0]))
                h[f].real, h[f].imag = v[0:6 * n:2].reshape(3, n), v[1:6 * n:2].reshape(3, n)
                hd[f] = v[6 * n:]
            res.append((fl, h, hd))
        return res
    return sweep


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("n,M", dc.CASES, ids=["n%d-M%d" % c for c in dc.CASES])
def test_reference_equals_host_compiled_header(host_sweep, n, M):
    c = dc.case(n, M)
    ref = dc.reference((n, M))
    for b, (fl, h, hd) in enumerate(host_sweep(c, dc.OMEGA)):
        assert fl == [p[0] | p[1] | p[2] for p in ref[b]["per_f"]] == [0] * len(dc.OMEGA), (n, M, b)
        assert not np.isnan(ref[b]["h"].view(np.float64)).any()
        assert np.array_equal(_bits(h), _bits(ref[b]["h"])), (n, M, b)
        assert np.array_equal(_bits(hd), _bits(ref[b]["hd"])), (n, M, b)
        if M:
            assert np.all(ref[b]["hd"] > 0)
        else:
            assert np.all(ref[b]["h"][:, 1:] == 0) and np.all(ref[b]["hd"] == 0)
    d, s = c["dev_d"], c["dev_s"]
    if M >= 3:
        assert d[1] == s[1] and c["dev_g"][2] == d[2] and s[0] == -1
    if M == 65:
        assert np.count_nonzero(d == 0) >= 30 and np.count_nonzero(s == 0) >= 8 and np.any(d[40:] == 0)


def test_tank_fails_once_at_every_order(host_sweep):
    """the LC tank is singular exactly where k w == 1: no order at w = 0.25, order 2 at 0.5, order 1 at 1.0, order 3 at
    1/3; regular at w = 0, with a row exchange.  The failed order and every higher one are +0.0, the flag is set."""
    c = dc.tank()
    ref, = dc.reference("tank")
    assert 3.0 * dc.TANK_OMEGA[3] == 1.0
    (fl, h, hd), = host_sweep(c, dc.TANK_OMEGA)
    assert np.array_equal(_bits(h), _bits(ref["h"])) and np.array_equal(_bits(hd), _bits(ref["hd"]))
    for f, first in enumerate(dc.TANK_FAILS_AT):
        per = ref["per_f"][f]
        assert [k + 1 for k in range(3) if per[k]][:1] == ([first] if first else []), (f, per)
        assert fl[f] == (4 if first else 0)
        for k in range(3):
            v = ref["h"][f, k].view(np.float64)
            if first and k + 1 >= first:
                assert np.all(v == 0) and not np.signbit(v).any(), (f, k)
            else:
                assert np.any(ref["h"][f, k] != 0), (f, k)
        want_hd = [0 if first and first <= 2 else 1, 0 if first else 1]
        assert [int(x > 0) for x in ref["hd"][f]] == want_hd and not np.signbit(ref["hd"][f]).any(), (f, ref["hd"][f])
    assert ref["logs"][4][0].swaps == 1 and ref["flags"] == 4


# ---- 5. refusals without a GPU ---------------------------------------------------------------------------------------

ORDER = "device n B G Cm J M dev_d dev_g dev_s coef out_p out_m omega F kernel h hd flags".split()


def _call(**change):
    i4 = lambda *v: np.array(v, dtype=np.int32)     # noqa: E731
    a = dict(device=0, n=2, B=1, G=np.eye(2)[None].copy(), Cm=np.zeros((1, 2, 2)), J=np.ones((1, 2, 2)), M=1, dev_d=i4(0),
             dev_g=i4(1), dev_s=i4(-1), coef=np.ones((1, 1, 7)), out_p=0, out_m=-1, omega=np.ones(1), F=1, kernel=0,
             h=np.zeros((1, 1, 3, 2, 2)), hd=np.zeros((1, 1, 2)), flags=np.zeros(1, dtype=np.uint32))
    for k, v in change.items():
        assert k in a, k
        a[k] = np.asarray(v, dtype=a[k].dtype) if isinstance(a[k], np.ndarray) and v is not None else v
    keep = [v for v in a.values() if isinstance(v, np.ndarray)]
    rc = capi.lib().csim_disto_solve_batch(*[a[k].ctypes.data if isinstance(a[k], np.ndarray) else a[k] for k in ORDER])
    del keep
    return rc


ARG_CASES = [dict(n=-1), dict(B=-1), dict(F=-1), dict(M=-1), dict(kernel=3), dict(kernel=5), dict(kernel=-1),
             dict(G=None), dict(Cm=None), dict(J=None), dict(omega=None), dict(hd=None), dict(dev_d=None), dict(dev_g=None),
             dict(dev_s=None), dict(coef=None),
             dict(out_p=2), dict(out_p=-1), dict(out_m=2), dict(out_m=-2), dict(out_p=1, out_m=1),
             dict(dev_d=[2]), dict(dev_g=[2]), dict(dev_s=[2]), dict(dev_d=[-2]), dict(dev_g=[-2]), dict(dev_s=[-2]),
             dict(kernel=3, n=64)]


@pytest.mark.parametrize("change", ARG_CASES, ids=lambda c: "-".join("%s=%s" % (k, "null" if v is None else v) for k, v in c.items()))
def test_refused_at_the_argument_stage(change):
    assert _call(**change) == capi.CSIM_ERR_ARG, capi.lib().csim_last_error()


def test_empty_calls_pass_the_argument_stage():
    after = capi.CSIM_OK if has_gpu() else capi.CSIM_ERR_NO_DEVICE
    nulls = dict(G=None, Cm=None, J=None, omega=None, hd=None)
    assert _call(F=0, **nulls) == after and _call(B=0, **nulls) == after
    assert _call(h=None, flags=None, M=0, dev_d=None, dev_g=None, dev_s=None, coef=None) == after


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_need_a_device():
    """the device check comes after the argument checks and before the refusal of the block kernel and of the sizes"""
    assert _call() == capi.CSIM_ERR_NO_DEVICE
    assert _call(kernel=4) == capi.CSIM_ERR_NO_DEVICE
    assert _call(n=64, G=np.eye(64)[None], Cm=np.zeros((1, 64, 64)), J=np.zeros((1, 64, 2)),
                 h=np.zeros((1, 1, 3, 64, 2))) == capi.CSIM_ERR_NO_DEVICE
    assert _call(n=33, kernel=2, G=np.eye(33)[None], Cm=np.zeros((1, 33, 33)), J=np.zeros((1, 33, 2)),
                 h=np.zeros((1, 1, 3, 33, 2))) == capi.CSIM_ERR_NO_DEVICE


# ---- 6. registers ---------------------------------------------------------------------------------------------------

def test_disto_kernel_registers(tmp_path):
    """Tripwire: no kernel of kernels_disto.hip uses scratch or spills, at any packed size (NP = 32 is the one at risk)"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "disto.s"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + ENGINE_DIR, "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "api"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ENGINE_DIR, "kernels_disto.hip"), "-o", str(asm)],
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
    packed = {k: v for k, v in meta.items() if "ac_disto_packed_kernel" in k}
    assert len(packed) == 4 and any("ILi32E" in k for k in packed), sorted(meta)
    assert len([k for k in meta if "ac_disto_wave_kernel" in k]) == 1 and len([k for k in meta if "disto_coef_kernel" in k]) == 1
    assert len(meta) == 6, sorted(meta)
    for k, v in meta.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
    print("kernels_disto.hip VGPRs (+AGPRs):", {k[-40:]: (v["vgpr_count"], v.get("agpr_count", 0)) for k, v in meta.items()})
