"""Intermodulation analysis without a GPU: tests/imd_reference.py (include/csim.h "Intermodulation analysis" restated in
numpy) against physics (a static solve on the two-tone torus, and a Fourier collocation of the stage with capacitors),
against the single-tone reference where the two must agree, the host-compiled ac_imd.hpp against it bit for bit on
every input of the GPU kernel tests, the argument refusals of csim_imd_solve_batch, and the resources of the kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import disto_reference as dref
import disto_timedomain as td
import imd_cases as ic
import imd_reference as iref
import imd_timedomain as itd
from circuitsimulator_amd import capi
from conftest import ROOT, has_gpu

ENGINE_DIR = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")

# ---- 1, 2. the reference against physics --------------------------------------------------------------------------

VTH, K, LAM = 0.5, 1.8e-3, 0.05
CL, CGD, W0 = 1e-9, 2e-10, 2.0 * np.pi * 1e4                 # RD CL = 2 us (saturation), 20 us (triode); tones at 70 and 50 kHz

STAGES = {                                                    # isP, VDD, RD, RS, VG
    "nmos-sat": (False, 3.0, 2e3, 200.0, 1.2),
    "nmos-triode": (False, 3.0, 20e3, 200.0, 1.5),
    "pmos-sat": (True, -3.0, 2e3, 200.0, -1.2),
    "pmos-triode": (True, -3.0, 20e3, 200.0, -1.5),
}


def _stage_reference(isP, rd, rs, vg0, xop, cl, cgd, w1, w2, amp=td.AMP):
    """the stage of tests/imd_timedomain.py through imd_reference: unknowns (vd, vg, vs, i of the gate source)"""
    vd0, vs0 = xop
    _, gg, gd = dref.mos_current(isP, VTH, K, LAM, vd0, vg0, vs0)
    G, C = np.zeros((4, 4)), np.zeros((4, 4))
    G[0, 0] += 1.0 / rd
    G[2, 2] += 1.0 / rs
    for row, sign in ((0, 1.0), (2, -1.0)):                   # the drain current leaves d and enters s
        G[row, 0] += sign * gd
        G[row, 1] += sign * gg
        G[row, 2] -= sign * (gd + gg)
    G[1, 3] = G[3, 1] = 1.0
    C[0, 0] += cl + cgd
    C[1, 1] += cgd
    C[0, 1] -= cgd
    C[1, 0] -= cgd
    J = np.array([0, 0, 0, amp], dtype=complex)
    c = dref.coef(isP, VTH, K, LAM, vd0, vg0, vs0)
    fl, _, x, im = iref.solve(G, C, J, None, w1, w2, [0], [1], [2], c[None], (0, -1))
    assert fl == 0
    return x[:, [0, 2]], im


def _op(name):
    isP, vdd, rd, rs, vg0 = STAGES[name]
    vd0, vs0, _ = td.dc_point(isP, VTH, K, LAM, vdd, rd, rs, vg0)
    return isP, rd, rs, vg0, (float(vd0), float(vs0))


def _compare(name, what, x, im, ph, bound):
    rel = np.abs(x - ph) / np.abs(ph)
    print("%s %s: |bins| at d %s, relative disagreement per solve %s, IM2+ %.3e IM2- %.3e IM3 %.3e"
          % (name, what, np.abs(ph[:, 0]), rel.max(axis=1), im[0], im[1], im[2]))
    assert np.all(np.abs(ph) > 0)
    assert rel.max() < bound, rel
    for q, k in enumerate((2, 3, 5)):
        assert np.isclose(im[q], abs(ph[k, 0]) / abs(ph[0, 0]), rtol=bound)


@pytest.mark.parametrize("name", list(STAGES))
def test_reference_against_the_torus(name):
    """The six solutions of the reference equal the bins (1, 0), (0, 1), (1, 1), (1, -1), (2, 0), (2, -1) of the
    statically stepped stage on a 16 x 16 torus at 1 mV per tone.  The two differ by the next term of the series.
    Measured largest relative disagreement over the six solutions and the two nodes: nmos-sat 5.02e-7, nmos-triode
    6.62e-6, pmos-sat 5.02e-7, pmos-triode 6.62e-6; the bound (imd_timedomain.PHYSICS_BOUND) is ten times the largest."""
    isP, rd, rs, vg0, xop = _op(name)
    ph, region = itd.torus(isP, VTH, K, LAM, rd, rs, (xop[0], vg0, xop[1]))
    assert region == ("sat" if "sat" in name else "triode")
    x, im = _stage_reference(isP, rd, rs, vg0, xop, 0.0, 0.0, 3.0, 2.0)
    _compare(name, "torus", x, im, ph, itd.PHYSICS_BOUND)


@pytest.mark.parametrize("name", list(STAGES))
def test_reference_against_the_collocation_with_memory(name):
    """With CL from d to ground and CGD from g to d and tones at 7 f0 and 5 f0, the six solutions equal the bins 7, 5,
    12, 2, 14 and 9 of the periodic solution, phase included: this is what a wrong conjugate or a wrong frequency in
    the solves at w1 - w2 and 2 w1 - w2 would miss.  Measured largest relative disagreement: nmos-sat 3.88e-7,
    nmos-triode 3.69e-6, pmos-sat 3.88e-7, pmos-triode 3.69e-6; the bound (imd_timedomain.MEMORY_BOUND) is ten times the
    largest."""
    isP, rd, rs, vg0, xop = _op(name)
    ph, region = itd.collocation(isP, VTH, K, LAM, rd, rs, CL, CGD, W0, (xop[0], vg0, xop[1]))
    assert region == ("sat" if "sat" in name else "triode")
    x, im = _stage_reference(isP, rd, rs, vg0, xop, CL, CGD, itd.TONES[0] * W0, itd.TONES[1] * W0)
    # memory matters: the solutions are far from real multiples of each other's phase
    assert abs(np.sin(np.angle(ph[3, 0]) - np.angle(ph[2, 0]))) > 0.1
    _compare(name, "collocation", x, im, ph, itd.MEMORY_BOUND)


# ---- 3. against the single-tone reference ---------------------------------------------------------------------------

DISTO_CROSS_BOUND = 1.6e-14


@pytest.mark.parametrize("n,M", [(5, 3), (5, 65), (31, 3)])
def test_memoryless_equal_tones_are_multiples_of_the_harmonics(n, M):
    """C = 0, a real J and J2 = J1: every frequency sees the same real matrix, so x2 = x3 = 2 (second harmonic) and
    x5 = 3 (third harmonic) of tests/disto_reference.py, up to rounding (the two references group their factors
    differently).  Measured largest difference relative to the largest entry of the vector, over the three cases and
    their three systems: 5.0e-16 at (5, 3), 5.6e-16 at (5, 65), 1.55e-15 at (31, 3), whose dense random matrices amplify
    a rounding the most; the bound is ten times the largest."""
    c = ic.case(n, M)
    worst = 0.0
    for b in range(ic.B):
        G, C, J = c["G"][b], np.zeros((n, n)), c["J"][b].real.astype(complex)
        args = (c["dev_d"], c["dev_g"], c["dev_s"], c["coef"][b], c["out"])
        fl, _, x, _ = iref.solve(G, C, J, None, 1.0, 0.5, *args)
        fd, _, h, _, _ = dref.solve(G, C, J, 1.0, *args)
        assert fl == 0 and fd == 0 and np.all(x.imag == 0)
        for got, want in ((x[2], 2.0 * h[1]), (x[3], 2.0 * h[1]), (x[4], h[1]), (x[5], 3.0 * h[2]), (x[0], h[0]), (x[1], h[0])):
            assert np.any(want != 0)
            worst = max(worst, np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("n %d M %d: largest relative difference %.3e" % (n, M, worst))
    assert worst < DISTO_CROSS_BOUND


# ---- 4. the host-compiled ac_imd.hpp against the reference ----------------------------------------------------------

# binary records on stdin -- int32 n, F, M, out_p, out_m, has_j2; G [n][n], C [n][n] row-major; J re [n], J im [n]; with
# has_j2 J2 re [n], J2 im [n]; omega1 [F], omega2 [F]; dev_d, dev_g, dev_s [M] int32; coef [M][7]; one line per pair:
# flags, x0 .. x5 (re im pairs), IM2+, IM2-, IM3 as %a
HOST_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ac_imd.hpp"
int main()
{
    int32_t hd[6];
    while (std::fread(hd, sizeof(int32_t), 6, stdin) == 6) {
        const int n = hd[0], F = hd[1], M = hd[2], ld = n + 1;
        std::vector<double> G((size_t)n * n), C((size_t)n * n), J(2 * n), J2(2 * n), om(2 * F), coef((size_t)M * 7 + 1),
            ar((size_t)n * ld), ai((size_t)n * ld), xr(6 * n), xi(6 * n);
        std::vector<int32_t> dev(3 * (size_t)M + 1);
        if (std::fread(G.data(), sizeof(double), G.size(), stdin) != G.size()) return 1;
        if (std::fread(C.data(), sizeof(double), C.size(), stdin) != C.size()) return 1;
        if (std::fread(J.data(), sizeof(double), J.size(), stdin) != J.size()) return 1;
        if (hd[5] && std::fread(J2.data(), sizeof(double), J2.size(), stdin) != J2.size()) return 1;
        if (!hd[5]) J2 = J;
        if (std::fread(om.data(), sizeof(double), om.size(), stdin) != om.size()) return 1;
        if (std::fread(dev.data(), sizeof(int32_t), 3 * (size_t)M, stdin) != 3 * (size_t)M) return 1;
        if (std::fread(coef.data(), sizeof(double), (size_t)M * 7, stdin) != (size_t)M * 7) return 1;
        for (int f = 0; f < F; ++f) {
            double im[3];
            const unsigned fl = csim::ac_imd_solve(n, G.data(), C.data(), J.data(), J.data() + n, J2.data(), J2.data() + n,
                                                   om[f], om[F + f], M, dev.data(), dev.data() + M, dev.data() + 2 * M,
                                                   coef.data(), hd[3], hd[4], 1e-15, ld, ar.data(), ai.data(), xr.data(),
                                                   xi.data(), im);
            std::printf("%u", fl);
            for (int i = 0; i < 6 * n; ++i) std::printf(" %a %a", xr[i], xi[i]);
            std::printf(" %a %a %a\n", im[0], im[1], im[2]);
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_sweep(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("imd")
    cpp, exe = d / "drv.cpp", d / "drv"
    cpp.write_text(HOST_DRIVER)
    p = subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-w", "-I" + ENGINE_DIR,
                        "-I" + os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def sweep(c, omega1, omega2, J2=None):
        """-> per system (flags [F], h complex [F][6][n], im [F][3]), values exactly as printed (%a)"""
        n, M, F = c["n"], c["M"], len(omega1)
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
        i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).tobytes()       # noqa: E731
        blob = b"".join(i4([n, F, M, c["out"][0], c["out"][1], J2 is not None]) + f8(c["G"][b]) + f8(c["C"][b])
                        + f8(c["J"][b].real) + f8(c["J"][b].imag)
                        + (f8(J2[b].real) + f8(J2[b].imag) if J2 is not None else b"")
                        + f8(omega1) + f8(omega2) + i4(c["dev_d"]) + i4(c["dev_g"]) + i4(c["dev_s"]) + f8(c["coef"][b])
                        for b in range(len(c["G"])))
        lines = subprocess.run([str(exe)], input=blob, capture_output=True, check=True).stdout.decode().splitlines()
        assert len(lines) == len(c["G"]) * F
        res = []
        for b in range(len(c["G"])):
            fl, h, im = [], np.zeros((F, 6, n), dtype=complex), np.zeros((F, 3))
            for f in range(F):
                tok = lines[b * F + f].split()
                v = np.array([float.fromhex(t) for t in tok[1:]])
                fl.append(int(tok[0]))
                h[f].real, h[f].imag = v[0:12 * n:2].reshape(6, n), v[1:12 * n:2].reshape(6, n)
                im[f] = v[12 * n:]
            res.append((fl, h, im))
        return res
    return sweep


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _or(per):
    fl = 0
    for p in per:
        fl |= p
    return fl


@pytest.mark.parametrize("n,M", ic.CASES, ids=["n%d-M%d" % c for c in ic.CASES])
def test_reference_equals_host_compiled_header(host_sweep, n, M):
    c = ic.case(n, M)
    runs = [((n, M), None)] + ([((n, M, "j2"), ic.second_excitation(n, M))] if (n, M) in ic.J2_CASES else [])
    for key, J2 in runs:
        ref = ic.reference(key)
        for b, (fl, h, im) in enumerate(host_sweep(c, ic.OMEGA1, ic.OMEGA2, J2)):
            assert fl == [_or(p) for p in ref[b]["per_f"]] == [0] * len(ic.OMEGA1), (key, b)
            assert not np.isnan(ref[b]["h"].view(np.float64)).any()
            assert np.array_equal(_bits(h), _bits(ref[b]["h"])), (key, b)
            assert np.array_equal(_bits(im), _bits(ref[b]["im"])), (key, b)
            assert np.all(ref[b]["h"][:, :2] != 0)
            if M:
                assert np.all(ref[b]["im"] > 0)
            else:
                assert np.all(ref[b]["h"][:, 2:] == 0) and np.all(ref[b]["im"] == 0)
    if (n, M) in ic.J2_CASES:                                 # the second excitation reaches x1 and everything after it
        a, b = ic.reference((n, M))[0]["h"], ic.reference((n, M, "j2"))[0]["h"]
        assert np.array_equal(_bits(a[:, 0]), _bits(b[:, 0])) and np.array_equal(_bits(a[:, 4]), _bits(b[:, 4]))
        assert all(not np.array_equal(a[:, k], b[:, k]) for k in (1, 2, 3, 5))
    # the pairs: w2 == 0, w1 == w2, w1 < w2
    assert ic.OMEGA2[1] == 0 and ic.OMEGA1[2] == ic.OMEGA2[2] and ic.OMEGA1[3] < ic.OMEGA2[3]


def test_tank_fails_once_at_every_solve(host_sweep):
    """the LC tank is singular exactly where w == 1: pair q puts solve q there first.  The failed solve and every
    later one are +0.0, the earlier ones are not, the flag is set."""
    c = ic.tank()
    ref, = ic.reference("tank")
    (fl, h, im), = host_sweep(c, ic.TANK_OMEGA1, ic.TANK_OMEGA2)
    assert np.array_equal(_bits(h), _bits(ref["h"])) and np.array_equal(_bits(im), _bits(ref["im"]))
    for f, first in enumerate(ic.TANK_FAILS_AT):
        w = iref.frequencies(ic.TANK_OMEGA1[f], ic.TANK_OMEGA2[f])
        assert w[first] == 1.0 and all(abs(v) != 1.0 for v in w[:first])
        per = ref["per_f"][f]
        assert [k for k in range(6) if per[k]][0] == first, (f, per)
        assert fl[f] == 4
        for k in range(6):
            v = ref["h"][f, k].view(np.float64)
            if k >= first:
                assert np.all(v == 0) and not np.signbit(v).any(), (f, k)
            else:
                assert np.any(ref["h"][f, k] != 0), (f, k)
        want = [0 if first <= k else 1 for k in (2, 3, 5)] if first > 0 else [0, 0, 0]
        assert [int(x > 0) for x in ref["im"][f]] == want and not np.signbit(ref["im"][f]).any(), (f, ref["im"][f])
    assert ref["flags"] == 4


# ---- 7. refusals without a GPU --------------------------------------------------------------------------------------

ORDER = "device n B G Cm J J2 M dev_d dev_g dev_s coef out_p out_m omega1 omega2 F kernel h im flags".split()


def _call(**change):
    i4 = lambda *v: np.array(v, dtype=np.int32)     # noqa: E731
    a = dict(device=0, n=2, B=1, G=np.eye(2)[None].copy(), Cm=np.zeros((1, 2, 2)), J=np.ones((1, 2, 2)), J2=np.ones((1, 2, 2)),
             M=1, dev_d=i4(0), dev_g=i4(1), dev_s=i4(-1), coef=np.ones((1, 1, 7)), out_p=0, out_m=-1, omega1=np.ones(1),
             omega2=np.ones(1), F=1, kernel=0, h=np.zeros((1, 1, 6, 2, 2)), im=np.zeros((1, 1, 3)),
             flags=np.zeros(1, dtype=np.uint32))
    for k, v in change.items():
        assert k in a, k
        a[k] = np.asarray(v, dtype=a[k].dtype) if isinstance(a[k], np.ndarray) and v is not None else v
    keep = [v for v in a.values() if isinstance(v, np.ndarray)]
    rc = capi.lib().csim_imd_solve_batch(*[a[k].ctypes.data if isinstance(a[k], np.ndarray) else a[k] for k in ORDER])
    del keep
    return rc


ARG_CASES = [dict(n=-1), dict(B=-1), dict(F=-1), dict(M=-1), dict(kernel=3), dict(kernel=5), dict(kernel=-1),
             dict(G=None), dict(Cm=None), dict(J=None), dict(omega1=None), dict(omega2=None), dict(im=None), dict(dev_d=None),
             dict(dev_g=None), dict(dev_s=None), dict(coef=None),
             dict(out_p=2), dict(out_p=-1), dict(out_m=2), dict(out_m=-2), dict(out_p=1, out_m=1),
             dict(dev_d=[2]), dict(dev_g=[2]), dict(dev_s=[2]), dict(dev_d=[-2]), dict(dev_g=[-2]), dict(dev_s=[-2]),
             dict(omega1=[np.inf]), dict(omega2=[np.nan]), dict(kernel=3, n=64)]


@pytest.mark.parametrize("change", ARG_CASES, ids=lambda c: "-".join("%s=%s" % (k, "null" if v is None else v) for k, v in c.items()))
def test_refused_at_the_argument_stage(change):
    assert _call(**change) == capi.CSIM_ERR_ARG, capi.lib().csim_last_error()


def test_empty_calls_pass_the_argument_stage():
    after = capi.CSIM_OK if has_gpu() else capi.CSIM_ERR_NO_DEVICE
    nulls = dict(G=None, Cm=None, J=None, J2=None, omega1=None, omega2=None, im=None)
    assert _call(F=0, **nulls) == after and _call(B=0, **nulls) == after
    assert _call(h=None, flags=None, J2=None, M=0, dev_d=None, dev_g=None, dev_s=None, coef=None) == after


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_need_a_device():
    """the device check comes after the argument checks and before the refusal of the block kernel and of the sizes;
    negative and zero frequencies are valid"""
    assert _call() == capi.CSIM_ERR_NO_DEVICE
    assert _call(omega1=[-1.0], omega2=[0.0]) == capi.CSIM_ERR_NO_DEVICE
    assert _call(kernel=4) == capi.CSIM_ERR_NO_DEVICE
    assert _call(n=64, G=np.eye(64)[None], Cm=np.zeros((1, 64, 64)), J=np.zeros((1, 64, 2)), J2=None,
                 h=np.zeros((1, 1, 6, 64, 2))) == capi.CSIM_ERR_NO_DEVICE
    assert _call(n=33, kernel=2, G=np.eye(33)[None], Cm=np.zeros((1, 33, 33)), J=np.zeros((1, 33, 2)), J2=None,
                 h=np.zeros((1, 1, 6, 33, 2))) == capi.CSIM_ERR_NO_DEVICE


# ---- 5. resources -----------------------------------------------------------------------------------------------------

def test_imd_kernel_resources(tmp_path):
    """Tripwire, by the means of the single-tone kernels' test: no kernel of kernels_imd.hip uses scratch or spills, at
    any packed size (NP = 32 is the one at risk); the packed kernels' static LDS is the small tile (the solution, four
    kept solutions, one device round: 6.5 KiB for the two instances) and the wave kernel has none beside its dynamic carve"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "imd.s"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + ENGINE_DIR, "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "api"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ENGINE_DIR, "kernels_imd.hip"), "-o", str(asm)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    # one metadata record per kernel, its keys in alphabetical order (.name in the middle): "  - .agpr_count:" opens it
    meta, rec = {}, None
    fields = "private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|agpr_count"
    for line in asm.read_text().splitlines():
        if re.match(r"  - \.\w+:", line):
            rec = {}
        m = re.match(r"\s+(?:- )?\.name:\s+(\S+)", line)
        if m and rec is not None and "ac_imd" in m.group(1):
            meta[m.group(1)] = rec
        m = re.match(r"\s+(?:- )?\.(%s):\s+(\d+)" % fields, line)
        if m and rec is not None:
            rec[m.group(1)] = int(m.group(2))
    packed = {k: v for k, v in meta.items() if "ac_imd_packed_kernel" in k}
    wave = {k: v for k, v in meta.items() if "ac_imd_wave_kernel" in k}
    assert len(packed) == 4 and any("ILi32E" in k for k in packed), sorted(meta)
    assert len(wave) == 1 and len(meta) == 5, sorted(meta)
    for k, v in meta.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
    for k, v in packed.items():
        assert v["group_segment_fixed_size"] == 8 * (2 * 2 * 32 + 2 * 4 * 2 * 32 + 2 * 2 * 32) + 4 * 2 * 2 * 32, (k, v)
    for k, v in wave.items():
        assert v["group_segment_fixed_size"] == 0, (k, v)
    print("kernels_imd.hip VGPRs (+AGPRs):", {k[-40:]: (v["vgpr_count"], v.get("agpr_count", 0)) for k, v in meta.items()})
