"""Periodic steady state without a GPU: the numpy restatement (tests/pss_reference.py) against the closed form of the
linear recursion and the analytic backward-Euler transfer, the host-compiled engine/pss.hpp against the restatement bit
for bit, the .HB card, the refusals that need no engine, K and the table, and the register budget of the kernels."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pss_cases as pc
import pss_reference as pr
from circuitsimulator_amd import CsimError, Netlist, capi, pss_num_steps, pss_twiddles
from conftest import ROOT, netlist_path

ENGINE_DIR = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")
ARG, CONFIG = capi.CSIM_ERR_ARG, capi.CSIM_ERR_CONFIG


# ---- 1. the restatement against what a steady state is ---------------------------------------------------------------

def _state_bound(A, Minv, K):
    """||(I - A^K)^-1||_inf (tol + per-step floor): how far a state that closes within tol under the damped iteration
    may be from the fixed point of the exact recursion.  Derived in pss_reference.step_floor, not tuned."""
    return pr.norm_inf(Minv) * (pr.TOL + pr.step_floor(A, K))


@pytest.mark.parametrize("name", ["rc", "rlc"])
def test_reference_x0_against_the_closed_form(name):
    nl, h, K, H = pr.setup(name)
    p, res = pr.reference(name, 3)
    for b, r in enumerate(res):
        assert r["status"] == 0 and r["closure"] < pr.TOL
        A, src = pr.linear_recursion(nl.ir_ptr, nl.n_unknowns, p, b, h, K)
        xstar, orbit, Minv = pr.closed_form(A, src)
        bound = _state_bound(A, Minv, K)
        err = float(np.max(np.abs(r["x0"] - xstar.astype(np.float64))))
        print("%s instance %d: |x0 - x0*| %.3e, bound %.3e, rounds %d" % (name, b, err, bound, r["rounds"]))
        assert err <= bound
        assert float(np.max(np.abs(orbit[-1] - xstar))) < 1e-15          # the closed form is periodic


def test_reference_harmonics_of_the_rc_against_the_analytic_transfer():
    """One node with a capacitor: (1/R + gmin + C/h) x_k = u_k / R + (C/h) x_(k-1), u_k = 100 sin(2 pi k / K).  At the tone
    z = exp(j 2 pi / K) the phasor of the output is (1/R) / (1/R + gmin + (C/h)(1 - 1/z)) times -j (a sine against the
    cosine reference).  The closed-form orbit has exactly that harmonic (the double data's rounding, 1e-16 of 100 V, through ||(I - A^K)^-1|| = 200: 1e-10 asked);
    the restatement's differs from it by the state bound carried along the orbit, twice over for a peak phasor."""
    nl, h, K, H = pr.setup("rc")
    p, res = pr.reference("rc", 3)
    out = nl.node_eq("out")
    c, s = pss_twiddles(K)
    for b, r in enumerate(res):
        iR, iC = (int(np.argmin(np.abs(nl.nominal_params / v - 1.0))) for v in (1e3, 200e-9))   # the slots of R1 and C1
        assert abs(nl.nominal_params[iR] / 1e3 - 1.0) < 1e-12 and abs(nl.nominal_params[iC] / 200e-9 - 1.0) < 1e-12
        R, Cv = p[iR, b], p[iC, b]
        gmin = 1e-6
        z = np.exp(2j * np.pi / K)
        want = (1.0 / R) / (1.0 / R + gmin + (Cv / h) * (1.0 - 1.0 / z)) * (-100j)      # the source's amplitude is 100 V
        A, src = pr.linear_recursion(nl.ir_ptr, nl.n_unknowns, p, b, h, K)
        xstar, orbit, Minv = pr.closed_form(A, src)
        exact = pr.dft(orbit.astype(np.float64), c, s, 1)[1][out]
        assert abs(exact - want) < 1e-10
        powmax, P = 1.0, np.eye(nl.n_unknowns, dtype=np.longdouble)
        for _ in range(K):
            P = P @ A
            powmax = max(powmax, pr.norm_inf(P))
        bound = 2.0 * (powmax * _state_bound(A, Minv, K) + pr.step_floor(A, K))
        err = abs(r["harm"][1][out] - want)
        print("rc instance %d: X1 %s, analytic %s, |difference| %.3e, bound %.3e" % (b, r["harm"][1][out], want, err, bound))
        assert err <= bound
        assert abs(r["harm"][0][out]) <= bound and r["harm"][0][out].imag == 0.0


def test_reference_rounds_and_the_divider():
    for name in pc.LINEAR:
        _, res = pr.reference(name, 3)
        assert max(r["rounds"] for r in res) <= (1 if name == "divider" else 2), name
    _, res = pr.reference("divider", 3)
    assert all(np.all(r["W"] == 0.0) for r in res)
    _, res = pr.reference("cs", 3)
    print("common-source stage: rounds", [r["rounds"] for r in res])
    assert all(r["status"] == 0 and r["rounds"] <= pr.MAX_ROUNDS for r in res)


def test_the_common_source_stage_crosses_into_triode():
    nl, h, K, H = pr.setup("cs")
    p, res = pr.reference("cs", 1)
    xs = res[0]["xs"]
    vd, vg = xs[:, nl.node_eq("d")], xs[:, nl.node_eq("g")]
    vth = 0.5
    sat = (vg > vth) & (vd >= vg - vth)
    tri = (vg > vth) & (vd < vg - vth)
    off = vg <= vth
    print("steps in saturation %d, triode %d, cut-off %d" % (sat.sum(), tri.sum(), off.sum()))
    assert sat.sum() >= 4 and tri.sum() >= 4 and off.sum() >= 1


# ---- 2. engine/pss.hpp on the host against the restatement, bit for bit ------------------------------------------------

HOST_DRIVER = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "pss.hpp"
using namespace csim;
static bool rd(void* p, size_t n) { return fread(p, 1, n, stdin) == n; }
int main()
{
    int32_t hd[3];
    while (rd(hd, sizeof hd)) {
        const int K = hd[0], N = hd[1], H = hd[2];
        std::vector<double> xs((size_t)K * N), c(K), s(K), x0(N), xK(N), d(N), w((size_t)N * N);
        double tol;
        if (!rd(xs.data(), 8 * xs.size()) || !rd(c.data(), 8 * K) || !rd(s.data(), 8 * K) || !rd(x0.data(), 8 * N) ||
            !rd(xK.data(), 8 * N) || !rd(d.data(), 8 * N) || !rd(w.data(), 8 * w.size()) || !rd(&tol, 8)) return 2;
        std::vector<double> out;
        for (int m = 0; m <= H; ++m)
            for (int p = 0; p < N; ++p) {
                double re = 0.0, im = 0.0;
                for (int k = 1; k <= K; ++k) {
                    const int j = pss_tw_index(m, k, K);
                    pss_dft_add(xs[(size_t)(k - 1) * N + p], c[j], s[j], &re, &im);
                }
                pss_dft_finish(m, K, &re, &im);
                out.push_back(re);
                out.push_back(im);
            }
        std::vector<double> r(N);
        for (int i = 0; i < N; ++i) { r[i] = pss_residual(xK[i], x0[i]); out.push_back(r[i]); }
        const double nrm = pss_norm_inf(r.data(), N);
        out.push_back(nrm);
        out.push_back(pss_closed(nrm, tol) ? 1.0 : 0.0);
        for (int i = 0; i < N; ++i) out.push_back(pss_update(x0[i], d[i]));
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) out.push_back(pss_shoot_entry(i, j, w[(size_t)i * N + j]));
        std::vector<double> tc(K), ts(K);
        pss_twiddles(K, tc.data(), ts.data());
        out.insert(out.end(), tc.begin(), tc.end());
        out.insert(out.end(), ts.begin(), ts.end());
        fwrite(out.data(), 8, out.size(), stdout);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_pss(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("pss")
    cpp, exe = d / "drv.cpp", d / "drv"
    cpp.write_text(HOST_DRIVER)
    p = subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-w", "-I" + ENGINE_DIR, str(cpp), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def run(items):
        """items: [(xs [K][N], c, s, H, x0, xK, d, W, tol)] -> [dict] from the host-compiled header"""
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
        blob = b"".join(struct.pack("<3i", xs.shape[0], xs.shape[1], H) + f8(xs) + f8(c) + f8(s) + f8(x0) + f8(xK) + f8(d) +
                        f8(W) + struct.pack("<d", tol) for xs, c, s, H, x0, xK, d, W, tol in items)
        raw = np.frombuffer(subprocess.run([str(exe)], input=blob, capture_output=True, check=True).stdout, dtype=np.float64)
        res, at = [], 0
        for xs, c, s, H, x0, xK, d, W, tol in items:
            K, N = xs.shape
            take = lambda n: raw[at:at + n]                                       # noqa: E731
            harm = take(2 * (H + 1) * N).reshape(H + 1, N, 2); at += harm.size
            r = take(N); at += N
            nrm, closed = raw[at], raw[at + 1]; at += 2
            upd = take(N); at += N
            ent = take(N * N).reshape(N, N); at += N * N
            tc = take(K); at += K
            ts = take(K); at += K
            res.append(dict(harm=harm, r=r, norm=nrm, closed=bool(closed), upd=upd, entry=ent, c=tc, s=ts))
        assert at == raw.size
        return res
    return run


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name,B", [(n, 65) for n in pc.CASES] + [(n, 3) for n in pc.SHIPPED])
def test_host_header_matches_the_restatement_bit_for_bit(host_pss, name, B):
    """the DFT, the residual, its norm, the closure decision, the update and the entries of I - W, on the last trajectory
    of every instance the GPU tests shoot; the table of this build of the header against the library's, to an ulp"""
    nl, h, K, H = pr.setup(name)
    _, res = pr.reference(name, B)
    c, s = pss_twiddles(K)
    rng = np.random.default_rng(7)
    items = []
    for r in res:
        xs = r["xs"]
        d = rng.standard_normal(xs.shape[1]) * 1e-3
        items.append((xs[1:], c, s, H, xs[0], xs[K], d, r["W"], pr.TOL))
    got = host_pss(items)
    for (xs, _, _, _, x0, xK, d, W, tol), g in zip(items, got):
        want = pr.dft(xs, c, s, H)
        assert np.array_equal(_bits(g["harm"][..., 0]), _bits(want.real))
        assert np.array_equal(g["harm"][..., 1], want.imag)               # -0.0 and +0.0 compare equal here, as in numpy's DFT
        assert np.array_equal(_bits(g["harm"][1:, :, 1]), _bits(want.imag[1:]))
        assert np.array_equal(_bits(g["r"]), _bits(xK - x0))
        assert g["norm"] == float(np.max(np.abs(xK - x0))) and g["closed"] == (g["norm"] < tol)
        assert np.array_equal(_bits(g["upd"]), _bits(x0 + d))
        assert np.array_equal(_bits(g["entry"]), _bits(np.where(np.eye(len(x0), dtype=bool), 1.0, 0.0) - W))
        # the table is made once, by the library; another compiler's build of the same loop may pair sin and cos into
        # one call of another routine: within an ulp of 1
        assert np.max(np.abs(g["c"] - c)) <= 2.3e-16 and np.max(np.abs(g["s"] - s)) <= 2.3e-16


# ---- 3. K and the table ----------------------------------------------------------------------------------------------

def test_num_steps():
    L = capi.lib()
    for name in pc.CASES:
        assert pss_num_steps(pc.tstep(name), pc.F0) == pc.CASES[name][1]
    assert pss_num_steps(1e-9, 10e6) == 100 and pss_num_steps(5e-11, 100e6) == 200
    assert pss_num_steps(1e-13, 100e6) == 100000                            # dbmixer.sp's own cards
    assert L.csim_pss_num_steps(1e-9, 1e-2) == CONFIG                       # buffer.sp's own cards: 1e11 steps, over the cap
    assert L.csim_pss_num_steps(1.0 / (1 << 22), 1.0) == 1 << 22
    assert L.csim_pss_num_steps(1.0 / (1 << 23), 1.0) == CONFIG
    assert L.csim_pss_num_steps(3e-9, 100e6) == CONFIG                      # 3.33 steps
    assert L.csim_pss_num_steps(1e-9 * (1 + 1e-8), 10e6) == CONFIG          # off by 1e-8 relative
    assert L.csim_pss_num_steps(1e-9 * (1 + 1e-10), 10e6) == 100            # within 1e-9
    assert L.csim_pss_num_steps(2e-6, 1e6) == CONFIG                        # half a step per period
    assert L.csim_pss_num_steps(0.0, 1e6) == CONFIG and L.csim_pss_num_steps(1e-9, -1.0) == CONFIG
    for bad in (float("nan"), float("inf")):
        assert L.csim_pss_num_steps(bad, 1e6) == ARG and L.csim_pss_num_steps(1e-9, bad) == ARG
    with pytest.raises(CsimError) as e:
        pss_num_steps(3e-9, 100e6)
    assert e.value.code == CONFIG


def test_twiddles():
    L = capi.lib()
    for K in (1, 2, 16, 32, 48, 64, 100, 200):
        c, s = pss_twiddles(K)
        rc, rs = pr.twiddles(K)
        assert c.shape == (K,) and c[0] == 1.0 and s[0] == 0.0
        assert np.max(np.abs(c - rc)) <= 2.3e-16 and np.max(np.abs(s - rs)) <= 2.3e-16     # one ulp of 1: two libms
        j = np.arange(K)
        exact = np.exp(2j * np.pi * j.astype(np.longdouble) / K)
        assert np.max(np.abs(c + 1j * s - exact.astype(complex))) < 1e-15
    buf = np.zeros(4)
    assert L.csim_pss_twiddles(0, buf.ctypes.data, buf.ctypes.data) == ARG
    assert L.csim_pss_twiddles((1 << 22) + 1, buf.ctypes.data, buf.ctypes.data) == ARG
    assert L.csim_pss_twiddles(4, None, buf.ctypes.data) == ARG and L.csim_pss_twiddles(4, buf.ctypes.data, None) == ARG


# ---- 4. the .HB card --------------------------------------------------------------------------------------------------

BASE = "V1 a 0 DC 1\nR1 a 0 1k\n.TRAN 1n 10n\n"


def test_hb_card_forms_and_shipped_values(buffer_nl, dbmixer_nl):
    assert dbmixer_nl.hb == (100e6, 50)
    assert buffer_nl.hb == (1e-2, 3)
    assert Netlist.from_text(BASE).hb is None
    assert Netlist.from_text(BASE + ".hb 1e6 7\n").hb == (1e6, 7)
    assert Netlist.from_text(BASE + ".HB 2meg 4\n").hb == (2e6, 4)
    assert Netlist.from_text(BASE + ".Hb 1k 0 extra\n").hb == (1e3, 0)      # further tokens are ignored, as upstream
    assert Netlist.from_text(BASE + ".hb 1e6 3\n.hb 5e6 2\n").hb == (5e6, 2)  # the last card counts
    assert pc.netlist("rc").hb == (1e6, 3)


@pytest.mark.parametrize("card", [".hb", ".hb 1e6", ".hb abc 3", ".hb 1e6 x"])
def test_hb_card_errors_leave_the_card_off(card, capfd):
    nl = Netlist.from_text(BASE + card + "\n")
    assert nl.hb is None
    assert ".hb" in capfd.readouterr().err.lower()
    en, f0, nh = C.c_int32(7), C.c_double(7.0), C.c_int32(7)
    assert capi.lib().csim_netlist_hb(nl.handle, C.byref(en), C.byref(f0), C.byref(nh)) == capi.CSIM_OK
    assert (en.value, f0.value, nh.value) == (0, 0.0, 0)
    assert capi.lib().csim_netlist_hb(None, None, None, None) == ARG
    assert capi.lib().csim_netlist_hb(nl.handle, None, None, None) == capi.CSIM_OK


@pytest.mark.parametrize("name", ["buffer.sp", "dbmixer.sp"])
def test_shipped_netlists_unchanged_by_hb_card(name):
    """Removing the .HB card, or replacing it with another, changes nothing else the netlist reports."""
    text = open(netlist_path(name)).read()
    ref = Netlist.from_text(text)
    assert ref.hb is not None
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.strip().lower().startswith(".hb"))
    without = Netlist.from_text("\n".join(lines[:at] + lines[at + 1:]) + "\n")
    other = Netlist.from_text("\n".join(lines[:at] + [".hb 25e6 9"] + lines[at + 1:]) + "\n")
    assert without.hb is None and other.hb == (25e6, 9)
    for nz in (without, other):
        assert nz.n_params == ref.n_params and nz.n_unknowns == ref.n_unknowns and nz.n_elems == ref.n_elems
        assert np.array_equal(nz.nominal_params, ref.nominal_params)
        assert nz.eq_names == ref.eq_names and nz.csv_header == ref.csv_header and nz.probes == ref.probes
        assert np.array_equal(nz.mc_kinds, ref.mc_kinds)
        assert (nz.tran_enabled, nz.tstep, nz.tstop, nz.tstart) == (ref.tran_enabled, ref.tstep, ref.tstop, ref.tstart)
        assert (nz.ac, nz.noise, nz.sp, nz.disto, nz.stb) == (ref.ac, ref.noise, ref.sp, ref.disto, ref.stb)
        assert nz.noise_sources == ref.noise_sources and nz.disto_devices == ref.disto_devices


# ---- 5. refusals that need no engine (the rest: tests/test_pss_gpu.py, an engine needs a device) ----------------------

def test_null_engine_is_an_argument_error():
    L = capi.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    assert L.csim_pss_batch_dev(None, p, 1, 1e-9, 10e6, 1, None, 0, 0.0, 0, p, p, p, p, None) == ARG
    assert L.csim_pss_batch(None, None, 1, 1e-9, 10e6, 1, None, 0, 0.0, 0, p, p, p, p) == ARG


# ---- 6. registers ------------------------------------------------------------------------------------------------------

def test_pss_kernel_registers(tmp_path):
    """Tripwire: neither kernel of kernels_pss.hip uses scratch memory or spills a vector register."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    obj = tmp_path / "pss.o"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage",
                        "-I" + ENGINE_DIR, "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "api"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ENGINE_DIR, "kernels_pss.hip"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    blocks = re.split(r"Function Name: ", c.stderr)[1:]
    seen = {}
    for blk in blocks:
        fn = blk.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", blk).group(1))     # noqa: E731
        seen[fn] = (num(r"VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"VGPRs Spill"))
    print(seen)
    assert any("k_pss_period" in k for k in seen) and any("k_pss_update" in k for k in seen)
    for fn, (vgpr, scratch, spill) in seen.items():
        assert scratch == 0 and spill == 0, (fn, vgpr, scratch, spill)
