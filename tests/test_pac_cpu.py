"""Periodic AC analysis without a GPU: the numpy restatement (tests/pac_reference.py) against the closed form of a linear
circuit and against an independent time-domain experiment, the host-compiled engine/pac.hpp against the restatement bit
for bit, the .PAC card, the refusals that need no engine, and the register budget of the kernels."""
import cmath
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pac_cases as ac
import pac_reference as par
import pss_reference as pr
from circuitsimulator_amd import CsimError, Netlist, capi, pss_twiddles
from conftest import ROOT, netlist_path
from oracle import binding as oracle

ENGINE_DIR = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")
ARG, CONFIG = capi.CSIM_ERR_ARG, capi.CSIM_ERR_CONFIG
M = ac.N_SIDE


# ---- 1. linear circuits: the restatement against (J - z Hm)^-1 u -------------------------------------------------------

@pytest.mark.parametrize("name", ac.LINEAR)
def test_reference_on_linear_circuits_against_the_closed_form(name):
    """A linear circuit translates nothing: P_0 is the AC solution with j w replaced by (1 - e^{-j w h}) / h and every
    other sideband is rounding.  The restatement reaches P_0 through K steps and the closure, the closed form through one
    solve in extended precision; they may differ by the bound of pac_reference.agreement_bound."""
    nl, h, K = par.setup(name)
    u = par.excitation(nl)
    _, _, res = par.reference(name, 3)
    for b, r in enumerate(res):
        assert not np.any(r["status"])
        for f in range(len(ac.freqs(name))):
            want = par.closed_form_linear(r["Js"][0], r["Hm"], u, r["z"][f]).astype(complex)
            err = float(np.max(np.abs(r["P"][f, M] - want)))
            bound = par.agreement_bound(r, f)
            side = float(np.max(np.abs(np.delete(r["P"][f], M, axis=0))))
            p0 = float(np.max(np.abs(r["P"][f, M])))
            print("%s instance %d f %.3g: |P0 - closed form| %.3e, bound %.3e, sidebands %.3e of |P0| %.3g"
                  % (name, b, ac.freqs(name)[f], err, bound, side / p0, p0))
            assert err <= bound
            assert side <= 1e-12 * p0


# ---- 2. the time-domain experiment --------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps,limit", [(1e-3, 2e-5), (1e-2, 1e-3)])
def test_reference_against_a_time_domain_experiment(eps, limit):
    """cs_rf with its 0 V source turned into a tone eps sin(2 pi f t) at f = f0 / 2, shot over the doubled period (K' = 2 K):
    the odd harmonics of that orbit exist only because of the tone.  eps sin = Re(a e^{j 2 pi f t}) with a = -j eps, the
    analysis was excited with 1 at 30 degrees, and the sidebands m and -m-1 land on the same positive frequency
    (m + 1/2) f0:  X'[2 m + 1] = (a / e^{j pi / 6}) P_m + conj((a / e^{j pi / 6}) P_(-m-1)),  m = 0 .. 3.
    Measured here: 3.8e-6 of eps at eps = 1e-3 (the limit is 5 times that, for other libm and LAPACK builds), 2.6e-4 at
    eps = 1e-2, where the second-order terms dominate (limit 1e-3)."""
    nl, h, K = par.setup("cs_rf")
    N = nl.n_unknowns
    p = ac.params(nl, 1)
    x_dc, _, _ = oracle.dc(nl.ir_ptr, N, p, 0)
    o = pr.shoot(nl.ir_ptr, N, p, 0, h, K, x_dc, pr.TOL, pr.MAX_ROUNDS, 0)
    r = par.pac(nl.ir_ptr, N, p, 0, h, K, ac.F0, o["x0"], [ac.F0 / 2], 4, par.excitation(nl), orbit=(o["xs"], o["W"]))
    assert o["status"] == 0 and not np.any(r["status"])
    assert abs(np.max(np.abs(r["P"]))) <= 1.3
    tone = Netlist.from_text(ac.CS_RF.replace("Vrf g lo DC 0 AC 1 30", "Vrf g lo SIN 0 %r 0.5e6 0" % eps))
    assert tone.n_unknowns == N
    p2 = ac.params(tone, 1)
    x2, _, _ = oracle.dc(tone.ir_ptr, N, p2, 0)
    o2 = pr.shoot(tone.ir_ptr, N, p2, 0, h, 2 * K, x2, pr.TOL, pr.MAX_ROUNDS, 7)
    assert o2["status"] == 0
    a = -1j * eps / cmath.exp(1j * np.pi / 6.0)
    worst = 0.0
    for m in range(4):
        want = a * r["P"][0, 4 + m] + np.conj(a * r["P"][0, 4 - m - 1])
        worst = max(worst, float(np.max(np.abs(o2["harm"][2 * m + 1] - want))))
    print("eps %g: error / eps %.3e (limit %.1e)" % (eps, worst / eps, limit))
    assert worst / eps <= limit


# ---- 3. engine/pac.hpp on the host against the restatement, bit for bit -------------------------------------------------

HOST_DRIVER = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "pac.hpp"
using namespace csim;
static bool rd(void* p, size_t n) { return fread(p, 1, n, stdin) == n; }
int main()
{
    int32_t hd[4];
    while (rd(hd, sizeof hd)) {
        const int K = hd[0], N = hd[1], F = hd[2], M = hd[3];
        std::vector<double> Hm((size_t)N * N), W((size_t)N * N), pr((size_t)K * N * F), pi(pr.size()), c(K), s(K), z(4 * F), u(2 * N),
            fr(F);
        double h, f0;
        if (!rd(Hm.data(), 8 * Hm.size()) || !rd(W.data(), 8 * W.size()) || !rd(pr.data(), 8 * pr.size()) ||
            !rd(pi.data(), 8 * pi.size()) || !rd(c.data(), 8 * K) || !rd(s.data(), 8 * K) || !rd(z.data(), 8 * z.size()) ||
            !rd(u.data(), 8 * u.size()) || !rd(fr.data(), 8 * F) || !rd(&h, 8) || !rd(&f0, 8)) return 2;
        std::vector<double> out;
        // q = Hm p_1 and z q + u, per frequency
        for (int part = 0; part < 4; ++part)
            for (int i = 0; i < N; ++i)
                for (int f = 0; f < F; ++f) {
                    double qr = 0.0, qi = 0.0;
                    for (int l = 0; l < N; ++l) {
                        const double hv = Hm[(size_t)i * N + l];
                        if (hv == 0.0) continue;
                        qr = pac_hm_add(qr, hv, pr[((size_t)0 * N + l) * F + f]);
                        qi = pac_hm_add(qi, hv, pi[((size_t)0 * N + l) * F + f]);
                    }
                    double re, im;
                    pac_step_rhs(z[f], z[F + f], qr, qi, u[i], u[N + i], &re, &im);
                    out.push_back(part == 0 ? qr : part == 1 ? qi : part == 2 ? re : im);
                }
        // sideband sums of p_1 .. p_K
        for (int part = 0; part < 2; ++part)
            for (int f = 0; f < F; ++f)
                for (int m = -M; m <= M; ++m)
                    for (int q = 0; q < N; ++q) {
                        double re = 0.0, im = 0.0;
                        for (int k = 1; k <= K; ++k) {
                            const int j = pac_tw_index(m, k, K);
                            pac_sum_add(pr[((size_t)(k - 1) * N + q) * F + f], pi[((size_t)(k - 1) * N + q) * F + f], c[j], s[j], &re, &im);
                        }
                        pac_sum_finish(K, &re, &im);
                        out.push_back(part == 0 ? re : im);
                    }
        // entries of I - z_K W at the first frequency
        for (int part = 0; part < 2; ++part)
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) {
                    double re, im;
                    pac_close_entry(i, j, W[(size_t)i * N + j], z[2 * F], z[3 * F], &re, &im);
                    out.push_back(part == 0 ? re : im);
                }
        // z and z_K of this build of the header
        for (int f = 0; f < F; ++f) {
            double v[4];
            pac_z(fr[f], h, f0, &v[0], &v[1], &v[2], &v[3]);
            out.insert(out.end(), v, v + 4);
        }
        fwrite(out.data(), 8, out.size(), stdout);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_pac(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("pac")
    cpp, exe = d / "drv.cpp", d / "drv"
    cpp.write_text(HOST_DRIVER)
    p = subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-w", "-I" + ENGINE_DIR, str(cpp), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def run(items):
        """items: [(Hm, W, ps complex [K][N][F], c, s, z [F], zK [F], u [N], freqs, h, f0, M)] -> [dict]"""
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()     # noqa: E731
        blob = b""
        for Hm, W, ps, c, s, z, zK, u, fr, h, f0, m in items:
            K, N, F = ps.shape
            blob += (struct.pack("<4i", K, N, F, m) + f8(Hm) + f8(W) + f8(ps.real) + f8(ps.imag) + f8(c) + f8(s) +
                     f8(np.concatenate([z.real, z.imag, zK.real, zK.imag])) + f8(np.concatenate([u.real, u.imag])) + f8(fr) +
                     struct.pack("<2d", h, f0))
        raw = np.frombuffer(subprocess.run([str(exe)], input=blob, capture_output=True, check=True).stdout, dtype=np.float64)
        res, at = [], 0
        for Hm, W, ps, c, s, z, zK, u, fr, h, f0, m in items:
            K, N, F = ps.shape
            step = raw[at:at + 4 * N * F].reshape(4, N, F); at += step.size
            sums = raw[at:at + 2 * F * (2 * m + 1) * N].reshape(2, F, 2 * m + 1, N); at += sums.size
            ent = raw[at:at + 2 * N * N].reshape(2, N, N); at += ent.size
            zz = raw[at:at + 4 * F].reshape(F, 4); at += zz.size
            res.append(dict(step=step, sums=sums, entry=ent, z=zz))
        assert at == raw.size
        return res
    return run


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name,B", [("rc", 3), ("rlc", 3), ("divider", 3), ("cs_rf", 65), ("mixer", 3)])
def test_host_header_matches_the_restatement_bit_for_bit(host_pac, name, B):
    """the product Hm p, the step's right-hand side z q + u, the sideband sums with their finish and the entries of
    I - z_K W_K, on the perturbations of every instance the GPU tests run; z and z_K of this build of the header against
    the restatement's, to an ulp"""
    nl, h, K = par.setup(name)
    c, s = pss_twiddles(K)
    u = par.excitation(nl)
    _, _, res = par.reference(name, B)
    fr = ac.freqs(name)
    items = [(r["Hm"], r["W"], r["ps"], c, s, r["z"], r["zK"], u, fr, h, ac.F0, M) for r in res]
    got = host_pac(items)
    for (Hm, W, ps, _, _, z, zK, _, _, _, _, _), g in zip(items, got):
        p1r, p1i = np.ascontiguousarray(ps[0].real), np.ascontiguousarray(ps[0].imag)
        qr, qi = par.hm_product(Hm, p1r, p1i)
        re, im = par.step_rhs(np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag), qr, qi, np.ascontiguousarray(u.real),
                              np.ascontiguousarray(u.imag))
        for k, want in enumerate((qr, qi, re, im)):
            assert np.array_equal(_bits(g["step"][k]), _bits(want)), (name, k)
        P = par.sideband_sums(ps, c, s, M)
        assert np.array_equal(_bits(g["sums"][0]), _bits(P.real)) and np.array_equal(_bits(g["sums"][1]), _bits(P.imag))
        Ar, Ai = par.close_matrix(W, zK[0])
        assert np.array_equal(_bits(g["entry"][0]), _bits(Ar)) and np.array_equal(_bits(g["entry"][1]), _bits(Ai))
        # the constants are made once, by the library; another compiler's build of the same lines may pair sin and cos
        # into one call of another routine: within an ulp of 1
        want = np.stack([z.real, z.imag, zK.real, zK.imag], axis=1)
        assert np.max(np.abs(g["z"] - want)) <= 2.3e-16


def test_z_of_a_whole_number_of_periods_is_one():
    """z_K comes from the fractional part of f / f0, never from powering z: at f = f0 and 3 f0 it is exactly 1"""
    for f in (ac.F0, 3 * ac.F0):
        z, zK = par.z_consts(f, 1.0 / (64 * ac.F0), ac.F0)
        assert zK == 1.0 and z != 1.0


# ---- 4. the .PAC card ---------------------------------------------------------------------------------------------------

BASE = "V1 a 0 DC 1 AC 1\nR1 a 0 1k\n.TRAN 1n 10n\n"


def test_pac_card_forms():
    assert Netlist.from_text(BASE).pac is None
    assert Netlist.from_text(BASE + ".pac dec 10 1k 1meg\n").pac == ("dec", 10, 1e3, 1e6, 1)
    assert Netlist.from_text(BASE + ".PAC LIN 16 790meg 810meg 2\n").pac == ("lin", 16, 790e6, 810e6, 2)
    assert Netlist.from_text(BASE + ".Pac oct 3 1k 8k 0\n").pac == ("oct", 3, 1e3, 8e3, 0)
    assert Netlist.from_text(BASE + ".pac dec 10 1k 1meg\n.pac lin 2 1 2 3\n").pac == ("lin", 2, 1.0, 2.0, 3)   # the last card counts
    nl = Netlist.from_text(ac.MIXER)
    assert nl.pac == ("lin", 3, 0.3e6, 0.9e6, 2) and nl.hb == (1e6, 3)
    assert __import__("circuitsimulator_amd").pss_num_steps(nl.tstep, 1e6) == ac.CASES["mixer"][1]
    assert np.array_equal(nl.pac_freqs(), np.array([0.3e6, 0.6e6, 0.9e6]))
    assert np.array_equal(Netlist.from_text(BASE + ".pac dec 2 1 100\n").pac_freqs(),
                          Netlist.from_text(BASE + ".ac dec 2 1 100\n").ac_freqs())
    with pytest.raises(CsimError) as e:
        Netlist.from_text(BASE).pac_freqs()
    assert e.value.code == CONFIG


@pytest.mark.parametrize("card", [".pac", ".pac dec 10 1k", ".pac foo 10 1k 1meg", ".pac dec x 1k 1meg", ".pac dec 10 1k abc",
                                  ".pac dec 10 1k 1meg 2 7", ".pac dec 10 1k 1meg -1", ".pac dec 10 1k 1meg 1.5"])
def test_pac_card_errors_leave_the_card_off(card, capfd):
    nl = Netlist.from_text(BASE + card + "\n")
    assert nl.pac is None
    assert ".pac" in capfd.readouterr().err.lower()
    v = [C.c_int32(7) for _ in range(3)]
    f0, f1, ns = C.c_double(7.0), C.c_double(7.0), C.c_int32(7)
    L = capi.lib()
    assert L.csim_netlist_pac(nl.handle, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(f0), C.byref(f1), C.byref(ns)) == capi.CSIM_OK
    assert (v[0].value, v[2].value, f0.value, f1.value, ns.value) == (0, 0, 0.0, 0.0, 0)
    assert L.csim_netlist_pac(None, None, None, None, None, None, None) == ARG
    assert L.csim_netlist_pac(nl.handle, None, None, None, None, None, None) == capi.CSIM_OK


@pytest.mark.parametrize("name", ["buffer.sp", "dbmixer.sp"])
def test_shipped_netlists_unchanged_by_a_pac_card(name):
    """The shipped netlists carry no .PAC card; adding one changes nothing else they report."""
    text = open(netlist_path(name)).read()
    ref = Netlist.from_text(text)
    assert ref.pac is None
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.strip().lower().startswith(".hb"))
    nz = Netlist.from_text("\n".join(lines[:at] + [".pac lin 16 790meg 810meg"] + lines[at:]) + "\n")
    assert nz.pac == ("lin", 16, 790e6, 810e6, 1)
    assert nz.n_params == ref.n_params and nz.n_unknowns == ref.n_unknowns and nz.n_elems == ref.n_elems
    assert np.array_equal(nz.nominal_params, ref.nominal_params)
    assert nz.eq_names == ref.eq_names and nz.csv_header == ref.csv_header and nz.probes == ref.probes
    assert np.array_equal(nz.mc_kinds, ref.mc_kinds)
    assert (nz.tran_enabled, nz.tstep, nz.tstop, nz.tstart) == (ref.tran_enabled, ref.tstep, ref.tstop, ref.tstart)
    assert (nz.ac, nz.noise, nz.sp, nz.disto, nz.stb, nz.hb) == (ref.ac, ref.noise, ref.sp, ref.disto, ref.stb, ref.hb)
    assert nz.noise_sources == ref.noise_sources and nz.disto_devices == ref.disto_devices


# ---- 5. refusals that need no engine (the rest: tests/test_pac_gpu.py, an engine needs a device) ------------------------

def test_null_engine_is_an_argument_error():
    L = capi.lib()
    buf = np.ones(64)
    p = buf.ctypes.data
    assert L.csim_pac_batch_dev(None, p, 1, 1e-9, 10e6, p, p, 1, 1, None, 0, p, p, None) == ARG
    assert L.csim_pac_batch(None, None, 1, 1e-9, 10e6, p, 1, 1, None, 0, p, None, None, None) == ARG
    assert capi.ST_PAC_SINGULAR == 0x0800 == par.ST_PAC_SINGULAR


# ---- 6. registers -------------------------------------------------------------------------------------------------------

def test_pac_kernel_registers(tmp_path):
    """Tripwire: neither kernel of kernels_pac.hip uses scratch memory or spills a vector register."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    obj = tmp_path / "pac.o"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage",
                        "-I" + ENGINE_DIR, "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "api"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ENGINE_DIR, "kernels_pac.hip"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    blocks = re.split(r"Function Name: ", c.stderr)[1:]
    seen = {}
    for blk in blocks:
        fn = blk.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", blk).group(1))     # noqa: E731
        seen[fn] = (num(r"VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"VGPRs Spill"))
    print(seen)
    assert any("k_pac_period" in k for k in seen) and any("k_period_close" in k for k in seen)
    for fn, (vgpr, scratch, spill) in seen.items():
        assert scratch == 0 and spill == 0, (fn, vgpr, scratch, spill)
