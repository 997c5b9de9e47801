"""Pole analysis without a GPU: the sequential statement of engine/pz.hpp, compiled for the host (tests/pz_host.py),
against closed forms, against numpy.linalg.eigvals on the golden netlists' own (G, C), the exactness of its balancing,
its flags and its order; and what the fixtures of the GPU kernel tests must satisfy."""
from decimal import Decimal, getcontext

import numpy as np
import pytest

import pz_cases as pc
import pz_host as ph
from conftest import netlist_path

ULP = 2.0 ** -52

# The closed forms are evaluated in 60-digit decimals from the stamped doubles, so the reference carries no rounding of
# its own.  What the routine adds: M by a 3 x 3 or 5 x 5 elimination with entries of G + 0 C that are exact or one
# rounding away, a 1 x 1 or 2 x 2 block whose eigenvalues hqr takes in closed form (one sqrt, a handful of products and
# sums), and one reciprocal -- each step at most an ulp or two of |s| on these well-conditioned systems.  Bound: 8 ulp
# of |s| ("a few").  Observed on the CPU: ac_rc_lowpass 0.04, pss_rc 0.14, ac_rlc_series 0.55 ulp.
ANALYTIC_ULPS = 8.0


def _system(name):
    import stb_netlist_system as sn
    from circuitsimulator_amd import Netlist
    nl = Netlist.from_file(netlist_path(name))
    G, C, _ = sn.nominal_system(nl)
    return nl, G, C


def _ulps(got, want_re, want_im):
    getcontext().prec = 60
    d = ((Decimal(float(got.real)) - want_re) ** 2 + (Decimal(float(got.imag)) - want_im) ** 2).sqrt()
    return float(d / (want_re ** 2 + want_im ** 2).sqrt()) / ULP


@pytest.mark.parametrize("name,r_ohm,c_farad", [("ac_rc_lowpass.sp", 1e3, 1e-9), ("pss_rc.sp", 1e3, 200 * 1e-9)])
def test_rc_lowpass_has_one_pole(name, r_ohm, c_farad):
    """-1 / (R C), with the gmin the stamp puts beside R: -(1 / R + gmin) / C"""
    getcontext().prec = 60
    nl, G, C = _system(name)
    o = nl.node_eq("out")
    assert C[o, o] == c_farad and abs(G[o, o] - 1.0 / r_ohm) <= 1.001e-6           # gmin = 1e-6 S
    r = ph.poles(G, C, 1e12)
    assert (r["flags"], r["n_poles"], r["n_rhp"]) == (0, 1, 0)
    want = -Decimal(float(G[o, o])) / Decimal(float(C[o, o]))
    assert abs(float(want) + 1.0 / (r_ohm * c_farad)) < 2e-3 / (r_ohm * c_farad)
    u = _ulps(r["poles"][0], want, Decimal(0))
    print("%s: pole %.17g, %.2f ulp" % (name, r["poles"][0].real, u))
    assert r["poles"][0].imag == 0.0 and u <= ANALYTIC_ULPS
    assert r["max_re"] == r["poles"][0].real and np.isnan(r["poles"][1:].view(np.float64)).all()


def test_series_rlc_has_a_conjugate_pair():
    """-R / 2L +- j sqrt(1 / LC - (R / 2L)^2); with the stamp's gmin g at both nodes the characteristic polynomial is
    L C s^2 + (L g + C / Ya) s + (g / Ya + 1), Ya = 1 / R + g, which is the textbook one at g = 0"""
    getcontext().prec = 60
    nl, G, C = _system("ac_rlc_series.sp")
    a, b, br = nl.node_eq("a"), nl.node_eq("b"), nl.eq_names.index("L1")
    ya, g, cb, ind = (Decimal(float(v)) for v in (G[a, a], G[b, b], C[b, b], -C[br, br]))
    assert (float(cb), float(ind)) == (1e-9, 1e-6) and abs(float(ya) - 0.02) <= 1.001e-6 and float(g) == 1e-6
    qa, qb, qc = ind * cb, ind * g + cb / ya, g / ya + 1
    re, im = -qb / (2 * qa), (4 * qa * qc - qb * qb).sqrt() / (2 * qa)
    assert abs(float(re) + 50.0 / 2e-6) < 1e-4 * 25e6 and abs(float(im) - np.sqrt(1e15 - 25e6 ** 2)) < 1e-4 * 25e6
    r = ph.poles(G, C, 1e12)
    assert (r["flags"], r["n_poles"], r["n_rhp"]) == (0, 2, 0)
    p0, p1 = r["poles"][:2]
    # the member with Im mu > 0 first: mu = 1 / s, so Im s < 0 first
    assert p0.real == p1.real and p0.imag == -p1.imag and p0.imag < 0.0
    u = max(_ulps(p0, re, -im), _ulps(p1, re, im))
    print("ac_rlc_series: pair %.17g +- %.17gj, %.2f ulp" % (p1.real, p1.imag, u))
    assert u <= ANALYTIC_ULPS


# ---- 2. against numpy on the golden netlists -------------------------------------------------------------------------

FMAX = 1e12
NETLISTS = [("stb_cs_loop.sp", 3), ("rlc_mesh.sp", 5), ("ac_rc_ladder.sp", 40), ("dbmixer.sp", 14), ("gate_only_node.sp", 9),
            ("disto_cs_amp.sp", 2), ("pac_switch_mixer.sp", 2)]


@pytest.mark.parametrize("name,count", NETLISTS)
def test_poles_against_numpy(name, count):
    """Per eigenvalue: 64 times the scatter numpy's own eigenvalue shows under 8 perturbations of relative size
    N 2^-52, floor N 2^-52 max|mu| (pz_host.scatter_bounds).  Observed largest ratio to that bound on the CPU:
    stb_cs_loop 0.0085, rlc_mesh 0.0060, ac_rc_ladder 0.018, dbmixer 0.0069, gate_only_node 0.020, disto_cs_amp 0.013,
    pac_switch_mixer 0.0085."""
    _, G, C = _system(name)
    M, mu = ph.numpy_mu(G, C)
    assert ph.gap_ok(mu, FMAX), "bad fixture: an eigenvalue within a factor 4 inside or 1e6 outside the cut"
    assert len(ph.kept(mu, FMAX)) == count
    r = ph.poles(G, C, FMAX)
    assert r["flags"] == 0 and r["n_poles"] == count
    ratio = ph.kept_ratio(r["mu"], M, mu, FMAX)
    print("%s: %d poles, largest difference / bound %.3g" % (name, count, ratio))
    assert ratio <= 1.0
    # the poles are the reciprocals of what was compared, dominant first
    s = r["poles"][:count]
    assert np.all(np.diff(np.abs(s)) >= 0.0) and r["n_rhp"] == 0 and r["max_re"] == s.real.max()
    assert np.allclose(np.sort_complex(1.0 / s), np.sort_complex(ph.kept(r["mu"], FMAX)), rtol=1e-14, atol=0.0)


# ---- 3. balancing ----------------------------------------------------------------------------------------------------

def _badly_scaled(n, seed):
    rng = np.random.default_rng(seed)
    d = 10.0 ** rng.integers(-6, 7, n)
    return rng.standard_normal((n, n)) * d[:, None] / d[None, :]


@pytest.mark.parametrize("which", ["dbmixer", "scaled5", "scaled33", "diag", "zero_row"])
def test_balancing_is_an_exact_power_of_two_similarity(which):
    if which == "dbmixer":
        M = ph.numpy_mu(*_system("dbmixer.sp")[1:])[0]
    elif which == "diag":
        M = np.diag([1.0, -2.0, 3e9])
    elif which == "zero_row":
        M = _badly_scaled(6, 3)
        M[2, :] = 0.0
    else:
        M = _badly_scaled(int(which[6:]), 20261021)
    a, d, sweeps = ph.balance(M)
    mant, _ = np.frexp(d)
    assert np.all(mant == 0.5) and np.all(d > 0.0)                      # every D_ii a power of two
    want = M / d[:, None] * d[None, :]
    normal = np.abs(M) > 1e-290                                         # entries that no factor can push into the denormals
    assert np.array_equal(a[normal], want[normal])                      # exact: scaling by powers of two rounds nothing
    assert np.all(np.abs(a[~normal]) < 1e-280)
    assert 0 <= sweeps < 16
    if which.startswith("scaled"):
        off = lambda m: (np.abs(m).sum(axis=0) - np.abs(np.diag(m)), np.abs(m).sum(axis=1) - np.abs(np.diag(m)))  # noqa: E731
        c, r = off(a)
        assert np.all(c <= 4.0 * r) and np.all(r <= 4.0 * c) and not np.array_equal(a, M)
    if which == "diag":
        assert sweeps == 0 and np.array_equal(a, M)


def test_hessenberg_form_keeps_the_spectrum():
    M = _badly_scaled(12, 7)
    h = ph.elmhes(M)
    assert np.all(np.tril(h, -2) == 0.0)
    assert np.allclose(np.sort_complex(np.linalg.eigvals(h)), np.sort_complex(np.linalg.eigvals(M)), rtol=1e-9)


# ---- 4. flags and structure ------------------------------------------------------------------------------------------

def test_flags_counts_and_order():
    s = pc.special()
    r = ph.poles_batch(s["G"], s["C"], s["fmax"])
    assert r["flags"].tolist() == s["want_flags"] == [ph.PZ_SINGULAR, 0, 0, 0]
    assert r["n_poles"].tolist() == s["want_n"] and r["n_rhp"].tolist() == s["want_rhp"]
    assert np.isnan(r["poles"][0].view(np.float64)).all() and np.isnan(r["max_re"][0])          # singular A0
    assert np.isnan(r["poles"][1].view(np.float64)).all() and np.isnan(r["max_re"][1])          # C = 0: no pole, no flag
    # the negative conductance: -(-1) / 1e-3 = +1000 beside the stable pole of the other branch
    assert abs(r["poles"][2][0] - 1000.0) <= ANALYTIC_ULPS * ULP * 1000.0 and r["poles"][2][1].real < 0.0
    assert r["max_re"][2] == r["poles"][2][0].real
    # order: dominant first
    assert np.all(np.diff(np.abs(r["poles"][3])) > 0.0) and r["max_re"][3] == r["poles"][3][0].real


def test_two_by_two_with_a_negative_conductance():
    G = np.array([[-1e-3, 0.0], [0.0, 2e-3]])
    C = np.diag([1e-9, 1e-9])
    r = ph.poles(G, C, 1e12)
    assert (r["flags"], r["n_poles"], r["n_rhp"]) == (0, 2, 1)
    assert abs(r["poles"][0] - 1e6) <= ANALYTIC_ULPS * ULP * 1e6 and abs(r["poles"][1] + 2e6) <= ANALYTIC_ULPS * ULP * 2e6
    assert r["max_re"] == r["poles"][0].real and r["poles"][0].imag == 0.0


def test_shift_recovers_the_pole_of_an_integrator():
    """G = 0, C = c: A0 = sigma0 C is regular for sigma0 != 0, mu = -1 / sigma0 and s = sigma0 + 1 / mu = 0.  Test 2's
    bound on mu is its floor here, N 2^-52 |mu| with N = 1, which is 2^-52 |sigma0| on s = sigma0 + mu / mu^2; that
    formula's own three roundings (the square, the quotient, the sum) add half an ulp of |sigma0| each: 2.5 ulp of
    |sigma0| in all.  Observed: 1.05 and 0.55 ulp."""
    for sigma0 in (-1e6, 3.7e3):
        r = ph.poles(np.zeros((1, 1)), np.array([[2.2e-9]]), 1e12, sigma0=sigma0)
        assert (r["flags"], r["n_poles"]) == (0, 1)
        print("sigma0 = %g: s = %.3g, %.2f ulp of |sigma0|" % (sigma0, r["poles"][0].real, abs(r["poles"][0]) / (ULP * abs(sigma0))))
        assert abs(r["poles"][0]) <= 2.5 * ULP * abs(sigma0)
    assert ph.poles(np.zeros((1, 1)), np.array([[2.2e-9]]), 1e12)["flags"] == ph.PZ_SINGULAR


def test_conjugate_pair_order_and_ties():
    """two pairs and a real pole: descending |mu|; within a pair Im mu > 0 first, so Im s < 0 first"""
    blocks = [np.array([[-1.0, 5.0], [-5.0, -1.0]]), np.array([[-30.0, 7.0], [-7.0, -30.0]]), np.array([[-4.0]])]
    n = 5
    A = np.zeros((n, n))
    A[0:2, 0:2], A[2:4, 2:4], A[4:, 4:] = blocks
    r = ph.poles(-A, np.eye(n), 1e3)                        # (G + s C) = s I - A: the poles are the eigenvalues of A
    assert (r["flags"], r["n_poles"], r["n_rhp"]) == (0, 5, 0)
    s = r["poles"]
    assert np.allclose(s, [-4.0, -1 - 5j, -1 + 5j, -30 - 7j, -30 + 7j], rtol=1e-14)
    assert s[1].real == s[2].real and s[1].imag == -s[2].imag and s[3].imag == -s[4].imag
    assert r["max_re"] == s[1].real


def test_the_cut_drops_what_lies_below_it():
    G = np.diag([1.0, 1.0, 1.0])
    C = np.diag([1e-3, 1e-6, 1e-9])                         # poles -1e3, -1e6, -1e9 rad/s
    for fmax, want in ((1e12, 3), (1e8 / (2 * np.pi), 2), (1e5 / (2 * np.pi), 1), (10.0, 0)):
        r = ph.poles(G, C, fmax)
        assert r["n_poles"] == want and r["flags"] == 0, fmax
        assert np.allclose(r["poles"][:want].real, [-1e3, -1e6, -1e9][:want], rtol=ANALYTIC_ULPS * ULP, atol=0.0)


def test_nonconvergence_is_flagged_and_bounded():
    """NaN entries never deflate: the iteration cap ends the routine with CSIM_ST_PZ_NONCONV and NaN slots"""
    M = np.full((4, 4), np.nan)
    fl, _ = ph.eig(M)
    assert fl == ph.PZ_NONCONV
    r = ph.poles(np.eye(4), M, 1e12)
    assert r["flags"] == ph.PZ_NONCONV and r["n_poles"] == 0 and np.isnan(r["poles"].view(np.float64)).all()


# ---- the fixtures of the GPU kernel tests ----------------------------------------------------------------------------

@pytest.mark.parametrize("n", pc.SIZES)
def test_kernel_fixtures_against_numpy(n):
    """what tests/test_pz_kernels_gpu.py compares the kernel with, held against numpy by the bound of test 2"""
    c, ref = pc.case(n), pc.reference(n)
    worst = 0.0
    for b in range(0, pc.NB, 8):
        r = ph.poles(c["G"][b], c["C"][b], c["fmax"])
        assert r["flags"] == 0 and r["n_poles"] == ref["n_poles"][b] == len(ph.kept(c["mu"][b], c["fmax"]))
        worst = max(worst, ph.kept_ratio(r["mu"], c["M"][b], c["mu"][b], c["fmax"]))
    print("n = %d: largest difference / bound %.3g" % (n, worst))
    assert worst <= 1.0


def test_status_bits_of_the_header():
    import re
    text = open(netlist_path("../../include/csim_ir.h")).read()
    bits = dict(re.findall(r"#define (CSIM_ST_PZ_\w+)\s+(0x[0-9a-fA-F]+)u", text))
    assert {k: int(v, 16) for k, v in bits.items()} == {"CSIM_ST_PZ_SINGULAR": 0x1000, "CSIM_ST_PZ_NONCONV": 0x2000}
