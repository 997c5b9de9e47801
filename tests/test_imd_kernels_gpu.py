"""The two intermodulation kernels (kernels_imd.hip: one wavefront per system in LDS, N <= 63; 32 lanes per system in
registers, N <= 32) fed directly through csim_imd_solve_batch and compared bit for bit with tests/imd_reference.py, the
specification of include/csim.h "Intermodulation analysis" restated in numpy (which tests/test_imd_cpu.py in turn holds
against the host-compiled ac_imd_solve(), on these same inputs, and against physics).

Inputs: tests/imd_cases.py -- the systems of tests/disto_cases.py (n in {1, 2, 5, 31, 32, 33, 63}, a batch of 3: the
packed kernel's half-empty last wavefront; 0, 1, 3 and 65 devices with grounded terminals, d == s and g == d), four tone
pairs with w2 = 0, w1 == w2 and w1 < w2 among them, a second excitation J2 != J1 on four of the cases; and the LC tank
that is singular exactly where w == 1, with six pairs that make each of the six solves the first to fail once.

Singular inputs are ordinary data for these kernels: only arithmetic results depend on them, never an address or a
loop bound.  The equation indices that do index LDS (output, device terminals) are checked on the host before a
launch.  Nothing here provokes a fault.
"""
import numpy as np
import pytest

import imd_cases as ic
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def _kernels(n):
    return ("wave", "packed") if n <= 32 else ("wave",)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(c, w1, w2, kernel, nb=None, J2=None, **kw):
    from circuitsimulator_amd import imd_solve_batch
    nb = len(c["G"]) if nb is None else nb
    return imd_solve_batch(c["G"][:nb], c["C"][:nb], c["J"][:nb], c["dev_d"], c["dev_g"], c["dev_s"], c["coef"][:nb],
                           c["out"], w1, w2, J2=None if J2 is None else J2[:nb], kernel=kernel, **kw)


@pytest.mark.parametrize("n,M", ic.CASES, ids=["n%d-M%d" % c for c in ic.CASES])
def test_kernels_equal_reference_bitwise(n, M):
    c = ic.case(n, M)
    ref = ic.reference((n, M))
    F = len(ic.OMEGA1)
    want_h = np.stack([r["h"] for r in ref])
    want_im = np.stack([r["im"] for r in ref])
    assert not np.isnan(want_h.view(np.float64)).any() and all(r["flags"] == 0 for r in ref)
    got = {}
    for kernel in _kernels(n):
        r = got[kernel] = _run(c, ic.OMEGA1, ic.OMEGA2, kernel)
        assert r["h"].shape == (ic.B, F, 6, n) and r["im"].shape == (ic.B, F, 3)
        assert np.all(r["flags"] == 0), (n, M, kernel)
        assert np.array_equal(_bits(r["h"]), _bits(want_h)), (n, M, kernel)
        assert np.array_equal(_bits(r["im"]), _bits(want_im)), (n, M, kernel)
    if "packed" in got:
        for k in ("h", "im", "flags"):
            assert np.array_equal(got["wave"][k].view(np.uint8), got["packed"][k].view(np.uint8)), (n, M, k)
    auto = _run(c, ic.OMEGA1, ic.OMEGA2, "auto", want_h=False)
    assert auto["h"] is None and np.array_equal(_bits(auto["im"]), _bits(want_im))
    # a batch of one and of two: the same instances, the same bits
    for nb in (1, 2):
        r = _run(c, ic.OMEGA1, ic.OMEGA2, _kernels(n)[-1], nb=nb)
        assert np.array_equal(_bits(r["h"]), _bits(want_h[:nb])) and np.array_equal(_bits(r["im"]), _bits(want_im[:nb]))


@pytest.mark.parametrize("n,M", ic.CASES, ids=["n%d-M%d" % c for c in ic.CASES])
def test_the_solves_shared_with_the_single_tone_chain_are_its_bits(n, M):
    """x0 (at w1, driven by J) and x4 (at 2.0 w1, driven by disto_i2 of x0) are the single-tone chain's x1 and x2 at
    w = w1: the same body computes both, so the bits are the same"""
    from circuitsimulator_amd import disto_solve_batch
    c = ic.case(n, M)
    for kernel in _kernels(n):
        two = _run(c, ic.OMEGA1, ic.OMEGA2, kernel)
        one = disto_solve_batch(c["G"], c["C"], c["J"], c["dev_d"], c["dev_g"], c["dev_s"], c["coef"], c["out"], ic.OMEGA1,
                                kernel=kernel)
        assert np.all(two["flags"] == 0) and np.all(one["flags"] == 0), (n, M, kernel)
        assert np.array_equal(_bits(two["h"][:, :, 0]), _bits(one["h"][:, :, 0])), (n, M, kernel)
        assert np.array_equal(_bits(two["h"][:, :, 4]), _bits(one["h"][:, :, 1])), (n, M, kernel)


@pytest.mark.parametrize("n,M", ic.J2_CASES, ids=["n%d-M%d" % c for c in ic.J2_CASES])
def test_a_second_excitation(n, M):
    c = ic.case(n, M)
    J2 = ic.second_excitation(n, M)
    ref = ic.reference((n, M, "j2"))
    want_h = np.stack([r["h"] for r in ref])
    want_im = np.stack([r["im"] for r in ref])
    same = np.stack([r["h"] for r in ic.reference((n, M))])
    assert not np.array_equal(want_h[:, :, 1], same[:, :, 1]) and np.array_equal(_bits(want_h[:, :, 0]), _bits(same[:, :, 0]))
    for kernel in _kernels(n):
        r = _run(c, ic.OMEGA1, ic.OMEGA2, kernel, J2=J2)
        assert np.all(r["flags"] == 0)
        assert np.array_equal(_bits(r["h"]), _bits(want_h)), (n, M, kernel)
        assert np.array_equal(_bits(r["im"]), _bits(want_im)), (n, M, kernel)
        # J2 given as a copy of J is J2 left out
        r = _run(c, ic.OMEGA1, ic.OMEGA2, kernel, J2=c["J"].copy(), nb=2)
        assert np.array_equal(_bits(r["h"]), _bits(same[:2])), (n, M, kernel)


@pytest.mark.parametrize("kernel", ["wave", "packed"])
def test_tank_zeroes_the_failed_solve_and_every_later_one(kernel):
    c = ic.tank()
    ref, = ic.reference("tank")
    r = _run(c, ic.TANK_OMEGA1, ic.TANK_OMEGA2, kernel)
    assert int(r["flags"][0]) == 4
    assert np.array_equal(_bits(r["h"][0]), _bits(ref["h"])) and np.array_equal(_bits(r["im"][0]), _bits(ref["im"]))
    for f, first in enumerate(ic.TANK_FAILS_AT):
        assert [k for k in range(6) if ref["per_f"][f][k]][0] == first
        for k in range(6):
            v = r["h"][0, f, k].view(np.float64)
            if k >= first:
                assert np.all(v == 0) and not np.signbit(v).any(), (kernel, f, k)
            else:
                assert np.any(v != 0), (kernel, f, k)
        assert not np.signbit(r["im"][0, f]).any()
    # pair by pair the flag is set exactly where a solve fails; a regular pair beside them is not flagged
    for f in range(len(ic.TANK_FAILS_AT)):
        one = _run(c, ic.TANK_OMEGA1[f:f + 1], ic.TANK_OMEGA2[f:f + 1], kernel)
        assert int(one["flags"][0]) == 4, (kernel, f)
        assert np.array_equal(_bits(one["h"][0, 0]), _bits(ref["h"][f]))
    clean = _run(c, [0.375], [0.125], kernel)                 # 0.375, 0.125, 0.5, 0.25, 0.75, 0.625: none is 1
    assert int(clean["flags"][0]) == 0 and np.all(np.any(clean["h"][0, 0] != 0, axis=-1)) and np.all(clean["im"] > 0)
    # no device at all: the factorisations are still attempted, so the flags are the same
    bare = dict(c, M=0, dev_d=c["dev_d"][:0], dev_g=c["dev_g"][:0], dev_s=c["dev_s"][:0], coef=np.zeros((1, 0, 7)))
    for f, first in enumerate(ic.TANK_FAILS_AT):
        one = _run(bare, ic.TANK_OMEGA1[f:f + 1], ic.TANK_OMEGA2[f:f + 1], kernel)
        assert int(one["flags"][0]) == 4, (kernel, f)
        v = one["h"][0, 0, 2:].view(np.float64)
        assert np.all(v == 0) and not np.signbit(v).any() and np.all(one["im"] == 0)
        assert np.array_equal(_bits(one["h"][0, 0, :2]), _bits(ref["h"][f, :2]))
    assert int(_run(bare, [0.375], [0.125], kernel)["flags"][0]) == 0


def test_a_singular_neighbour_leaves_the_others_alone():
    c = ic.case(5, 3)
    ref = ic.reference((5, 3))
    G = c["G"].copy()
    G[1] = 0.0
    C = c["C"].copy()
    C[1] = 0.0
    for kernel in ("wave", "packed"):
        r = _run(dict(c, G=G, C=C), ic.OMEGA1, ic.OMEGA2, kernel)
        assert r["flags"].tolist() == [0, 4, 0]
        v = np.concatenate([r["h"][1].view(np.float64).ravel(), r["im"][1].ravel()])
        assert np.all(v == 0) and not np.signbit(v).any()
        for b in (0, 2):
            assert np.array_equal(_bits(r["h"][b]), _bits(ref[b]["h"])) and np.array_equal(_bits(r["im"][b]), _bits(ref[b]["im"]))


@pytest.mark.parametrize("n,kernel", [(64, "wave"), (64, "packed"), (64, "auto"), (33, "packed"), (5, "block")])
def test_sizes_and_kernels_beyond_the_analysis_are_refused(n, kernel):
    from circuitsimulator_amd import CsimError, capi, imd_solve_batch
    G = np.eye(n)[None]
    with pytest.raises(CsimError) as e:
        imd_solve_batch(G, np.zeros_like(G), np.ones((1, n), dtype=complex), [0], [0], [-1], np.ones((1, 1, 7)), (0, -1),
                        ic.OMEGA1, ic.OMEGA2, kernel=kernel)
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED


@pytest.mark.parametrize("change", [dict(out=(5, -1)), dict(out=(0, 5)), dict(out=(-1, 0)), dict(out=(2, 2)), dict(dev_d=[5]),
                                    dict(dev_g=[-2]), dict(dev_s=[7])], ids=str)
def test_equations_out_of_range_are_refused_without_a_launch(change):
    from circuitsimulator_amd import CsimError, capi, imd_solve_batch
    a = dict(dev_d=[0], dev_g=[1], dev_s=[-1], out=(0, -1))
    a.update(change)
    G = np.eye(5)[None]
    with pytest.raises(CsimError) as e:
        imd_solve_batch(G, np.zeros_like(G), np.ones((1, 5), dtype=complex), a["dev_d"], a["dev_g"], a["dev_s"],
                        np.ones((1, 1, 7)), a["out"], [1.0], [0.5])
    assert e.value.code == capi.CSIM_ERR_ARG
