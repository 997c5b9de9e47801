"""The pole kernel (kernels_pz.hip: one wavefront per instance, everything in LDS) fed directly through
csim_pz_solve_batch and compared bit for bit with the host-compiled statement of engine/pz.hpp (tests/pz_host.py, which
tests/test_pz_cpu.py in turn holds against numpy): poles, counts, max_re and flags.

Inputs: tests/pz_cases.py -- n in {1, 2, 3, 31, 32, 33, 63}, batches of 1, 2 and 65, seeded G and rank-deficient C; the
singular, C = 0 and right-half-plane systems.

Singular inputs are ordinary data for this kernel: only arithmetic results depend on them, never an address; every
loop has a fixed cap (16 balancing sweeps, 30 QR iterations per eigenvalue).  Nothing here provokes a fault.
"""
import numpy as np
import pytest

import pz_cases as pc
import pz_host as ph
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def _same(got, want, what):
    """bit for bit, NaN slots as NaN slots"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    g, w = got.view(np.float64), want.view(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    ok = ~np.isnan(w)
    assert np.array_equal(g[ok].view(np.uint64), w[ok].view(np.uint64)), what


def _compare(r, ref, nb, what):
    assert r["flags"].tolist() == ref["flags"][:nb].tolist(), what
    assert r["n_poles"].tolist() == ref["n_poles"][:nb].tolist(), what
    assert r["n_rhp"].tolist() == ref["n_rhp"][:nb].tolist(), what
    _same(r["max_re"], ref["max_re"][:nb], what)
    _same(r["poles"], ref["poles"][:nb], what)


@pytest.mark.parametrize("n", pc.SIZES)
def test_kernel_equals_the_host_statement(n):
    from circuitsimulator_amd import pz_solve_batch
    c, ref = pc.case(n), pc.reference(n)
    assert not ref["flags"].any()
    # the fixture does what it is for: every instance has poles and eigenvalues the cut drops (n = 1: poles only)
    assert (ref["n_poles"] == (n + 1) // 2).all()
    for nb in pc.BATCHES:
        r = pz_solve_batch(c["G"][:nb], c["C"][:nb], c["fmax"])
        assert r["poles"].shape == (nb, n)
        _compare(r, ref, nb, (n, nb))


@pytest.mark.parametrize("n", (3, 33))
def test_kernel_with_a_shift(n):
    """sigma0 != 0 goes through pz_shift and the pole formula: the same comparison"""
    from circuitsimulator_amd import pz_solve_batch
    c = pc.case(n)
    ref = ph.poles_batch(c["G"][:2], c["C"][:2], c["fmax"], sigma0=-1e8)
    assert not ref["flags"].any() and ref["n_poles"].all()
    _compare(pz_solve_batch(c["G"][:2], c["C"][:2], c["fmax"], sigma0=-1e8), ref, 2, n)


def test_singular_empty_and_right_half_plane():
    from circuitsimulator_amd import pz_solve_batch
    s = pc.special()
    ref = ph.poles_batch(s["G"], s["C"], s["fmax"])
    assert ref["flags"].tolist() == s["want_flags"] and ref["n_poles"].tolist() == s["want_n"]
    r = pz_solve_batch(s["G"], s["C"], s["fmax"])
    _compare(r, ref, 4, "special")
    assert r["n_rhp"].tolist() == s["want_rhp"]
    assert np.isnan(r["poles"][0].view(np.float64)).all() and np.isnan(r["max_re"][:2]).all()
    assert r["max_re"][2] > 0.0 and r["max_re"][3] < 0.0


def test_results_do_not_depend_on_the_batch():
    from circuitsimulator_amd import pz_solve_batch
    c = pc.case(32)
    whole = pz_solve_batch(c["G"], c["C"], c["fmax"])
    for b in (0, 17, 64):
        one = pz_solve_batch(c["G"][b:b + 1], c["C"][b:b + 1], c["fmax"])
        for k in ("poles", "n_poles", "n_rhp", "max_re", "flags"):
            assert np.array_equal(one[k].view(np.uint8), whole[k][b:b + 1].view(np.uint8)), (b, k)


def test_refusals_of_the_engine_free_entry():
    from circuitsimulator_amd import capi, pz_solve_batch
    G = np.eye(2)[None]
    for fmax, sigma0 in ((0.0, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1e6, float("inf"))):
        with pytest.raises(capi.CsimError) as e:
            pz_solve_batch(G, G, fmax, sigma0)
        assert e.value.code == capi.CSIM_ERR_ARG
    big = np.zeros((1, 64, 64))
    with pytest.raises(capi.CsimError) as e:
        pz_solve_batch(big, big, 0.0)                         # the bad argument first
    assert e.value.code == capi.CSIM_ERR_ARG
    with pytest.raises(capi.CsimError) as e:
        pz_solve_batch(big, big, 1e6)
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
    r = pz_solve_batch(np.zeros((0, 2, 2)), np.zeros((0, 2, 2)), 1e6)
    assert r["poles"].shape == (0, 2)
