"""The two distortion kernels (kernels_disto.hip: one wavefront per system in LDS, N <= 63; 32 lanes per system in
registers, N <= 32) fed directly through csim_disto_solve_batch and compared bit for bit with
tests/disto_reference.py, the specification of include/csim.h "Distortion analysis" restated in numpy (which
tests/test_disto_cpu.py in turn holds against the host-compiled ac_disto_solve(), on these same inputs).

Inputs: tests/disto_cases.py -- n in {1, 2, 5, 31, 32, 33, 63}, a batch of 3 (the packed kernel's half-empty last
wavefront), four frequencies with w = 0 among them, 0, 1, 3 and 65 devices with grounded terminals, d == s and g == d;
and the LC tank that is singular exactly where k w == 1, so that each order fails once.

Singular inputs are ordinary data for these kernels: only arithmetic results depend on them, never an address or a
loop bound.  The equation indices that do index LDS (output, device terminals) are checked on the host before a
launch.  Nothing here provokes a fault.
"""
import numpy as np
import pytest

import disto_cases as dc
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def _kernels(n):
    return ("wave", "packed") if n <= 32 else ("wave",)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(c, omega, kernel, nb=None, **kw):
    from circuitsimulator_amd import disto_solve_batch
    nb = len(c["G"]) if nb is None else nb
    return disto_solve_batch(c["G"][:nb], c["C"][:nb], c["J"][:nb], c["dev_d"], c["dev_g"], c["dev_s"], c["coef"][:nb],
                             c["out"], omega, kernel=kernel, **kw)


@pytest.mark.parametrize("n,M", dc.CASES, ids=["n%d-M%d" % c for c in dc.CASES])
def test_kernels_equal_reference_bitwise(n, M):
    c = dc.case(n, M)
    ref = dc.reference((n, M))
    want_h = np.stack([r["h"] for r in ref])
    want_hd = np.stack([r["hd"] for r in ref])
    assert not np.isnan(want_h.view(np.float64)).any() and all(r["flags"] == 0 for r in ref)
    got = {}
    for kernel in _kernels(n):
        r = got[kernel] = _run(c, dc.OMEGA, kernel)
        assert r["h"].shape == (dc.B, len(dc.OMEGA), 3, n) and r["hd"].shape == (dc.B, len(dc.OMEGA), 2)
        assert np.all(r["flags"] == 0), (n, M, kernel)
        assert np.array_equal(_bits(r["h"]), _bits(want_h)), (n, M, kernel)
        assert np.array_equal(_bits(r["hd"]), _bits(want_hd)), (n, M, kernel)
    if "packed" in got:
        for k in ("h", "hd", "flags"):
            assert np.array_equal(got["wave"][k].view(np.uint8), got["packed"][k].view(np.uint8)), (n, M, k)
    auto = _run(c, dc.OMEGA, "auto", want_h=False)
    assert auto["h"] is None and np.array_equal(_bits(auto["hd"]), _bits(want_hd))
    # a batch of one and of two: the same instances, the same bits
    for nb in (1, 2):
        r = _run(c, dc.OMEGA, _kernels(n)[-1], nb=nb)
        assert np.array_equal(_bits(r["h"]), _bits(want_h[:nb])) and np.array_equal(_bits(r["hd"]), _bits(want_hd[:nb]))


@pytest.mark.parametrize("kernel", ["wave", "packed"])
def test_tank_zeroes_the_failed_order_and_every_higher_one(kernel):
    c = dc.tank()
    ref, = dc.reference("tank")
    r = _run(c, dc.TANK_OMEGA, kernel)
    assert int(r["flags"][0]) == 4
    assert np.array_equal(_bits(r["h"][0]), _bits(ref["h"])) and np.array_equal(_bits(r["hd"][0]), _bits(ref["hd"]))
    for f, first in enumerate(dc.TANK_FAILS_AT):
        for k in range(3):
            v = r["h"][0, f, k].view(np.float64)
            if first and k + 1 >= first:
                assert np.all(v == 0) and not np.signbit(v).any(), (kernel, f, k)
            else:
                assert np.any(v != 0), (kernel, f, k)
        assert not np.signbit(r["hd"][0, f]).any()
    # frequency by frequency the flag is set exactly where an order fails
    for f, first in enumerate(dc.TANK_FAILS_AT):
        one = _run(c, dc.TANK_OMEGA[f:f + 1], kernel)
        assert int(one["flags"][0]) == (4 if first else 0), (kernel, f)
        assert np.array_equal(_bits(one["h"][0, 0]), _bits(ref["h"][f]))
    # no device at all: the factorisations are still attempted, so the flags are the same
    bare = dict(c, M=0, dev_d=c["dev_d"][:0], dev_g=c["dev_g"][:0], dev_s=c["dev_s"][:0], coef=np.zeros((1, 0, 7)))
    for f, first in enumerate(dc.TANK_FAILS_AT):
        one = _run(bare, dc.TANK_OMEGA[f:f + 1], kernel)
        assert int(one["flags"][0]) == (4 if first else 0), (kernel, f)
        v = one["h"][0, 0, 1:].view(np.float64)
        assert np.all(v == 0) and not np.signbit(v).any() and np.all(one["hd"] == 0)


def test_a_singular_neighbour_leaves_the_others_alone():
    c = dc.case(5, 3)
    ref = dc.reference((5, 3))
    G = c["G"].copy()
    G[1] = 0.0
    C = c["C"].copy()
    C[1] = 0.0
    for kernel in ("wave", "packed"):
        r = _run(dict(c, G=G, C=C), dc.OMEGA, kernel)
        assert r["flags"].tolist() == [0, 4, 0]
        v = np.concatenate([r["h"][1].view(np.float64).ravel(), r["hd"][1].ravel()])
        assert np.all(v == 0) and not np.signbit(v).any()
        for b in (0, 2):
            assert np.array_equal(_bits(r["h"][b]), _bits(ref[b]["h"])) and np.array_equal(_bits(r["hd"][b]), _bits(ref[b]["hd"]))


@pytest.mark.parametrize("n,kernel", [(64, "wave"), (64, "packed"), (64, "auto"), (33, "packed"), (5, "block")])
def test_sizes_and_kernels_beyond_the_analysis_are_refused(n, kernel):
    from circuitsimulator_amd import CsimError, capi, disto_solve_batch
    G = np.eye(n)[None]
    with pytest.raises(CsimError) as e:
        disto_solve_batch(G, np.zeros_like(G), np.ones((1, n), dtype=complex), [0], [0], [-1], np.ones((1, 1, 7)), (0, -1),
                          dc.OMEGA, kernel=kernel)
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
