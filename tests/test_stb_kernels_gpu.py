"""The loop-gain kernels (kernels_stb.hip: one wavefront per system in LDS, N <= 63; 32 lanes per system in registers,
N <= 32; the margins kernel) fed directly through csim_stb_solve_batch and compared with tests/stb_reference.py, the
specification of include/csim.h "Loop-gain analysis" restated in numpy (which tests/test_stb_cpu.py in turn holds
against the host-compiled ac_stb.hpp, on these same inputs): T and the two solutions bit for bit, the margins within
stb_cases.MARGIN_BOUND (the device's atan2 / log10 / log / exp are not numpy's), the crossings found exactly.

Inputs: tests/stb_cases.py -- n in {3, 5, 31, 32, 33, 63}, a batch of 3 (the packed kernel's half-empty last
wavefront), four frequencies with w = 0 among them; the chain of three equal poles; the LC tank that is singular at
exactly one frequency; the loop whose den is exactly zero.

Singular inputs are ordinary data for these kernels: only arithmetic results depend on them, never an address or a
loop bound.  The probe's equations, which do index LDS, are checked on the host before a launch.  Nothing here
provokes a fault.
"""
import numpy as np
import pytest

import stb_cases as sc
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

KEYS = list(sc.SIZES) + ["chain", "tank", "zero_den"]


def _kernels(n):
    return ("wave", "packed") if n <= 32 else ("wave",)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(c, omega, kernel, nb=None, **kw):
    from circuitsimulator_amd import stb_solve_batch
    nb = len(c["G"]) if nb is None else nb
    return stb_solve_batch(c["G"][:nb], c["C"][:nb], c["probe"], omega, kernel=kernel, **kw)


def _margins(r):
    return np.stack([r["pm"], r["fc"], r["gm"], r["f180"]], axis=1)


@pytest.mark.parametrize("key", KEYS, ids=[str(k) for k in KEYS])
def test_kernels_equal_reference(key):
    """Measured on the GPU: the largest deviation of the device's margins from the reference over all cases is printed
    below (stb_cases.MARGIN_BOUND says how it is bounded); T, x, flags and found are exact."""
    c, omega, fhz = sc.inputs(key)
    n, nb = c["n"], len(c["G"])
    ref = sc.reference(key)
    want_t = np.stack([r["t"] for r in ref])
    want_x = np.stack([r["x"] for r in ref])
    want_m = np.stack([r["margins"] for r in ref])
    want_found = [r["found"] for r in ref]
    want_flags = [r["flags"] for r in ref]
    assert not np.isnan(want_x.view(np.float64)).any()
    got, worst = {}, 0.0
    for kernel in _kernels(n):
        r = got[kernel] = _run(c, omega, kernel, freqs=fhz)
        assert r["t"].shape == (nb, len(omega)) and r["x"].shape == (nb, len(omega), 2, n)
        assert r["flags"].tolist() == want_flags, (key, kernel)
        assert np.array_equal(_bits(r["t"]), _bits(want_t)), (key, kernel)
        assert np.array_equal(_bits(r["x"]), _bits(want_x)), (key, kernel)
        assert r["found"].tolist() == want_found, (key, kernel)
        worst = max(worst, sc.margins_close(_margins(r), want_m))
    print("%s: margins of the device against numpy: largest deviation %.3e" % (key, worst))
    if "packed" in got:
        for k in ("t", "x", "flags", "found", "pm", "fc", "gm", "f180"):
            assert np.array_equal(got["wave"][k].view(np.uint8), got["packed"][k].view(np.uint8)), (key, k)
    # without the solutions and without margins: the same T
    auto = _run(c, omega, "auto", want_x=False)
    assert auto["x"] is None and auto["pm"] is None and auto["found"] is None
    assert np.array_equal(_bits(auto["t"]), _bits(want_t))
    # a batch of one and of two: the same instances, the same bits
    for k in (1, 2):
        if k <= nb:
            r = _run(c, omega, _kernels(n)[-1], nb=k, freqs=fhz)
            assert np.array_equal(_bits(r["t"]), _bits(want_t[:k])) and np.array_equal(_bits(r["x"]), _bits(want_x[:k]))
            assert r["found"].tolist() == want_found[:k]


@pytest.mark.parametrize("kernel", ["wave", "packed"])
def test_tank_and_zero_den_zero_t_and_flag_it(kernel):
    c, omega, fhz = sc.inputs("tank")
    r = _run(c, omega, kernel, freqs=fhz)
    assert int(r["flags"][0]) == 4 and int(r["found"][0]) == 0 and np.isnan(_margins(r)).all()
    for f, fails in enumerate(sc.TANK_FAILS):
        v = np.concatenate([r["t"][0, f:f + 1].view(np.float64), r["x"][0, f].view(np.float64).ravel()])
        assert (np.all(v == 0) and not np.signbit(v).any()) if fails else r["t"][0, f] != 0, (kernel, f)
        one = _run(c, omega[f:f + 1], kernel)                 # frequency by frequency the flag is set where A fails
        assert int(one["flags"][0]) == (4 if fails else 0), (kernel, f)
    c, omega, fhz = sc.inputs("zero_den")
    r = _run(c, omega, kernel, freqs=fhz)
    v = r["t"].view(np.float64)
    assert int(r["flags"][0]) == 4 and np.all(v == 0) and not np.signbit(v).any()
    assert np.all(r["x"][0, :, 0, :2] == [1.5, 0.5]) and np.all(r["x"][0, :, 1, 2] == 0.5)   # the solutions are there


def test_a_singular_neighbour_leaves_the_others_alone():
    c, omega, fhz = sc.inputs(5)
    ref = sc.reference(5)
    G = c["G"].copy()
    G[1] = 0.0
    C = c["C"].copy()
    C[1] = 0.0
    for kernel in ("wave", "packed"):
        r = _run(dict(c, G=G, C=C), omega, kernel, freqs=fhz)
        assert r["flags"].tolist() == [0, 4, 0] and int(r["found"][1]) == 0
        v = np.concatenate([r["t"][1].view(np.float64), r["x"][1].view(np.float64).ravel()])
        assert np.all(v == 0) and not np.signbit(v).any()
        for b in (0, 2):
            assert np.array_equal(_bits(r["t"][b]), _bits(ref[b]["t"])) and np.array_equal(_bits(r["x"][b]), _bits(ref[b]["x"]))
            assert int(r["found"][b]) == ref[b]["found"]


@pytest.mark.parametrize("n,kernel", [(64, "wave"), (64, "packed"), (64, "auto"), (33, "packed"), (5, "block")])
def test_sizes_and_kernels_beyond_the_analysis_are_refused(n, kernel):
    from circuitsimulator_amd import CsimError, capi, stb_solve_batch
    G = np.eye(n)[None]
    with pytest.raises(CsimError) as e:
        stb_solve_batch(G, np.zeros_like(G), (0, 1, 2), sc.OMEGA, kernel=kernel)
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED


def test_margins_with_a_grid_that_does_not_increase_are_refused():
    from circuitsimulator_amd import CsimError, capi, stb_solve_batch
    c, omega, _ = sc.inputs(5)
    for bad in ([0.0, 1.0, 2.0, 3.0], [1.0, 2.0, 2.0, 3.0], [4.0, 3.0, 2.0, 1.0]):
        with pytest.raises(CsimError) as e:
            stb_solve_batch(c["G"], c["C"], c["probe"], omega, freqs=bad)
        assert e.value.code == capi.CSIM_ERR_ARG
