"""The two two-port noise kernels (kernels_spnoise.hip: one wavefront per system in LDS, N <= 63; 32 lanes per system in
registers, N <= 32) fed directly through csim_spnoise_solve_batch and compared bit for bit with
tests/spnoise_reference.py, the specification of include/csim.h "Two-port noise analysis" restated in numpy (which
tests/test_spnoise_cpu.py in turn holds against the host-compiled ac_port_noise.hpp, on these same inputs).

Inputs: tests/spnoise_cases.py -- the systems of tests/ac_cases.py at both sides of every size boundary, P = 1 .. 4
ports, generator tables of 0 .. 65 entries, batches of 1 and 3 (an odd batch leaves the second half of the last packed
wavefront empty).

NaN and singular inputs are ordinary data for these kernels, as for their siblings: only arithmetic results depend on
them, never an address or a loop bound.  Port equations and generator terminals index LDS and are range-checked on the
host.
"""
import numpy as np
import pytest

import ac_cases as cs
import spnoise_cases as spc
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def _kernels(n):
    return ("wave", "packed") if n <= 32 else ("wave",)


def _same(x, ref, nan_expected, where):
    """bitwise equality; where NaNs are expected: equal NaN masks, bitwise equality elsewhere"""
    x, ref = np.ascontiguousarray(x), np.ascontiguousarray(ref)
    xb, rb = x.view(np.uint64), ref.view(np.uint64)
    if not nan_expected:
        assert not np.isnan(ref.view(np.float64)).any(), where
        assert np.array_equal(xb, rb), where
        return
    nx, nr = np.isnan(x.view(np.float64)), np.isnan(ref.view(np.float64))
    assert np.array_equal(nx, nr), where
    assert np.array_equal(np.where(nx, 0, xb), np.where(nr, 0, rb)), where


def _run(c, B, kernel, sel=None):
    from circuitsimulator_amd import sp_noise_solve_batch
    sel = slice(0, B) if sel is None else sel
    return sp_noise_solve_batch(c["G"][sel], c["C"][sel], c["port_eq"], c["z0"], c["src_a"], c["src_b"], c["psd"][sel],
                                cs.OMEGA, kernel=kernel)


@pytest.mark.parametrize("n", spc.SIZES)
def test_kernels_equal_reference_bitwise(n):
    """both kernels, every kind, batches of 1 and 3: flags, adjoint solutions, Y, Cy and the noise parameters; the
    "auto" choice is the packed kernel up to n = 32 and the wave kernel above"""
    launches = flagged = 0
    for c in spc.all_cases(sizes=(n,)):
        kind, P = c["kind"], c["P"]
        ref = spc.reference(c)
        want_fl = np.array([r["flags"] for r in ref], dtype=np.uint32)
        flagged += int(np.count_nonzero(want_fl))
        out = {}
        for kernel in _kernels(n) + ("auto",):
            for B in spc.BATCHES:
                r = _run(c, B, kernel)
                launches += 1
                where = (kind, n, P, c["S"], kernel, B)
                assert np.array_equal(r["flags"], want_fl[:B]), where + (r["flags"].tolist(), want_fl[:B].tolist())
                assert set(spc.keys(P)) | {"flags"} == set(r), where
                for key in spc.keys(P):                         # Y21 == 0 gets IEEE's answer: NaN parameters from finite data
                    _same(r[key], np.stack([ref[s][key] for s in range(B)]), kind in cs.HAS_NAN or key in spc.KEYS2,
                          where + (key,))
                out[kernel, B] = r
        for B in spc.BATCHES:
            for key in spc.keys(P):
                _same(out["auto", B][key], out["packed" if n <= 32 else "wave", B][key], True, (kind, n, "auto", key))
    print("n = %d: %d launches, %d flagged systems" % (n, launches, flagged))
    assert flagged > 0


@pytest.mark.parametrize("n", [2, 9, 32, 33, 63])
def test_singular_neighbour_leaves_the_others_alone(n):
    """a batch of five with system 2 singular: its outputs are all +0.0, systems 0, 1, 3, 4 equal their solo results
    bit for bit"""
    good, bad = spc.case("dense", n), spc.case("sing_mid", n)
    c = dict(good)
    c["G"], c["C"] = good["G"].copy(), good["C"].copy()
    c["G"][2], c["C"][2] = bad["G"][0], bad["C"][0]
    for kernel in _kernels(n):
        r = _run(c, 5, kernel)
        assert r["flags"].tolist() == [0, 0, 4, 0, 0], (n, kernel)
        for key in spc.keys(c["P"]):
            v = np.ascontiguousarray(r[key][2]).view(np.float64)
            assert np.all(v == 0) and not np.signbit(v).any(), (n, kernel, key)
        for s in (0, 1, 3, 4):
            solo = _run(c, 1, kernel, slice(s, s + 1))
            assert int(solo["flags"][0]) == 0
            for key in spc.keys(c["P"]):
                _same(solo[key][0], r[key][s], True, (n, kernel, s, key))


def test_outputs_are_optional_and_x_is_the_adjoint():
    """without x and the noise parameters the rest is unchanged; row i of x solves A^T x = e_{k_i}"""
    from circuitsimulator_amd import sp_noise_solve_batch
    c = spc.case("reversed", 9)
    full = sp_noise_solve_batch(c["G"], c["C"], [0, 8], [50.0, 75.0], c["src_a"], c["src_b"], c["psd"], cs.OMEGA)
    bare = sp_noise_solve_batch(c["G"], c["C"], [0, 8], [50.0, 75.0], c["src_a"], c["src_b"], c["psd"], cs.OMEGA,
                                noise_params=False, want_x=False)
    assert bare["x"] is None and "nf" not in bare and "nf" in full
    for key in ("y", "cy"):
        assert np.array_equal(full[key].view(np.uint64), bare[key].view(np.uint64)), key
    A = c["G"][0] + 1j * cs.OMEGA[0] * c["C"][0]
    e = np.zeros(9)
    e[8] = 1.0
    assert np.allclose(A.T @ full["x"][0, 0, 1], e, atol=1e-12)


def test_arguments_are_checked():
    from circuitsimulator_amd import CsimError, capi, sp_noise_solve_batch
    c = spc.case("dense", 9)
    ok = dict(port_eq=[0, 8], z0=[50.0, 50.0], src_a=[0, -1], src_b=[-1, 8])

    def call(n=9, kernel="auto", **kw):
        a = dict(ok, **kw)
        G = c["G"] if n == 9 else np.eye(n)[None]
        Cm = c["C"] if n == 9 else np.zeros((1, n, n))
        return sp_noise_solve_batch(G, Cm, a["port_eq"], a["z0"], a["src_a"], a["src_b"],
                                    np.ones((G.shape[0], len(a["src_a"]))), cs.OMEGA, kernel=kernel)
    assert call()["cy"].shape == (cs.NSYS, len(cs.OMEGA), 2, 2)
    for kw in (dict(port_eq=[0, 9]), dict(port_eq=[-1, 0]), dict(z0=[0.0, 50.0]), dict(z0=[50.0, float("inf")]),
               dict(src_a=[9, 0]), dict(src_b=[0, -2]), dict(port_eq=[0, 1, 2, 3, 4], z0=[50.0] * 5)):
        with pytest.raises(CsimError) as e:
            call(**kw)
        assert e.value.code == capi.CSIM_ERR_ARG, kw
    for n, kernel in ((64, "wave"), (64, "auto"), (33, "packed")):
        with pytest.raises(CsimError) as e:
            call(n=n, kernel=kernel)
        assert e.value.code == capi.CSIM_ERR_UNSUPPORTED, (n, kernel)
    assert call(n=33, kernel="wave")["cy"].shape == (1, len(cs.OMEGA), 2, 2)
    # the library's own answer to noise parameters with one port (the Python wrapper refuses earlier, with a ValueError)
    one = np.zeros(1)
    pe, z0 = np.array([0], dtype=np.int32), np.array([50.0])
    cy = np.zeros((1, 1, 1, 1), dtype=np.complex128)
    G, Cm, om = np.eye(2), np.zeros((2, 2)), np.array([1.0])
    rc = capi.lib().csim_spnoise_solve_batch(0, 2, 1, 1, G.ctypes.data, Cm.ctypes.data, pe.ctypes.data, z0.ctypes.data, 0, None,
                                             None, None, om.ctypes.data, 1, 0, None, cy.ctypes.data, one.ctypes.data, None,
                                             None, None, None, None)
    assert rc == capi.CSIM_ERR_CONFIG
