"""The two noise kernels (kernels_noise.hip: one wavefront per system in LDS, N <= 63; 32 lanes per system in
registers, N <= 32) fed directly through csim_noise_solve_batch and compared bit for bit with
tests/noise_reference.py, the specification of include/csim.h "Noise analysis" restated in numpy (which
tests/test_noise_cpu.py in turn holds against the host-compiled ac_noise_solve(), on these same inputs).

Inputs: the systems of tests/ac_cases.py, transposed (noise_reference.adjoint_case: the solve factors A^T, so the
structured kinds meet their ties, zero columns, thresholds and NaNs where the AC solve does) -- every n from 1 to 63, batches of 1, 2, 3 and 5, three frequencies with
w = 0 among them, every kind -- with the seeded output pairs, generator tables (0 .. 3n generators, ground
terminals, a == b) and gain inputs of noise_reference.setup().

NaN and singular inputs are ordinary data for these kernels: only arithmetic results depend on them, never an
address or a loop bound.  The equation indices that do index LDS (output, generator terminals, gain input) are
checked on the host before a launch.  Nothing here provokes a fault.
"""
import numpy as np
import pytest

import ac_cases as cs
import noise_reference as nref
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

KEYS = ("onoise", "contrib", "gain", "y")


def _kernels(n):
    return ("wave", "packed") if n <= 32 else ("wave",)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(x, ref, nan_expected, where):
    """bitwise equality; where NaNs are expected: equal NaN masks, bitwise equality elsewhere"""
    x, ref = np.ascontiguousarray(x), np.ascontiguousarray(ref)
    assert x.shape == ref.shape, where + (x.shape, ref.shape)
    if not nan_expected:
        assert not np.isnan(ref.view(np.float64)).any(), where
        assert np.array_equal(_bits(x), _bits(ref)), where
        return
    nx, nr = np.isnan(x.view(np.float64)), np.isnan(ref.view(np.float64))
    assert np.array_equal(nx, nr), where
    assert np.array_equal(np.where(nx, 0, _bits(x)), np.where(nr, 0, _bits(ref))), where


def _reference(c, st):
    """-> dict(flags [5], onoise [5][F], contrib [5][F][S], gain [5][F], y [5][F][n], per_f, logs)"""
    res = [nref.solve_sweep(c["G"][s], c["C"][s], cs.OMEGA, st["out"], st["src_a"], st["src_b"], st["psd"][s],
                            st["gain_in"]) for s in range(cs.NSYS)]
    out = {k: np.stack([r[k] for r in res]) for k in KEYS}
    out["flags"] = np.array([r["flags"] for r in res], dtype=np.uint32)
    out["per_f"] = [r["per_f"] for r in res]
    out["logs"] = [r["logs"] for r in res]
    return out


def _run(c, st, B, kernel):
    from circuitsimulator_amd import noise_solve_batch
    return noise_solve_batch(c["G"][:B], c["C"][:B], st["out"], st["src_a"], st["src_b"], st["psd"][:B], cs.OMEGA,
                             gain_in=st["gain_in"], kernel=kernel)


@pytest.mark.parametrize("cls", range(len(cs.SIZE_CLASSES)), ids=["n<=%d" % hi for _, hi in cs.SIZE_CLASSES])
def test_kernels_equal_reference_bitwise(cls):
    lo, hi = cs.SIZE_CLASSES[cls]
    cov = cs.Coverage()
    launches = 0
    for c in map(nref.adjoint_case, cs.all_cases(sizes=range(lo, hi + 1))):
        n, kind = c["n"], c["kind"]
        st = nref.setup(cs.KINDS.index(kind), n)
        ref = _reference(c, st)
        for s in range(cs.NSYS):
            cov.add(n, ref["logs"][s])
        for kernel in _kernels(n):
            for B in cs.BATCHES:
                r = _run(c, st, B, kernel)
                launches += 1
                where = (kind, n, kernel, B)
                assert np.array_equal(r["flags"], ref["flags"][:B]), where + (r["flags"].tolist(), ref["flags"][:B].tolist())
                for k in KEYS:
                    _same(r[k], ref[k][:B], kind in cs.HAS_NAN, where + (k,))
    print("size class n<=%d: %d launches; systems that swapped in >= n/2 columns %d, took the first of tied rows %d, "
          "skipped a zero multiplier %d" % (hi, launches, cov.swaps[cls], cov.ties[cls], cov.skips[cls]))
    assert cov.swaps[cls] > 0 and cov.ties[cls] > 0 and cov.skips[cls] > 0, str(cov)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 16, 17, 23, 24, 25, 31, 32, 33, 48, 63])
def test_singular_neighbour_leaves_the_others_alone(n):
    """a batch of five with system 2 singular: systems 0, 1, 3, 4 equal their solo results bit for bit"""
    from circuitsimulator_amd import noise_solve_batch
    good, bad = nref.adjoint_case(cs.case("dense", n)), nref.adjoint_case(cs.case("sing_mid", n))
    st = nref.setup(cs.KINDS.index("dense"), n)
    G, C = good["G"].copy(), good["C"].copy()
    G[2], C[2] = bad["G"][0], bad["C"][0]
    args = (st["out"], st["src_a"], st["src_b"])
    for kernel in _kernels(n):
        r = noise_solve_batch(G, C, *args, st["psd"], cs.OMEGA, gain_in=st["gain_in"], kernel=kernel)
        assert r["flags"].tolist() == [0, 0, 4, 0, 0], (n, kernel)
        for k in KEYS:
            v = np.ascontiguousarray(r[k][2]).view(np.float64)
            assert np.all(v == 0) and not np.signbit(v).any(), (n, kernel, k)
        for s in (0, 1, 3, 4):
            solo = noise_solve_batch(G[s:s + 1], C[s:s + 1], *args, st["psd"][s:s + 1], cs.OMEGA, gain_in=st["gain_in"],
                                     kernel=kernel)
            assert int(solo["flags"][0]) == 0
            for k in KEYS:
                assert np.array_equal(_bits(solo[k][0]), _bits(r[k][s])), (n, kernel, s, k)


def test_singular_at_one_frequency_only():
    """a row that lives in C alone: singular at w = 0, regular before and after it in the same sweep -- +0.0 at that
    frequency only (no sign bit), 0x4 for the instance, the other frequencies the reference's"""
    for n in (2, 8, 13, 24, 32, 40, 63):
        c = nref.adjoint_case(cs.case("sing_dc_only", n))
        st = nref.setup(cs.KINDS.index("sing_dc_only"), n)
        ref = _reference(c, st)
        assert all(p == [0, 4, 0] for p in ref["per_f"])
        for kernel in _kernels(n):
            r = _run(c, st, cs.NSYS, kernel)
            assert r["flags"].tolist() == [4] * cs.NSYS
            for k in KEYS:
                v = np.ascontiguousarray(r[k][:, 1]).view(np.float64)
                assert np.all(v == 0) and not np.signbit(v).any(), (n, kernel, k)
                assert np.array_equal(_bits(r[k]), _bits(ref[k])), (n, kernel, k)
            assert np.all(r["y"][:, 0] != 0) and np.all(r["y"][:, 2] != 0)


def test_auto_kernel_optional_outputs_and_empty_batches():
    from circuitsimulator_amd import capi, noise_solve_batch
    for n, same_as in ((32, "packed"), (33, "wave")):
        c = cs.case("dense", n)
        st = nref.setup(0, n)
        ra, rk = _run(c, st, cs.NSYS, "auto"), _run(c, st, cs.NSYS, same_as)
        for k in KEYS + ("flags",):
            assert np.array_equal(ra[k].view(np.uint8), rk[k].view(np.uint8)), (n, k)
    # contrib, gain, y and flags are optional; B == 0 and F == 0 do nothing
    n = 6
    c = cs.case("dense", n)
    st = nref.setup(0, n)
    ref = _reference(c, st)
    S = len(st["src_a"])
    assert S > 0
    L = capi.lib()
    on = np.full((cs.NSYS, len(cs.OMEGA)), 7.0)
    psd = np.ascontiguousarray(st["psd"])
    head = (c["G"].ctypes.data, c["C"].ctypes.data, st["out"][0], st["out"][1], S, st["src_a"].ctypes.data,
            st["src_b"].ctypes.data, psd.ctypes.data, 0, -1, -1, cs.OMEGA.ctypes.data)
    assert L.csim_noise_solve_batch(0, n, 0, *head, 3, 0, on.ctypes.data, None, None, None, None) == capi.CSIM_OK
    assert L.csim_noise_solve_batch(0, n, cs.NSYS, *head, 0, 0, on.ctypes.data, None, None, None, None) == capi.CSIM_OK
    assert np.all(on == 7.0)
    assert L.csim_noise_solve_batch(0, n, cs.NSYS, *head, 3, 0, on.ctypes.data, None, None, None, None) == capi.CSIM_OK
    assert np.array_equal(_bits(on), _bits(ref["onoise"]))
    # no generators at all: onoise is +0.0
    r0 = noise_solve_batch(c["G"], c["C"], st["out"], [], [], np.zeros((cs.NSYS, 0)), cs.OMEGA)
    assert np.all(r0["onoise"] == 0) and not np.signbit(r0["onoise"]).any() and r0["gain"] is None
    assert np.array_equal(_bits(r0["y"]), _bits(ref["y"]))
    # bad arguments
    assert L.csim_noise_solve_batch(0, n, cs.NSYS, *head, 3, 3, on.ctypes.data, None, None, None, None) == capi.CSIM_ERR_ARG
    assert L.csim_noise_solve_batch(0, n, cs.NSYS, None, *head[1:], 3, 0, on.ctypes.data, None, None, None, None) == capi.CSIM_ERR_ARG
    for out in ((2, 2), (-1, 0), (n, -1), (0, n), (0, -2)):
        with pytest.raises(capi.CsimError) as e:
            noise_solve_batch(c["G"], c["C"], out, st["src_a"], st["src_b"], st["psd"], cs.OMEGA)
        assert e.value.code == capi.CSIM_ERR_ARG, out
    for a, b in ((n, 0), (0, n), (-2, 0)):
        with pytest.raises(capi.CsimError) as e:
            noise_solve_batch(c["G"], c["C"], (0, -1), [a], [b], np.ones((cs.NSYS, 1)), cs.OMEGA)
        assert e.value.code == capi.CSIM_ERR_ARG, (a, b)
    for gin in (("v", -1), ("v", n), ("i", n, 0), ("i", 0, -2)):
        with pytest.raises(capi.CsimError) as e:
            noise_solve_batch(c["G"], c["C"], (0, -1), [0], [1], np.ones((cs.NSYS, 1)), cs.OMEGA, gain_in=gin)
        assert e.value.code == capi.CSIM_ERR_ARG, gin


@pytest.mark.parametrize("n,kernel", [(64, "wave"), (64, "packed"), (64, "auto"), (33, "packed")])
def test_sizes_beyond_a_kernel_are_refused(n, kernel):
    from circuitsimulator_amd import CsimError, capi, noise_solve_batch
    G = np.eye(n)[None]
    with pytest.raises(CsimError) as e:
        noise_solve_batch(G, np.zeros_like(G), (0, -1), [0], [-1], np.ones((1, 1)), cs.OMEGA, kernel=kernel)
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
