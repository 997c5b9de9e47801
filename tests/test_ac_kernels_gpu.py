"""The two AC sweep kernels (kernels_ac.hip: one wavefront per system in LDS, N <= 63; 32 lanes per system in
registers, N <= 32) fed directly through csim_ac_solve_batch and compared bit for bit with tests/ac_reference.py,
the specification of include/csim.h "AC analysis" restated in numpy (which tests/test_ac_cpu.py in turn holds
against the host-compiled ac_lu_solve(), on these same inputs).

Inputs: tests/ac_cases.py -- every n from 1 to 63, batches of 1, 2, 3 and 5 (an odd batch leaves the second
half of the last packed wavefront empty), three frequencies with w = 0 among them; dense, MNA-like sparse,
permuted rows, exact ties, singular columns, the lu_eps threshold, NaNs.

NaN and singular inputs are ordinary data for these kernels: only arithmetic results depend on them, never an
address or a loop bound.  In the packed kernel a finite diagonal guarantees a candidate equal to the column
maximum and a NaN diagonal takes the keep-the-pivot branch, so the ballot that names the pivot lane is never
empty; the wave kernel indexes LDS by lane and column only.  Nothing here provokes a fault.
"""
import numpy as np
import pytest

import ac_cases as cs
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def _kernels(n):
    return ("wave", "packed") if n <= 32 else ("wave",)


def _same(x, ref, nan_expected, where):
    """bitwise equality; where NaNs are expected: equal NaN masks, bitwise equality elsewhere"""
    xb, rb = np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(ref).view(np.uint64)
    if not nan_expected:
        assert not np.isnan(ref.view(np.float64)).any(), where
        assert np.array_equal(xb, rb), where
        return
    nx, nr = np.isnan(x.view(np.float64)), np.isnan(ref.view(np.float64))
    assert np.array_equal(nx, nr), where
    assert np.array_equal(np.where(nx, 0, xb), np.where(nr, 0, rb)), where


@pytest.mark.parametrize("cls", range(len(cs.SIZE_CLASSES)), ids=["n<=%d" % hi for _, hi in cs.SIZE_CLASSES])
def test_kernels_equal_reference_bitwise(cls):
    from circuitsimulator_amd import ac_solve_batch
    lo, hi = cs.SIZE_CLASSES[cls]
    cov = cs.Coverage()
    launches = 0
    for c in cs.all_cases(sizes=range(lo, hi + 1)):
        n, kind = c["n"], c["kind"]
        flags, xref, per_f, logs = cs.reference(c)
        for s in range(cs.NSYS):
            cov.add(n, logs[s])
        for kernel in _kernels(n):
            for B in cs.BATCHES:
                x, fl = ac_solve_batch(c["G"][:B], c["C"][:B], c["J"][:B], cs.OMEGA, kernel=kernel)
                launches += 1
                where = (kind, n, kernel, B)
                assert x.shape == (B, len(cs.OMEGA), n)
                assert np.array_equal(fl, flags[:B]), where + (fl.tolist(), flags[:B].tolist())
                _same(x, xref[:B], kind in cs.HAS_NAN, where)
    print("size class n<=%d: %d launches; systems that swapped in >= n/2 columns %d, took the first of tied rows %d, "
          "skipped a zero multiplier %d" % (hi, launches, cov.swaps[cls], cov.ties[cls], cov.skips[cls]))
    assert cov.swaps[cls] > 0 and cov.ties[cls] > 0 and cov.skips[cls] > 0, str(cov)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 16, 17, 23, 24, 25, 31, 32, 33, 48, 63])
def test_singular_neighbour_leaves_the_others_alone(n):
    """a batch of five with system 2 singular: systems 0, 1, 3, 4 equal their solo results bit for bit"""
    from circuitsimulator_amd import ac_solve_batch
    good, bad = cs.case("dense", n), cs.case("sing_mid", n)
    G, C, J = good["G"].copy(), good["C"].copy(), good["J"].copy()
    G[2], C[2], J[2] = bad["G"][0], bad["C"][0], bad["J"][0]
    for kernel in _kernels(n):
        x, fl = ac_solve_batch(G, C, J, cs.OMEGA, kernel=kernel)
        assert fl.tolist() == [0, 0, 4, 0, 0], (n, kernel)
        assert np.all(x[2] == 0) and not np.signbit(x[2].view(np.float64)).any()
        for s in (0, 1, 3, 4):
            xs, fs = ac_solve_batch(G[s:s + 1], C[s:s + 1], J[s:s + 1], cs.OMEGA, kernel=kernel)
            assert int(fs[0]) == 0
            assert np.array_equal(xs[0].view(np.uint64), x[s].view(np.uint64)), (n, kernel, s)


def test_singular_at_one_frequency_only():
    """a row that lives in C alone: singular at w = 0, regular before and after it in the same sweep -- the zero
    vector at that frequency, 0x4 for the instance, the other frequencies' vectors the reference's"""
    from circuitsimulator_amd import ac_solve_batch
    for n in (2, 8, 13, 24, 32, 40, 63):
        c = cs.case("sing_dc_only", n)
        flags, xref, per_f, _ = cs.reference(c)
        assert all(p == [0, 4, 0] for p in per_f)
        for kernel in _kernels(n):
            x, fl = ac_solve_batch(c["G"], c["C"], c["J"], cs.OMEGA, kernel=kernel)
            assert fl.tolist() == [4] * cs.NSYS
            assert np.all(x[:, 1] == 0) and np.all(x[:, 0] != 0) and np.all(x[:, 2] != 0)
            assert np.array_equal(x.view(np.uint64), xref.view(np.uint64)), (n, kernel)


def test_auto_kernel_and_optional_flags():
    from circuitsimulator_amd import ac_solve_batch, capi
    for n, same_as in ((32, "packed"), (33, "wave")):
        c = cs.case("dense", n)
        xa, fa = ac_solve_batch(c["G"], c["C"], c["J"], cs.OMEGA)
        xk, fk = ac_solve_batch(c["G"], c["C"], c["J"], cs.OMEGA, kernel=same_as)
        assert np.array_equal(xa.view(np.uint64), xk.view(np.uint64)) and np.array_equal(fa, fk)
    # flags are optional; B == 0 and F == 0 do nothing
    c = cs.case("dense", 5)
    x = np.full((cs.NSYS, 3, 5), 7.0 + 7.0j)
    L = capi.lib()
    args = (c["G"].ctypes.data, c["C"].ctypes.data, c["J"].ctypes.data, cs.OMEGA.ctypes.data)
    assert L.csim_ac_solve_batch(0, 5, 0, *args, 3, 0, x.ctypes.data, None) == capi.CSIM_OK
    assert L.csim_ac_solve_batch(0, 5, cs.NSYS, *args, 0, 0, x.ctypes.data, None) == capi.CSIM_OK
    assert np.all(x == 7.0 + 7.0j)
    assert L.csim_ac_solve_batch(0, 5, cs.NSYS, *args, 3, 0, x.ctypes.data, None) == capi.CSIM_OK
    assert np.array_equal(x.view(np.uint64), cs.reference(c)[1].view(np.uint64))
    assert L.csim_ac_solve_batch(0, 5, cs.NSYS, *args, 3, 3, x.ctypes.data, None) == capi.CSIM_ERR_ARG
    assert L.csim_ac_solve_batch(0, 5, cs.NSYS, None, *args[1:], 3, 0, x.ctypes.data, None) == capi.CSIM_ERR_ARG


@pytest.mark.parametrize("n,kernel", [(64, "wave"), (64, "packed"), (64, "auto"), (33, "packed")])
def test_sizes_beyond_a_kernel_are_refused(n, kernel):
    from circuitsimulator_amd import CsimError, ac_solve_batch, capi
    G = np.eye(n)[None]
    with pytest.raises(CsimError) as e:
        ac_solve_batch(G, np.zeros_like(G), np.ones((1, n), dtype=complex), cs.OMEGA, kernel=kernel)
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
