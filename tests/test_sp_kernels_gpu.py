"""The two S-parameter sweep kernels (kernels_sp.hip: one wavefront per system in LDS, N <= 63; 32 lanes per system
in registers, N <= 32) fed directly through csim_sp_solve_batch and compared bit for bit with tests/sp_reference.py,
the specification of include/csim.h "S-parameter analysis" restated in numpy (which tests/test_sp_cpu.py in turn
holds against the host-compiled ac_port.hpp, on these same inputs).

Inputs: tests/sp_cases.py -- the systems of tests/ac_cases.py at both sides of every size boundary, K = 1 .. 4
right-hand sides, batches of 1 and 3 (an odd batch leaves the second half of the last packed wavefront empty).

NaN and singular inputs are ordinary data for these kernels, as for the AC kernels: only arithmetic results depend
on them, never an address or a loop bound.  Port equations index LDS and are range-checked on the host.
"""
import numpy as np
import pytest

import ac_cases as cs
import sp_cases as sc
import sp_reference as spref
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


@pytest.mark.parametrize("K", sc.KS)
def test_kernels_equal_reference_bitwise(K):
    from circuitsimulator_amd import ac_solve_batch, sp_solve_batch
    cov = cs.Coverage()
    launches = 0
    for c in sc.all_cases():
        n, kind = c["n"], c["kind"]
        J = sc.rhs(c, K)
        flags, xref, per_f, logs = sc.reference_rhs(c, K)
        for s in range(cs.NSYS):
            cov.add(n, logs[s])
        for kernel in _kernels(n):
            for B in sc.BATCHES:
                x, fl = sp_solve_batch(c["G"][:B], c["C"][:B], J[:B], cs.OMEGA, kernel=kernel)
                launches += 1
                where = (kind, n, K, kernel, B)
                assert x.shape == (B, len(cs.OMEGA), K, n)
                assert np.array_equal(fl, flags[:B]), where + (fl.tolist(), flags[:B].tolist())
                _same(x, xref[:B], kind in cs.HAS_NAN, where)
            if K == 1:                                          # the single-RHS AC kernels on the same inputs
                xa, fa = ac_solve_batch(c["G"], c["C"], c["J"], cs.OMEGA, kernel=kernel)
                xs, fs = sp_solve_batch(c["G"], c["C"], J, cs.OMEGA, kernel=kernel)
                assert np.array_equal(fa, fs), (kind, n, kernel)
                _same(xs[:, :, 0], xa, True, (kind, n, kernel, "ac_solve_batch"))
    print("K = %d: %d launches; %s" % (K, launches, cov))
    cov.check()


@pytest.mark.parametrize("n", [8, 9, 32, 33, 63])
def test_singular_neighbour_leaves_the_others_alone(n):
    """a batch of five with system 2 singular: systems 0, 1, 3, 4 equal their solo results bit for bit"""
    from circuitsimulator_amd import sp_solve_batch
    good, bad = cs.case("dense", n), cs.case("sing_mid", n)
    G, C, J = good["G"].copy(), good["C"].copy(), sc.rhs(good, 4)
    G[2], C[2], J[2] = bad["G"][0], bad["C"][0], sc.rhs(bad, 4)[0]
    for kernel in _kernels(n):
        x, fl = sp_solve_batch(G, C, J, cs.OMEGA, kernel=kernel)
        assert fl.tolist() == [0, 0, 4, 0, 0], (n, kernel)
        assert np.all(x[2] == 0) and not np.signbit(x[2].view(np.float64)).any()
        for s in (0, 1, 3, 4):
            xs, fs = sp_solve_batch(G[s:s + 1], C[s:s + 1], J[s:s + 1], cs.OMEGA, kernel=kernel)
            assert int(fs[0]) == 0
            assert np.array_equal(xs[0].view(np.uint64), x[s].view(np.uint64)), (n, kernel, s)


@pytest.mark.parametrize("P", sc.KS)
def test_y_and_s_equal_reference_bitwise(P):
    """the port mode: unit right-hand sides at the first, last and middle equations, Z0 = (50, 75, 25, 100)"""
    from circuitsimulator_amd import sp_solve_batch
    n_failed = 0
    for c in sc.all_cases():
        n, kind = c["n"], c["kind"]
        ref = sc.reference_ports(c, P)
        want_fl = np.array([r["flags"] for r in ref], dtype=np.uint32)
        for kernel in _kernels(n):
            for B in sc.BATCHES:
                r = sp_solve_batch(c["G"][:B], c["C"][:B], None, cs.OMEGA, kernel=kernel, port_eq=sc.port_eq(n, P),
                                   z0=sc.Z0[:P])
                where = (kind, n, P, kernel, B)
                assert np.array_equal(r["flags"], want_fl[:B]), where
                for key in ("x", "y", "s"):
                    _same(r[key], np.stack([ref[s][key] for s in range(B)]), kind in cs.HAS_NAN, where + (key,))
        n_failed += int(np.count_nonzero(want_fl))
    assert n_failed > 0
    # S is optional
    c = cs.case("dense", 9)
    r = sp_solve_batch(c["G"], c["C"], None, cs.OMEGA, port_eq=sc.port_eq(9, P), z0=sc.Z0[:P], want_s=False)
    assert r["s"] is None
    assert np.array_equal(r["y"].view(np.uint64), np.stack([q["y"] for q in sc.reference_ports(c, P)]).view(np.uint64))


@pytest.mark.parametrize("P", sc.KS)
def test_singular_m_keeps_y(P):
    """Y = -I at Z0 = 1 (built directly as G): S = 0, Y kept, flag 0x4 -- beside a regular neighbour"""
    from circuitsimulator_amd import sp_solve_batch
    n = 2 * P
    G = np.zeros((2, n, n))
    G[0] = np.eye(n)
    G[1] = np.eye(n)
    G[1, P:, P:] *= 3.0                                         # Y = -I / 3: regular
    pe = [P + i for i in range(P)]
    ref = [spref.sweep_ports(G[b], np.zeros((n, n)), cs.OMEGA, pe, [1.0] * P) for b in range(2)]
    assert ref[0]["per_f"] == [4, 4, 4] and ref[1]["per_f"] == [0, 0, 0]
    for kernel in ("wave", "packed"):
        r = sp_solve_batch(G, np.zeros_like(G), None, cs.OMEGA, kernel=kernel, port_eq=pe, z0=[1.0] * P)
        assert r["flags"].tolist() == [4, 0]
        assert np.array_equal(r["y"][0, 0], -np.eye(P))
        v = r["s"][0].view(np.float64)
        assert np.all(v == 0) and not np.signbit(v).any()
        for key in ("y", "s"):
            assert np.array_equal(r[key].view(np.uint64), np.stack([q[key] for q in ref]).view(np.uint64)), (kernel, key)


def test_arguments_are_checked():
    from circuitsimulator_amd import CsimError, capi, sp_solve_batch
    c = cs.case("dense", 5)
    for kw in (dict(port_eq=[0, 5], z0=[50.0, 50.0]), dict(port_eq=[-1], z0=[50.0]), dict(port_eq=[0], z0=[0.0]),
               dict(port_eq=[0], z0=[float("inf")]), dict(port_eq=[0, 1, 2, 3, 4], z0=[50.0] * 5)):
        with pytest.raises(CsimError) as e:
            sp_solve_batch(c["G"], c["C"], None, cs.OMEGA, **kw)
        assert e.value.code == capi.CSIM_ERR_ARG, kw
    for K in (0, 5):
        with pytest.raises(CsimError) as e:
            sp_solve_batch(c["G"], c["C"], np.zeros((cs.NSYS, K, 5), dtype=complex), cs.OMEGA)
        assert e.value.code == capi.CSIM_ERR_ARG
    for n, kernel in ((64, "wave"), (64, "auto"), (33, "packed")):
        G = np.eye(n)[None]
        with pytest.raises(CsimError) as e:
            sp_solve_batch(G, np.zeros_like(G), np.ones((1, 2, n), dtype=complex), cs.OMEGA, kernel=kernel)
        assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
