"""The inputs of the block-kernel tests (ac_kernel=block, 64 to 1024 unknowns), shared by the CPU test (reference
against the host-compiled ac_lu_solve(), tests/test_ac_block_cpu.py) and the GPU tests (kernels against the reference,
tests/test_ac_block_kernels_gpu.py).

The systems are those of tests/ac_cases.py -- case(kind, n) works at any n -- at sizes beyond its SIZES; the tests run
the first NSYS systems of a case.  One more input, "tri1024", is a 1024-unknown complex tridiagonal system whose
sub-diagonal outweighs its diagonal at many columns, so that rows are exchanged all along the factorisation.
References are computed once per process and shared (never written to).
"""
import functools

import numpy as np

import ac_cases as cs
import ac_reference

SIZES = (64, 65, 97, 129)                     # every kind, in the CPU and the GPU test
GPU_SIZES = (64, 65, 97, 98, 99, 100, 128, 129)
SMALL_SIZES = (1, 2, 3, 33, 63)               # block against wave
NOISE_SIZES = (64, 65, 99, 129)
BIG_N = 257
BIG_KINDS = ("dense", "mna", "tie_rows", "sing_mid", "thr_both", "nan_below")
NSYS = 3
OMEGA = cs.OMEGA
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def case(kind, n, nsys=NSYS):
    """the first nsys systems of ac_cases.case(kind, n), bit for bit (the same generator, drawn in the same order;
    the MNA-like kind takes seconds per system at 257 unknowns, so only those that run are drawn)"""
    if nsys == cs.NSYS:
        return cs.case(kind, n)
    rng = np.random.default_rng([20240607, cs.KINDS.index(kind), n])
    sys = [cs._system(rng, kind, n) for _ in range(nsys)]
    if any(s is None for s in sys):
        return None
    A = np.stack([s[0] for s in sys])
    return dict(kind=kind, n=n, G=np.ascontiguousarray(A.real), C=np.ascontiguousarray(A.imag),
                J=np.stack([s[1] for s in sys]))


@functools.lru_cache(maxsize=None)
def reference(kind, n, nsys=NSYS):
    """-> (flags [nsys] uint32, x [nsys][F][n] complex, per-frequency flags, pivot logs) of the first nsys systems"""
    c = case(kind, n, nsys)
    res = [ac_reference.solve_sweep(c["G"][s], c["C"][s], c["J"][s], OMEGA) for s in range(nsys)]
    x = np.stack([r[1] for r in res])
    x.setflags(write=False)
    return (np.array([r[0] for r in res], dtype=np.uint32), x, [r[2] for r in res], [r[3] for r in res])


@functools.lru_cache(maxsize=None)
def tri1024(n=1024):
    """-> (G [n][n], C [n][n], J complex [n])"""
    rng = np.random.default_rng(5)
    G = np.zeros((n, n))
    C = np.zeros((n, n))
    i = np.arange(n)
    G[i, i] = 4.0 * rng.choice([-1, 1], n)
    C[i, i] = rng.standard_normal(n)
    G[i[:-1], i[:-1] + 1] = rng.standard_normal(n - 1)
    C[i[:-1], i[:-1] + 1] = rng.standard_normal(n - 1)
    G[i[:-1] + 1, i[:-1]] = 2.0 * rng.standard_normal(n - 1)
    C[i[:-1] + 1, i[:-1]] = 2.0 * rng.standard_normal(n - 1)
    J = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    for a in (G, C, J):
        a.setflags(write=False)
    return G, C, J


@functools.lru_cache(maxsize=None)
def tri1024_reference():
    """-> (flags OR-ed, x [F][n] complex, per-frequency flags, pivot logs)"""
    G, C, J = tri1024()
    r = ac_reference.solve_sweep(G, C, J, OMEGA)
    r[1].setflags(write=False)
    return r


def same(x, ref, nan_expected, where):
    """bitwise equality; where NaNs are expected: equal NaN masks, bitwise equality elsewhere"""
    x, ref = np.ascontiguousarray(x), np.ascontiguousarray(ref)
    assert x.shape == ref.shape, where + (x.shape, ref.shape)
    xb, rb = x.view(np.uint64), ref.view(np.uint64)
    if not nan_expected:
        assert not np.isnan(ref.view(np.float64)).any(), where
        assert np.array_equal(xb, rb), where
        return
    nx, nr = np.isnan(x.view(np.float64)), np.isnan(ref.view(np.float64))
    assert np.array_equal(nx, nr), where
    assert np.array_equal(np.where(nx, 0, xb), np.where(nr, 0, rb)), where


def failed_are_plus_zero(x, per_f, where):
    """x [nsys][F][...]: the solves that per_f flags are +0.0 with no sign bit anywhere"""
    for s, fl in enumerate(per_f):
        for f, v in enumerate(fl):
            if v:
                w = np.ascontiguousarray(x[s, f]).view(np.float64)
                assert np.all(w == 0) and not np.signbit(w).any(), where + (s, f)
