"""The inputs of the two-port noise kernel tests, shared by the CPU test (reference against the host-compiled
ac_port_noise.hpp) and the GPU test (kernels against the reference).

A case is an ac_cases case (kind, n) -- five systems -- handed over transposed (noise_reference.adjoint_case: the
analysis factors A^T, so the structured kinds meet their feature where the AC solve meets it), with ports
sp_cases.port_eq(n, P) and one generator table shared by the five systems, as the instances of a circuit share theirs.
P and the generator count S walk through all 32 combinations of P = 1 .. 4 and S in S_VALUES along the case list, so
every size sees every P, and each S (an empty table; one below, at and above the 32-lane and the 64-lane chunk) meets
sizes on both sides of the packed kernel's limit.

Generator ends: generator 0 runs from ground (-1) to the branch equation of port 1; generator 1 lies between an
equation and its neighbour; generator 2 has a PSD of 0.0 in every system; the rest are random in -1 .. n-1.
"""
import functools

import numpy as np

import ac_cases as cs
import noise_reference as nref
import sp_cases as sc
import spnoise_reference as spnref

SIZES = (2, 3, 8, 9, 16, 17, 24, 25, 31, 32, 33, 48, 63)
PORTS = (1, 2, 3, 4)
S_VALUES = (0, 1, 5, 31, 32, 33, 64, 65)
BATCHES = (1, 3)
Z0 = sc.Z0


def shape(kind, n):
    """-> (P, S) of the case (kind, n)"""
    idx = cs.KINDS.index(kind) * len(SIZES) + SIZES.index(n)
    return PORTS[idx % 4], S_VALUES[(idx // 4) % 8]


def table(kind, n, seed=20250822):
    """-> (src_a [S] int32, src_b [S] int32, psd [NSYS][S])"""
    P, S = shape(kind, n)
    rng = np.random.default_rng([seed, cs.KINDS.index(kind), n])
    a = rng.integers(-1, n, S).astype(np.int32)
    b = rng.integers(-1, n, S).astype(np.int32)
    psd = 1.6e-20 * rng.uniform(1e-6, 1.0, (cs.NSYS, S))
    if S >= 1:
        a[0], b[0] = -1, sc.port_eq(n, P)[0]
    if S >= 2:
        b[1] = max(int(b[1]), 0)
        a[1] = (b[1] + 1) % n
    if S >= 3:
        psd[:, 2] = 0.0
    return a, b, psd


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """-> dict(kind, n, P, S, G, C [5][n][n] (the systems whose TRANSPOSE is factored), port_eq, z0, src_a, src_b,
    psd [5][S]) or None when the size has no room for the kind's feature"""
    c = cs.case(kind, n)
    if c is None:
        return None
    c = nref.adjoint_case(c)
    P, S = shape(kind, n)
    a, b, psd = table(kind, n)
    return dict(kind=kind, n=n, P=P, S=S, G=c["G"], C=c["C"], port_eq=sc.port_eq(n, P), z0=list(Z0[:P]), src_a=a, src_b=b,
                psd=psd)


def all_cases(sizes=SIZES, kinds=cs.KINDS):
    for n in sizes:
        for kind in kinds:
            c = case(kind, n)
            if c is not None:
                yield c


@functools.lru_cache(maxsize=None)
def _reference(kind, n):
    c = case(kind, n)
    return tuple(spnref.sweep(c["G"][s], c["C"][s], cs.OMEGA, c["port_eq"], c["z0"], c["src_a"], c["src_b"], c["psd"][s])
                 for s in range(cs.NSYS))


def reference(c):
    """-> per system the dict of spnoise_reference.sweep; computed once per case, shared, never written to"""
    return _reference(c["kind"], c["n"])


KEYS2 = ("nf", "fmin", "rn", "yopt")


def keys(P):
    return ("x", "y", "cy") + (KEYS2 if P == 2 else ())
