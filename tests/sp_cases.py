"""The inputs of the S-parameter kernel tests, shared by the CPU test (reference against the host-compiled
ac_port.hpp) and the GPU test (kernels against the reference).  The systems are those of tests/ac_cases.py, all 16
kinds, at the sizes on both sides of every boundary of the register-resident kernel and at the ends of the LDS one.

Right-hand sides of a case: column 0 is the case's J; odd columns c are unit vectors at equation (7 c) mod n, the
ports' shape; column 2 is np.roll(J, 2) * -1, which is exact.
"""
import functools

import numpy as np

import ac_cases as cs
import sp_reference as spref

SIZES = (1, 2, 3, 7, 8, 9, 16, 17, 24, 25, 31, 32, 33, 48, 62, 63)
KS = (1, 2, 3, 4)
BATCHES = (1, 3)
Z0 = (50.0, 75.0, 25.0, 100.0)


def rhs(c, K):
    """-> J [NSYS][K][n] complex"""
    n = c["n"]
    J = np.zeros((cs.NSYS, K, n), dtype=np.complex128)
    for col in range(K):
        if col == 0:
            J[:, 0] = c["J"]
        elif col == 2:
            J[:, 2] = np.roll(c["J"], 2, axis=1) * -1
        else:
            J[:, col, (7 * col) % n] = 1.0
    return J


def port_eq(n, P):
    """first, last and middle equations (and one in between)"""
    return [0, n - 1, n // 2, (n - 1) // 3][:P]


def all_cases():
    return cs.all_cases(sizes=SIZES)


@functools.lru_cache(maxsize=None)
def _reference_rhs(kind, n):
    """the reference for K = 4 (column c of it is the reference of every K > c): per system (flags, x [F][4][n],
    per_f, logs)"""
    c = cs.case(kind, n)
    J = rhs(c, 4)
    return tuple(spref.sweep_rhs(c["G"][s], c["C"][s], J[s], cs.OMEGA) for s in range(cs.NSYS))


def reference_rhs(c, K):
    """-> (flags [NSYS] uint32, x [NSYS][F][K][n] complex, per_f, logs); computed once per case and shared"""
    res = _reference_rhs(c["kind"], c["n"])
    return (np.array([r[0] for r in res], dtype=np.uint32), np.stack([r[1][:, :K] for r in res]),
            [r[2] for r in res], [r[3] for r in res])


@functools.lru_cache(maxsize=None)
def _reference_ports(kind, n, P):
    c = cs.case(kind, n)
    return tuple(spref.sweep_ports(c["G"][s], c["C"][s], cs.OMEGA, port_eq(n, P), Z0[:P]) for s in range(cs.NSYS))


def reference_ports(c, P):
    """-> per system dict(flags, per_f, x, y, s, logs)"""
    return _reference_ports(c["kind"], c["n"], P)
