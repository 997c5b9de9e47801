"""An independent statement of include/csim.h "S-parameter analysis" for the tests: the multi-RHS solve, the
admittance read-out and the S epilogue.

Written from the specification, not from the engine's sources (it neither includes, parses nor calls ac_port.hpp).
The multi-RHS solve is ac_reference.solve applied column by column: pivoting never looks at a right-hand side, so
that IS the definition.  Real and imaginary parts live on separate float64 planes and every IEEE operation of the
specification is one numpy operation on them.
"""
import numpy as np

import ac_reference

LU_TINY_PIVOT = ac_reference.LU_TINY_PIVOT
EPS = ac_reference.EPS


def solve_multi(Ar, Ai, Br, Bi, eps=EPS):
    """One system, K right-hand sides.  Ar, Ai [n][n]; Br, Bi [K][n] -> (flags, xr [K][n], xi [K][n], PivotLog)."""
    K, n = Br.shape
    xr, xi = np.zeros((K, n)), np.zeros((K, n))
    flags, log = 0, None
    for c in range(K):
        fl, xr[c], xi[c], lg = ac_reference.solve(Ar, Ai, Br[c].copy(), Bi[c].copy(), eps)
        flags |= fl
        log = log or lg
    if flags:                                                   # one factorisation: it fails for every column or none
        xr[:], xi[:] = 0.0, 0.0
    return flags, xr, xi, log


def sweep_rhs(G, C, J, omega, eps=EPS):
    """(G + j w C) X = J for every w.  J [K][n] complex -> (flags, x complex [F][K][n], [flags per w], [PivotLog])"""
    G, C = np.asarray(G, dtype=np.float64), np.asarray(C, dtype=np.float64)
    J = np.asarray(J, dtype=np.complex128)
    K, n = J.shape
    x = np.zeros((len(omega), K, n), dtype=np.complex128)
    flags, per_f, logs = 0, [], []
    for f, w in enumerate(omega):
        with np.errstate(all="ignore"):
            Ai = np.float64(w) * C
        fl, xr, xi, log = solve_multi(G, Ai, np.ascontiguousarray(J.real), np.ascontiguousarray(J.imag), eps)
        x[f].real, x[f].imag = xr, xi
        flags |= fl
        per_f.append(fl)
        logs.append(log)
    return flags, x, per_f, logs


def y_from_x(xr, xi, port_eq, failed):
    """Y(i,j) = -x(j)[k_i]; all +0.0 when the factorisation failed"""
    P = len(port_eq)
    Yr, Yi = np.zeros((P, P)), np.zeros((P, P))
    if not failed:
        for i in range(P):
            for j in range(P):
                Yr[i, j] = -xr[j][port_eq[i]]
                Yi[i, j] = -xi[j][port_eq[i]]
    return Yr, Yi


def s_from_y(Yr, Yi, sz, eps=EPS):
    """M = I + (s_i Y) s_j, M X = 2 I, S = X - I -> (flags, Sr, Si)"""
    P = len(sz)
    Mr, Mi = np.zeros((P, P)), np.zeros((P, P))
    with np.errstate(all="ignore"):
        for i in range(P):
            for j in range(P):
                t = sz[i] * Yr[i, j]
                re = t * sz[j]
                t = sz[i] * Yi[i, j]
                im = t * sz[j]
                Mr[i, j] = np.float64(1.0) + re if i == j else re
                Mi[i, j] = im
    rhs = 2.0 * np.eye(P)
    fl, xr, xi, _ = solve_multi(Mr, Mi, rhs, np.zeros((P, P)), eps)
    Sr, Si = np.zeros((P, P)), np.zeros((P, P))
    if not fl:
        with np.errstate(all="ignore"):
            for i in range(P):
                for j in range(P):
                    Sr[i, j] = xr[j][i] - np.float64(1.0) if i == j else xr[j][i]
                    Si[i, j] = xi[j][i]
    return fl, Sr, Si


def sweep_ports(G, C, omega, port_eq, z0, eps=EPS):
    """Unit right-hand sides at port_eq; -> dict(flags, per_f, x [F][P][n], y [F][P][P], s [F][P][P], logs)"""
    G, C = np.asarray(G, dtype=np.float64), np.asarray(C, dtype=np.float64)
    n, P, F = G.shape[0], len(port_eq), len(omega)
    sz = np.sqrt(np.asarray(z0, dtype=np.float64))
    J = np.zeros((P, n), dtype=np.complex128)
    for j in range(P):
        J[j, port_eq[j]] = 1.0
    _, x, per_a, logs = sweep_rhs(G, C, J, omega, eps)
    y = np.zeros((F, P, P), dtype=np.complex128)
    s = np.zeros((F, P, P), dtype=np.complex128)
    per_f = []
    for f in range(F):
        Yr, Yi = y_from_x(np.ascontiguousarray(x[f].real), np.ascontiguousarray(x[f].imag), port_eq, per_a[f] != 0)
        y[f].real, y[f].imag = Yr, Yi
        fl = per_a[f]
        if not fl:
            fl, Sr, Si = s_from_y(Yr, Yi, sz, eps)
            s[f].real, s[f].imag = Sr, Si
        per_f.append(fl)
    flags = 0
    for fl in per_f:
        flags |= fl
    return dict(flags=flags, per_f=per_f, x=x, y=y, s=s, logs=logs)
