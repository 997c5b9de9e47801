"""The small-signal system of a netlist's nominal instance without a GPU, for the CPU tests of the loop-gain analysis:
the operating point and G from the CPU oracle (its transient stamp at a step of 1e300 s leaves no companion
conductance), C from the IR records as include/csim.h "AC analysis" states it."""
import ctypes as C

import numpy as np


class _IR(C.Structure):
    _fields_ = [("n_unknowns", C.c_int32), ("n_node_eq", C.c_int32), ("n_branch_eq", C.c_int32),
                ("n_elems", C.c_int32), ("n_params", C.c_int32), ("has_nonlinear", C.c_int32),
                ("kind", C.POINTER(C.c_int32)), ("eq", C.POINTER(C.c_int32)), ("branch_eq", C.POINTER(C.c_int32)),
                ("param_slot", C.POINTER(C.c_int32))]


def records(nl):
    ir = C.cast(nl.ir_ptr, C.POINTER(_IR)).contents
    return [(ir.kind[e], [ir.eq[4 * e + t] for t in range(4)], ir.branch_eq[e], ir.param_slot[e])
            for e in range(ir.n_elems)]


def numpy_c(nl, p):
    """the C part from the IR records, parameters p [P]"""
    N = nl.n_unknowns
    Cm = np.zeros((N, N))

    def cap(a, b, v):
        if v <= 0.0:
            return
        for i, j, s in ((a, a, 1), (b, b, 1), (a, b, -1), (b, a, -1)):
            if i >= 0 and j >= 0:
                Cm[i, j] += s * v
    for kind, q, k, s in records(nl):
        if kind == 1:
            cap(q[0], q[1], p[s])
        elif kind == 2 and p[s] > 0.0 and 0 <= k < N:
            Cm[k, k] -= p[s]
        elif kind in (5, 6):
            cj = p[s + 3]
            D, G, S, Bk = q
            cap(G, S, 0.5 * cj)
            cap(G, D, 0.5 * cj)
            cap(S, Bk, cj)
            cap(D, Bk, cj)
    return Cm


def nominal_system(nl):
    """-> (G [N][N], C [N][N], x_op [N]) of the nominal instance"""
    from oracle import binding as orc
    p = np.ascontiguousarray(nl.nominal_params, dtype=np.float64)
    x, _, st = orc.dc(nl.ir_ptr, nl.n_unknowns, p)
    assert st == 0
    G, _ = orc.stamp_tran(nl.ir_ptr, p, 0, x.copy(), x.copy(), 0.0, 1e300)
    return np.array(G), numpy_c(nl, p), x
