"""numpy restatement of the periodic AC analysis (include/csim.h "Periodic AC analysis") on top of the oracle binding
and tests/pss_reference.py: the orbit is pss_reference.period's (the reference's transient), J_k is oracle.stamp_tran at
the converged state, Hm and W_K are pss_reference's.  The product Hm p, the step's right-hand side z q + u and the
sideband sums are written as engine/pac.hpp writes them, operation by operation on separate real and imaginary planes,
so they agree with it bit for bit; the closure goes through ac_reference.solve (the complex LU stated from the
specification), the step solves through numpy.linalg.solve and agree to rounding."""
import ctypes as C
import math

import numpy as np

import ac_reference
import pss_reference as pr
from oracle import binding as oracle

PI = 3.14159265358979323846
ST_PAC_SINGULAR = 0x800


class _IR(C.Structure):
    _fields_ = [("n_unknowns", C.c_int32), ("n_node_eq", C.c_int32), ("n_branch_eq", C.c_int32),
                ("n_elems", C.c_int32), ("n_params", C.c_int32), ("has_nonlinear", C.c_int32),
                ("kind", C.POINTER(C.c_int32)), ("eq", C.POINTER(C.c_int32)), ("branch_eq", C.POINTER(C.c_int32)),
                ("param_slot", C.POINTER(C.c_int32))]


def excitation(nl):
    """u: a V source's AC value on its branch row, an I source's leaving its first node and entering its second"""
    ir = C.cast(nl.ir_ptr, C.POINTER(_IR)).contents
    N = nl.n_unknowns
    u = np.zeros(N, dtype=complex)
    for e in range(ir.n_elems):
        mag, deg = nl.ac_source(e)
        phi = deg * PI / 180.0
        v = complex(mag * math.cos(phi), mag * math.sin(phi))
        kind, k = ir.kind[e], ir.branch_eq[e]
        if kind == 3 and 0 <= k < N:
            u[k] += v
        elif kind == 4:
            if ir.eq[4 * e] >= 0:
                u[ir.eq[4 * e]] -= v
            if ir.eq[4 * e + 1] >= 0:
                u[ir.eq[4 * e + 1]] += v
    return u


def z_consts(f, h, f0):
    """-> (z, z_K) as pac.hpp's pac_z makes them: libm's cos and sin of the same arguments"""
    th = 2.0 * PI * f * h
    ratio = f / f0
    thK = 2.0 * PI * (ratio - math.floor(ratio))
    return complex(math.cos(th), -math.sin(th)), complex(math.cos(thK), -math.sin(thK))


def hm_product(Hm, pr_, pi_):
    """q = Hm p over the non-zero entries of each row, l ascending; pr_, pi_ [N][F]"""
    qr = np.zeros_like(pr_)
    qi = np.zeros_like(pi_)
    for l in range(Hm.shape[1]):
        nz = (Hm[:, l] != 0.0)[:, None]
        tr = Hm[:, l][:, None] * pr_[l][None, :]
        ti = Hm[:, l][:, None] * pi_[l][None, :]
        qr = np.where(nz, qr + tr, qr)
        qi = np.where(nz, qi + ti, qi)
    return qr, qi


def step_rhs(zr, zi, qr, qi, ur, ui):
    """z q + u; zr, zi [F], q [N][F], u [N]"""
    a = zr[None, :] * qr
    b = zi[None, :] * qi
    t = a - b
    re = t + ur[:, None]
    c = zr[None, :] * qi
    d = zi[None, :] * qr
    v = c + d
    im = v + ui[:, None]
    return re, im


def close_matrix(W, zK):
    """I - z_K W entry by entry -> (Ar, Ai)"""
    n = W.shape[0]
    a = zK.real * W
    b = zK.imag * W
    return np.where(np.eye(n, dtype=bool), 1.0, 0.0) - a, 0.0 - b


def sideband_sums(ps, c, s, M):
    """ps complex [K][N][F]: p_1 .. p_K -> P complex [F][2 M + 1][N], the sums in pac.hpp's order"""
    K = ps.shape[0]
    out = np.zeros((ps.shape[2], 2 * M + 1, ps.shape[1]), dtype=complex)
    scale = 1.0 / float(K)
    for m in range(-M, M + 1):
        re = np.zeros(ps.shape[1:])
        im = np.zeros(ps.shape[1:])
        for k in range(1, K + 1):
            j = ((m * k) % K + K) % K
            pr_, pi_ = ps[k - 1].real, ps[k - 1].imag
            a = pr_ * c[j]
            b = pi_ * s[j]
            t = a + b
            re = re + t
            d = pi_ * c[j]
            e = pr_ * s[j]
            v = d - e
            im = im + v
        out[:, m + M, :].real = (scale * re).T
        out[:, m + M, :].imag = (scale * im).T
    return out


def jacobians(ir, params, b, h, xs):
    """J_k at the converged states of the orbit xs [K+1][N], k = 1 .. K"""
    return [oracle.stamp_tran(ir, params, b, xs[k], xs[k - 1], float(k) * h, h)[0] for k in range(1, xs.shape[0])]


def recursion(Js, Hm, u, z, p0):
    """J_k p_k = z (Hm p_{k-1}) + u from p0 complex [N][F] -> complex [K][N][F]"""
    zr, zi = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    ur, ui = np.ascontiguousarray(u.real), np.ascontiguousarray(u.imag)
    p_r, p_i = np.ascontiguousarray(p0.real), np.ascontiguousarray(p0.imag)
    F = len(z)
    out = np.zeros((len(Js),) + p0.shape, dtype=complex)
    for k, J in enumerate(Js):
        qr, qi = hm_product(Hm, p_r, p_i)
        re, im = step_rhs(zr, zi, qr, qi, ur, ui)
        sol = np.linalg.solve(J, np.concatenate([re, im], axis=1))
        p_r, p_i = np.ascontiguousarray(sol[:, :F]), np.ascontiguousarray(sol[:, F:])
        out[k].real = p_r
        out[k].imag = p_i
    return out


def pac(ir, N, params, b, h, K, f0, x0, freqs, M, u, table=None, orbit=None):
    """The analysis of instance b around the orbit that starts at x0.
    -> dict(P complex [F][2 M + 1][N], status [F] (ST_PAC_SINGULAR per frequency whose closure fails), p0 [N][F],
            ps [K][N][F], xs, Js, Hm, W, z, zK)"""
    c, s = table if table is not None else pr.twiddles(K)
    Hm = pr.hm_matrix(ir, N, params, b, h)
    if orbit is None:
        xs, st = pr.period(ir, N, params, b, h, K, x0)
        assert xs is not None and np.all(np.isfinite(xs)), st
        W = pr.sensitivity(ir, N, params, b, h, xs, Hm)
    else:
        xs, W = orbit
    Js = jacobians(ir, params, b, h, xs)
    zs = [z_consts(float(f), h, f0) for f in freqs]
    z = np.array([v[0] for v in zs])
    zK = np.array([v[1] for v in zs])
    F = len(freqs)
    rK = recursion(Js, Hm, u, z, np.zeros((N, F), dtype=complex))[-1]
    p0 = np.zeros((N, F), dtype=complex)
    status = np.zeros(F, dtype=np.uint32)
    for f in range(F):
        Ar, Ai = close_matrix(W, zK[f])
        fl, xr, xi, _ = ac_reference.solve(Ar, Ai, rK[:, f].real.copy(), rK[:, f].imag.copy())
        if fl:
            status[f] |= ST_PAC_SINGULAR
        p0[:, f].real = xr
        p0[:, f].imag = xi
    ps = recursion(Js, Hm, u, z, p0)
    P = sideband_sums(ps, c, s, M)
    P[status != 0] = 0.0
    return dict(P=P, status=status, p0=p0, ps=ps, xs=xs, Js=Js, Hm=Hm, W=W, z=z, zK=zK)


def closed_form_linear(J, Hm, u, z):
    """P_0 = (J - z Hm)^-1 u of a linear circuit, numpy.clongdouble by Newton refinement of numpy's double inverse"""
    CL = np.clongdouble
    A = J.astype(CL) - CL(z) * Hm.astype(CL)
    Ai = np.linalg.inv(A.astype(complex)).astype(CL)
    for _ in range(3):
        Ai = Ai + Ai @ (np.eye(A.shape[0], dtype=CL) - A @ Ai)
    return Ai @ u.astype(CL)


def agreement_bound(r, f):
    """How far two evaluations of the recursion in float64 may lie apart at frequency index f of a pac() result: the
    rounding of one step's solve, 2^-52 cond(J_k) |p|, reaches p_K through S_K .. S_(k+1), S_k = J_k^-1 Hm, and the
    periodic start through (I - z_K W_K)^-1:
        2^-52 ||(I - z_K W_K)^-1||_inf  sum_k ||S_K .. S_(k+1)||_inf  max_k cond_inf(J_k)  max |P|"""
    N = r["Hm"].shape[0]
    S = [np.linalg.solve(J, r["Hm"]) for J in r["Js"]]
    total, Pm = 0.0, np.eye(N)
    for k in range(len(S), 0, -1):
        total += pr.norm_inf(Pm)
        Pm = Pm @ S[k - 1]
    cond = max(pr.norm_inf(J) * pr.norm_inf(np.linalg.inv(J)) for J in r["Js"])
    Ar, Ai = close_matrix(r["W"], r["zK"][f])
    A = Ar + 1j * Ai
    minv = float(np.max(np.sum(np.abs(np.linalg.inv(A)), axis=1)))
    return 2.0 ** -52 * minv * total * cond * float(np.max(np.abs(r["P"][f])))


_CACHE = {}


def setup(name):
    """-> (netlist, tstep, K) of a case of tests/pac_cases.py"""
    import pac_cases as ac
    return ac.netlist(name), ac.tstep(name), ac.CASES[name][1]


def reference(name, B, M=None):
    """The steady state (pss_reference.shoot from the DC point) and the analysis around it for every instance of a batch
    of B at pac_cases.freqs(), computed once per (name, B) and shared by the tests
    -> (params [P][B], [shoot() result], [pac() result])"""
    import pac_cases as ac
    M = ac.N_SIDE if M is None else M
    if (name, B, M) not in _CACHE:
        nl, h, K = setup(name)
        N = nl.n_unknowns
        p = ac.params(nl, B)
        u = excitation(nl)
        orbits, res = [], []
        for b in range(B):
            xdc, _, _ = oracle.dc(nl.ir_ptr, N, p, b)
            o = pr.shoot(nl.ir_ptr, N, p, b, h, K, xdc, pr.TOL, pr.MAX_ROUNDS, 0)
            orbits.append(o)
            res.append(pac(nl.ir_ptr, N, p, b, h, K, ac.F0, o["x0"], ac.freqs(name), M, u, orbit=(o["xs"], o["W"])))
        _CACHE[(name, B, M)] = (p, orbits, res)
    return _CACHE[(name, B, M)]
