"""An independent statement of include/csim.h "Two-port noise analysis" for the tests: the adjoint multi-RHS solve, the
admittance read-out, the correlation sums and the two-port noise parameters.

Written from the specification, not from the engine's sources (it neither includes, parses nor calls
ac_port_noise.hpp).  The solve is sp_reference.solve_multi (ac_reference.solve column by column) on the transposed
planes.  As in ac_reference.py every IEEE operation of the specification is one numpy operation on float64 values.
"""
import numpy as np

import ac_reference
import sp_reference as spref

K_BOLTZMANN = 1.380649e-23
EPS = ac_reference.EPS
F64 = np.float64


def kt4(temp_k):
    return F64(4.0) * F64(K_BOLTZMANN) * F64(temp_k)


KT4_0 = kt4(290.0)


def _at(xr, xi, eq):
    if eq < 0:
        return F64(0.0), F64(0.0)
    return xr[eq], xi[eq]


def _transfer(xr, xi, a, b):
    ar, ai = _at(xr, xi, a)
    br, bi = _at(xr, xi, b)
    return ar - br, ai - bi


def _abs2(re, im):
    a = re * re
    b = im * im
    return a + b


def _div(ar, ai, pr, pi):
    inv = F64(1.0) / _abs2(pr, pi)
    t1 = ar * pr
    t2 = ai * pi
    t3 = ai * pr
    t4 = ar * pi
    return (t1 + t2) * inv, (t3 - t4) * inv


def two_port(y11, y21, c11, c22, c12, gs, kt40=KT4_0):
    """-> dict(nf, fmin, rn, yopt, cvv_positive) from Y11, Y21 (complex), Cy11.re, Cy22.re, Cy12 (complex), Gs"""
    one, two = F64(1.0), F64(2.0)
    y11r, y11i, y21r, y21i = F64(y11.real), F64(y11.imag), F64(y21.real), F64(y21.imag)
    c11, c22, c12r, c12i, gs = F64(c11), F64(c22), F64(c12.real), F64(c12.imag), F64(gs)
    with np.errstate(all="ignore"):
        ikt = one / F64(kt40)
        igs = one / gs
        d = _abs2(y21r, y21i)
        rr, ri = _div(y11r, y11i, y21r, y21i)
        cvv = c22 * (one / d)
        t1 = rr * c12r
        t2 = ri * c12i
        rc = t1 + t2
        t3 = two * rc
        t4 = _abs2(rr, ri) * c22
        cii = (c11 - t3) + t4
        if not cvv > 0.0:
            t = cii * ikt
            return dict(nf=one + t * igs, fmin=one, rn=F64(0.0), yopt=complex(0.0, 0.0), cvv_positive=False)
        t5 = rr * c22
        t6 = ri * c22
        qr, qi = _div(c12r - t5, t6 - c12i, y21r, y21i)
        icvv = one / cvv
        gcor = (-qr) * icvv
        bcor = qi * icvv
        rn = cvv * ikt
        g2 = gcor * gcor
        b2 = bcor * bcor
        t7 = (g2 + b2) * cvv
        gu = (cii - t7) * ikt
        t8 = gu * (one / rn)
        arg = t8 + g2
        if arg < 0.0:
            arg = F64(0.0)
        gopt = np.sqrt(arg)
        gsc = gs + gcor
        t9 = gsc * gsc
        t10 = rn * (t9 + b2)
        t11 = two * rn
        return dict(nf=one + (gu + t10) * igs, fmin=one + t11 * (gcor + gopt), rn=rn, yopt=complex(gopt, -bcor),
                    cvv_positive=True)


def solve(G, C, w, port_eq, z0, src_a, src_b, psd, eps=EPS):
    """One system at one angular frequency -> dict(flags, x [P][n], y [P][P], cy [P][P], nf, fmin, rn, yopt (P == 2),
    log, cvv_positive)"""
    G = np.asarray(G, dtype=F64)
    C = np.asarray(C, dtype=F64)
    n, P, S = G.shape[0], len(port_eq), len(src_a)
    with np.errstate(all="ignore"):
        Ai = F64(w) * C
    rhs = np.zeros((P, n))
    for i in range(P):
        rhs[i, port_eq[i]] = 1.0
    fl, xr, xi, log = spref.solve_multi(np.ascontiguousarray(G.T), np.ascontiguousarray(Ai.T), rhs, np.zeros((P, n)), eps)
    Yr, Yi = np.zeros((P, P)), np.zeros((P, P))
    Cr, Ci = np.zeros((P, P)), np.zeros((P, P))
    if not fl:
        with np.errstate(all="ignore"):
            for i in range(P):
                for j in range(P):
                    Yr[i, j] = -xr[i][port_eq[j]]
                    Yi[i, j] = -xi[i][port_eq[j]]
            tr = np.zeros((P, S))
            ti = np.zeros((P, S))
            for i in range(P):
                for s in range(S):
                    tr[i, s], ti[i, s] = _transfer(xr[i], xi[i], int(src_a[s]), int(src_b[s]))
            p = np.asarray(psd, dtype=F64)
            for i in range(P):
                for j in range(i, P):
                    a = tr[i] * tr[j]
                    b = ti[i] * ti[j]
                    qre = (a + b) * p
                    re = F64(0.0)
                    for s in range(S):
                        re = re + qre[s]
                    Cr[i, j] = re
                    if i != j:
                        a = ti[i] * tr[j]
                        b = tr[i] * ti[j]
                        qim = (a - b) * p
                        im = F64(0.0)
                        for s in range(S):
                            im = im + qim[s]
                        Ci[i, j] = im
                        Cr[j, i] = re
                        Ci[j, i] = -im
    res = dict(flags=fl, log=log, cvv_positive=None)
    res["x"] = np.zeros((P, n), dtype=np.complex128)
    res["x"].real, res["x"].imag = xr, xi
    for key, re, im in (("y", Yr, Yi), ("cy", Cr, Ci)):
        res[key] = np.zeros((P, P), dtype=np.complex128)
        res[key].real, res[key].imag = re, im
    if P == 2:
        if fl:
            res.update(nf=0.0, fmin=0.0, rn=0.0, yopt=complex(0.0, 0.0))
        else:
            res.update(two_port(res["y"][0, 0], res["y"][1, 0], Cr[0, 0], Cr[1, 1], res["cy"][0, 1], F64(1.0) / F64(z0[0])))
    return res


def sweep(G, C, omega, port_eq, z0, src_a, src_b, psd, eps=EPS):
    """-> dict(flags (OR-ed), per_f, x [F][P][n], y, cy [F][P][P], logs, cvv_positive [F]) and for P == 2 nf, fmin, rn
    [F], yopt complex [F]"""
    F, n, P = len(omega), np.asarray(G).shape[0], len(port_eq)
    res = dict(flags=0, per_f=[], logs=[], cvv_positive=[], x=np.zeros((F, P, n), dtype=np.complex128),
               y=np.zeros((F, P, P), dtype=np.complex128), cy=np.zeros((F, P, P), dtype=np.complex128))
    if P == 2:
        res.update(nf=np.zeros(F), fmin=np.zeros(F), rn=np.zeros(F), yopt=np.zeros(F, dtype=np.complex128))
    for f, w in enumerate(omega):
        r = solve(G, C, w, port_eq, z0, src_a, src_b, psd, eps)
        res["flags"] |= r["flags"]
        res["per_f"].append(r["flags"])
        res["logs"].append(r["log"])
        res["cvv_positive"].append(r["cvv_positive"])
        for key in ("x", "y", "cy"):
            res[key][f].real, res[key][f].imag = r[key].real, r[key].imag     # parts set separately: keeps a -0.0
        if P == 2:
            for key in ("nf", "fmin", "rn"):
                res[key][f] = r[key]
            res["yopt"][f] = r["yopt"]
    return res
