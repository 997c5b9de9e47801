"""An independent statement of include/csim.h "Intermodulation analysis" for the tests of the intermodulation kernels:
two-tone IM2+, IM2- and IM3 of (G + j w C) with level-1 MOSFETs by a Volterra series, six solves per tone pair.

Written from the specification, not from the engine's sources (it neither includes, parses nor calls ac_imd.hpp).  The
coefficients, the complex helpers and the second-harmonic current are those of tests/disto_reference.py.

  pair          of a solution x and a device: (Ug, Ud) = (x[g] - x[s], x[d] - x[s]), ground = (0, 0); * the conjugate
  Q(A, B)       0.5 ((c_gg (Ag Bg) + c_gd ((Ag Bd) + (Ad Bg))) + c_dd (Ad Bd))
  T(A, A, B)    (((c_ggg (GG Bg) + c_ggd ((GG Bd) + 2.0 (GD Bg))) + c_gdd (2.0 (GD Bd) + (DD Bg))) + c_ddd (DD Bd)) / 6.0
  solves        k  frequency        right-hand side (devices ascending, minus at d, then plus at s, from +0.0)
                0  w1               J1
                1  w2               J2
                2  w1 + w2          Q(Ua, Ub)
                3  w1 - w2          Q(Ua, Ub*)
                4  2.0 w1           I2 of the distortion analysis on Ua
                5  (2.0 w1) - w2    (0.75 T(Ua, Ua, Ub*) + Q(Ua, Vd)) + Q(Ub*, Vh), Vd and Vh the pairs of x3 and x4
  outputs       v_k = x_k[out_p] - x_k[out_m]; IM2+ = |v2| / |v0|, IM2- = |v3| / |v0|, IM3 = |v5| / |v0|, +0.0 where
                |v0| == 0
  failed LU     the failed solve and every later one are +0.0, flag 0x4; all six factorisations are attempted

Every solve is ac_reference.solve(); every IEEE operation of the specification is one numpy operation.
"""
import numpy as np

import ac_reference
from disto_reference import DD, DDD, F64, GD, GDD, GG, GGD, GGG, NCOEF, _abs, _add, _mul, _scale, _u, current2

NSOLVE = 6


def _conj(a):
    return a[0], -a[1]


def q_form(c, Ag, Ad, Bg, Bd):
    t = _scale(c[GG], _mul(Ag, Bg))
    t = _add(t, _scale(c[GD], _add(_mul(Ag, Bd), _mul(Ad, Bg))))
    t = _add(t, _scale(c[DD], _mul(Ad, Bd)))
    return _scale(F64(0.5), t)


def t_form(c, Ag, Ad, Bg, Bd):
    gg, gd, dd = _mul(Ag, Ag), _mul(Ag, Ad), _mul(Ad, Ad)
    t = _scale(c[GGG], _mul(gg, Bg))
    t = _add(t, _scale(c[GGD], _add(_mul(gg, Bd), _scale(F64(2.0), _mul(gd, Bg)))))
    t = _add(t, _scale(c[GDD], _add(_scale(F64(2.0), _mul(gd, Bd)), _mul(dd, Bg))))
    t = _add(t, _scale(c[DDD], _mul(dd, Bd)))
    return t[0] / F64(6.0), t[1] / F64(6.0)


def frequencies(w1, w2):
    w1, w2 = F64(w1), F64(w2)
    wh = F64(2.0) * w1
    return [w1, w2, w1 + w2, w1 - w2, wh, wh - w2]


def current(k, c, d, g, s, xr, xi):
    """drain current of one device in solve k (2 .. 5) from the solutions so far"""
    Uag, Uad = _u(xr[0], xi[0], g, s), _u(xr[0], xi[0], d, s)
    if k == 4:
        return current2(c, Uag, Uad)
    Ubg, Ubd = _u(xr[1], xi[1], g, s), _u(xr[1], xi[1], d, s)
    if k == 2:
        return q_form(c, Uag, Uad, Ubg, Ubd)
    Cbg, Cbd = _conj(Ubg), _conj(Ubd)
    if k == 3:
        return q_form(c, Uag, Uad, Cbg, Cbd)
    t = _scale(F64(0.75), t_form(c, Uag, Uad, Cbg, Cbd))
    t = _add(t, q_form(c, Uag, Uad, _u(xr[3], xi[3], g, s), _u(xr[3], xi[3], d, s)))
    return _add(t, q_form(c, Cbg, Cbd, _u(xr[4], xi[4], g, s), _u(xr[4], xi[4], d, s)))


def solve(G, C, J1, J2, w1, w2, dev_d, dev_g, dev_s, coefs, out, eps=ac_reference.EPS):
    """One system at one tone pair.  G, C [n][n]; J1, J2 [n] complex (J2 None: J1); devices [M] with coefs [M][7];
    out = (out_p, out_m).  -> (flags, [flags of solve 0 .. 5 as factored], x complex [6][n], im [3])"""
    G = np.asarray(G, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    J1 = np.asarray(J1, dtype=np.complex128)
    J2 = J1 if J2 is None else np.asarray(J2, dtype=np.complex128)
    coefs = np.asarray(coefs, dtype=np.float64).reshape(len(dev_d), NCOEF)
    n = len(J1)
    xr, xi = np.zeros((NSOLVE, n)), np.zeros((NSOLVE, n))
    per_solve = []
    failed = False
    with np.errstate(all="ignore"):
        for k, wk in enumerate(frequencies(w1, w2)):
            Ai = wk * C
            if k < 2:
                J = J1 if k == 0 else J2
                br, bi = J.real.copy(), J.imag.copy()
            else:
                br, bi = np.zeros(n), np.zeros(n)
                for m in range(len(dev_d)):
                    d, g, s = int(dev_d[m]), int(dev_g[m]), int(dev_s[m])
                    I = current(k, coefs[m], d, g, s, xr, xi)
                    if d >= 0:
                        br[d] = br[d] - I[0]
                        bi[d] = bi[d] - I[1]
                    if s >= 0:
                        br[s] = br[s] + I[0]
                        bi[s] = bi[s] + I[1]
            fl, yr, yi, _ = ac_reference.solve(G, Ai, br, bi, eps)
            per_solve.append(fl)
            failed = failed or fl != 0
            if not failed:
                xr[k], xi[k] = yr, yi
        v = [_abs(_u(xr[k], xi[k], out[0], out[1])) for k in range(NSOLVE)]
        im = np.zeros(3)
        if v[0] != 0.0:
            im[0] = v[2] / v[0]
            im[1] = v[3] / v[0]
            im[2] = v[5] / v[0]
    x = np.zeros((NSOLVE, n), dtype=np.complex128)
    x.real, x.imag = xr, xi
    flags = 0
    for fl in per_solve:
        flags |= fl
    return flags, per_solve, x, im


def solve_sweep(G, C, J1, J2, omega1, omega2, dev_d, dev_g, dev_s, coefs, out, eps=ac_reference.EPS):
    """-> dict(flags (OR-ed), per_f [F][6], h complex [F][6][n], im [F][3])"""
    F, n = len(omega1), len(J1)
    res = dict(flags=0, per_f=[], h=np.zeros((F, NSOLVE, n), dtype=np.complex128), im=np.zeros((F, 3)))
    for f in range(F):
        fl, per_solve, x, im = solve(G, C, J1, J2, omega1[f], omega2[f], dev_d, dev_g, dev_s, coefs, out, eps)
        res["flags"] |= fl
        res["per_f"].append(per_solve)
        res["h"][f] = x
        res["im"][f] = im
    return res
