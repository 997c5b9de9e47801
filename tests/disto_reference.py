"""An independent statement of include/csim.h "Distortion analysis" for the tests of the distortion kernels: single-tone
HD2 and HD3 of (G + j w C) with level-1 MOSFETs by a Volterra series, three solves per frequency.

Written from the specification, not from the engine's sources (it neither includes, parses nor calls ac_disto.hpp):

  coefficients  seven per device at the operating point: c_gg, c_gd, c_dd, c_ggg, c_ggd, c_gdd, c_ddd (coef())
  order 1       A(w) x1 = J
  order 2       per device Ug = x1[g] - x1[s], Ud = x1[d] - x1[s], ground = (0, 0);
                I2 = 0.5 (((0.5 c_gg) (Ug Ug) + c_gd (Ug Ud)) + (0.5 c_dd) (Ud Ud));
                rhs2 starts at +0.0, the devices in ascending order subtract I2 at d, then add it at s; A(2.0 w) x2 = rhs2
  order 3       a = (((c_ggg / 6.0) (GG Ug) + (0.5 c_ggd) (GG Ud)) + (0.5 c_gdd) (Ug DD)) + (c_ddd / 6.0) (DD Ud),
                b = (c_gg (Ug Ug2) + c_gd ((Ug Ud2) + (Ud Ug2))) + c_dd (Ud Ud2), I3 = 0.25 a + 0.5 b; A(3.0 w) x3 = rhs3
  outputs       v_k = x_k[out_p] - x_k[out_m], |z| = sqrt(re re + im im), HD_k = |v_k| / |v_1|, +0.0 where |v_1| == 0
  failed LU     the failed order and every higher one are +0.0, flag 0x4; all three factorisations are attempted

Every solve is ac_reference.solve().  As there, real and imaginary parts live on separate float64 values and every IEEE
operation of the specification is one numpy operation on them.
"""
import numpy as np

import ac_reference

NCOEF = 7
GG, GD, DD, GGG, GGD, GDD, DDD = range(NCOEF)
F64 = np.float64


def mos_region(isP, Vth, K, lam, Vd, Vg, Vs):
    """-> (p, Vgs, Vds, Vov, factor, region): region "off" | "clamped" | "triode" | "sat", decided by the comparisons
    of the level-1 model (src/element.cpp:207-256)"""
    p = F64(-1.0 if isP else 1.0)
    Vgs = p * (F64(Vg) - F64(Vs))
    Vds = p * (F64(Vd) - F64(Vs))
    Vov = Vgs - F64(Vth)
    factor = F64(1.0) + F64(lam) * Vds
    if not (Vgs > Vth and Vds >= 0.0):
        return p, Vgs, Vds, Vov, factor, "off"
    if factor < 0.0:
        return p, Vgs, Vds, Vov, factor, "clamped"
    return p, Vgs, Vds, Vov, factor, ("triode" if Vds < Vov else "sat")


def coef(isP, Vth, K, lam, Vd, Vg, Vs):
    """the seven coefficients of one device -> float64 [7]"""
    K, lam = F64(K), F64(lam)
    c = np.zeros(NCOEF)
    with np.errstate(all="ignore"):
        p, Vgs, Vds, Vov, factor, region = mos_region(isP, Vth, K, lam, Vd, Vg, Vs)
        if region in ("off", "clamped"):
            return c
        gg = gd = dd = F64(0.0)
        if region == "triode":
            t1 = K * factor
            t2 = (K * Vds) * lam
            gd = t1 + t2
            t3 = F64(2.0) * ((K * (Vov - Vds)) * lam)
            t4 = K * factor
            dd = t3 - t4
            c[GDD] = F64(2.0) * (K * lam)
            c[DDD] = F64(-3.0) * (K * lam)
        else:
            gg = K * factor
            gd = (K * Vov) * lam
            c[GGD] = K * lam
        c[GG] = p * gg
        c[GD] = p * gd
        c[DD] = p * dd
    return c


def mos_current(isP, Vth, K, lam, Vd, Vg, Vs):
    """the level-1 drain current (drain -> source) and its first derivatives in Ug = Vg - Vs and Ud = Vd - Vs
    (src/element.cpp:207-270; the off-conductance is left out: it is linear) -> (Ids, dI/dUg, dI/dUd)"""
    p, Vgs, Vds, Vov, factor, region = mos_region(isP, Vth, K, lam, Vd, Vg, Vs)
    if region in ("off", "clamped"):
        return F64(0.0), F64(0.0), F64(0.0)
    K, lam = F64(K), F64(lam)
    if region == "triode":
        ids0 = K * (Vov * Vds - F64(0.5) * Vds * Vds)
        gds0 = K * (Vov - Vds)
        gm0 = K * Vds
    else:
        ids0 = F64(0.5) * K * Vov * Vov
        gds0 = F64(0.0)
        gm0 = K * Vov
    return p * (ids0 * factor), gm0 * factor, gds0 * factor + ids0 * lam


# ---- complex values as (re, im) pairs of float64

def _mul(a, b):
    t1 = a[0] * b[0]
    t2 = a[1] * b[1]
    t3 = a[0] * b[1]
    t4 = a[1] * b[0]
    return t1 - t2, t3 + t4


def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _scale(s, a):
    return s * a[0], s * a[1]


def _at(xr, xi, eq):
    if eq < 0:
        return F64(0.0), F64(0.0)
    return xr[eq], xi[eq]


def _u(xr, xi, a, s):
    return _sub(_at(xr, xi, a), _at(xr, xi, s))


def current2(c, Ug, Ud):
    t = _scale(F64(0.5) * c[GG], _mul(Ug, Ug))
    t = _add(t, _scale(c[GD], _mul(Ug, Ud)))
    t = _add(t, _scale(F64(0.5) * c[DD], _mul(Ud, Ud)))
    return _scale(F64(0.5), t)


def current3(c, Ug, Ud, Ug2, Ud2):
    gg, dd = _mul(Ug, Ug), _mul(Ud, Ud)
    a = _scale(c[GGG] / F64(6.0), _mul(gg, Ug))
    a = _add(a, _scale(F64(0.5) * c[GGD], _mul(gg, Ud)))
    a = _add(a, _scale(F64(0.5) * c[GDD], _mul(Ug, dd)))
    a = _add(a, _scale(c[DDD] / F64(6.0), _mul(dd, Ud)))
    b = _scale(c[GG], _mul(Ug, Ug2))
    b = _add(b, _scale(c[GD], _add(_mul(Ug, Ud2), _mul(Ud, Ug2))))
    b = _add(b, _scale(c[DD], _mul(Ud, Ud2)))
    return _add(_scale(F64(0.25), a), _scale(F64(0.5), b))


def _abs(z):
    t1 = z[0] * z[0]
    t2 = z[1] * z[1]
    return np.sqrt(t1 + t2)


def solve(G, C, J, w, dev_d, dev_g, dev_s, coefs, out, eps=ac_reference.EPS):
    """One system at one angular frequency.  G, C [n][n]; J [n] complex; devices [M] with coefs [M][7]; out = (out_p,
    out_m).  -> (flags, [flags of order 1, 2, 3 as factored], x complex [3][n], hd [2], [PivotLog per order])"""
    G = np.asarray(G, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    J = np.asarray(J, dtype=np.complex128)
    coefs = np.asarray(coefs, dtype=np.float64).reshape(len(dev_d), NCOEF)
    n = len(J)
    xr, xi = np.zeros((3, n)), np.zeros((3, n))
    per_order, logs = [], []
    failed = False
    with np.errstate(all="ignore"):
        for k in (1, 2, 3):
            Ai = (F64(k) * F64(w)) * C
            if k == 1:
                br, bi = J.real.copy(), J.imag.copy()
            else:
                br, bi = np.zeros(n), np.zeros(n)
                for m in range(len(dev_d)):
                    d, g, s = int(dev_d[m]), int(dev_g[m]), int(dev_s[m])
                    Ug, Ud = _u(xr[0], xi[0], g, s), _u(xr[0], xi[0], d, s)
                    if k == 2:
                        I = current2(coefs[m], Ug, Ud)
                    else:
                        I = current3(coefs[m], Ug, Ud, _u(xr[1], xi[1], g, s), _u(xr[1], xi[1], d, s))
                    if d >= 0:
                        br[d] = br[d] - I[0]
                        bi[d] = bi[d] - I[1]
                    if s >= 0:
                        br[s] = br[s] + I[0]
                        bi[s] = bi[s] + I[1]
            fl, yr, yi, log = ac_reference.solve(G, Ai, br, bi, eps)
            per_order.append(fl)
            logs.append(log)
            failed = failed or fl != 0
            if not failed:
                xr[k - 1], xi[k - 1] = yr, yi
        v = [_abs(_u(xr[k], xi[k], out[0], out[1])) for k in range(3)]
        hd = np.zeros(2)
        if v[0] != 0.0:
            hd[0] = v[1] / v[0]
            hd[1] = v[2] / v[0]
    x = np.zeros((3, n), dtype=np.complex128)
    x.real, x.imag = xr, xi
    flags = per_order[0] | per_order[1] | per_order[2]
    return flags, per_order, x, hd, logs


def solve_sweep(G, C, J, omega, dev_d, dev_g, dev_s, coefs, out, eps=ac_reference.EPS):
    """-> dict(flags (OR-ed), per_f [F][3], h complex [F][3][n], hd [F][2], logs)"""
    F, n = len(omega), len(J)
    res = dict(flags=0, per_f=[], h=np.zeros((F, 3, n), dtype=np.complex128), hd=np.zeros((F, 2)), logs=[])
    for f, w in enumerate(omega):
        fl, per_order, x, hd, logs = solve(G, C, J, w, dev_d, dev_g, dev_s, coefs, out, eps)
        res["flags"] |= fl
        res["per_f"].append(per_order)
        res["h"][f] = x
        res["hd"][f] = hd
        res["logs"].append(logs)
    return res
