"""An independent statement of include/csim.h "Loop-gain analysis" for the tests of the loop-gain kernels: T of a
feedback loop by Middlebrook's double injection at a V source in series in the loop, and the margins of a sweep.

Written from the specification, not from the engine's sources (it neither includes, parses nor calls ac_stb.hpp):

  probe       + node equation x (drives), - node equation y (receives), branch equation k
  column 0    A X0 = e_k (the real unit vector at row k);  vx = X0[x], vy = X0[y]
  column 1    A X1 = e_x (+1.0 at row x: `Iinj 0 <+node> AC 1`);  ib = X1[k]
  loop gain   a = 1.0 - ib, b = 1.0 + ib;  num = -(vx a) - (vy ib);  den = (vy b) - (vx ib);  T = num / den
  failures    A fails, or den == 0 exactly: T = +0.0 + 0.0j, flag 0x4
  margins     margins(): the walk over the frequencies of one instance

Every solve is ac_reference.solve(): pivoting never looks at a right-hand side, so each column is the single-RHS solve.
As there, real and imaginary parts live on separate float64 values and every IEEE operation of the specification is
one numpy operation on them.
"""
import numpy as np

import ac_reference

F64 = np.float64
PI = F64(3.14159265358979323846)
LU_TINY_PIVOT = 4
FOUND_UNITY, FOUND_PHASE = 1, 2


def _mul(a, b):
    t1 = a[0] * b[0]
    t2 = a[1] * b[1]
    t3 = a[0] * b[1]
    t4 = a[1] * b[0]
    return t1 - t2, t3 + t4


def _div(a, p):
    t1 = p[0] * p[0]
    t2 = p[1] * p[1]
    inv = F64(1.0) / (t1 + t2)
    t3 = a[0] * p[0]
    t4 = a[1] * p[1]
    t5 = a[1] * p[0]
    t6 = a[0] * p[1]
    return (t3 + t4) * inv, (t5 - t6) * inv


def loop_gain(vx, vy, ib, failed=False):
    """vx, vy, ib as (re, im) float64 pairs -> (flags, (re, im))"""
    with np.errstate(all="ignore"):
        a = (F64(1.0) - ib[0], F64(0.0) - ib[1])
        b = (F64(1.0) + ib[0], F64(0.0) + ib[1])
        p1 = _mul(vx, a)
        p2 = _mul(vy, ib)
        num = (-p1[0] - p2[0], -p1[1] - p2[1])
        p3 = _mul(vy, b)
        p4 = _mul(vx, ib)
        den = (p3[0] - p4[0], p3[1] - p4[1])
        if failed or (den[0] == 0.0 and den[1] == 0.0):
            return LU_TINY_PIVOT, (F64(0.0), F64(0.0))
        return 0, _div(num, den)


def solve(G, C, w, probe, eps=ac_reference.EPS):
    """One system at one angular frequency.  G, C [n][n]; probe = (x, y, k).
    -> (flags, T complex, X complex [2][n], [PivotLog per column])"""
    G = np.asarray(G, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    n = G.shape[0]
    x, y, k = probe
    with np.errstate(all="ignore"):
        Ai = F64(w) * C
        X = np.zeros((2, n), dtype=np.complex128)
        flags, logs = 0, []
        for c, row in enumerate((k, x)):
            br = np.zeros(n)
            br[row] = 1.0
            fl, xr, xi, log = ac_reference.solve(G, Ai, br, np.zeros(n), eps)
            flags |= fl
            logs.append(log)
            X[c].real, X[c].imag = xr, xi
    fl, t = loop_gain((X[0, x].real, X[0, x].imag), (X[0, y].real, X[0, y].imag), (X[1, k].real, X[1, k].imag), flags != 0)
    T = np.zeros(1, dtype=np.complex128)
    T.real, T.imag = t[0], t[1]
    return flags | fl, T[0], X, logs


def solve_sweep(G, C, omega, probe, eps=ac_reference.EPS):
    """-> dict(flags (OR-ed), per_f [F], t complex [F], x complex [F][2][n], logs)"""
    F, n = len(omega), np.asarray(G).shape[0]
    res = dict(flags=0, per_f=[], t=np.zeros(F, dtype=np.complex128), x=np.zeros((F, 2, n), dtype=np.complex128), logs=[])
    for f, w in enumerate(omega):
        fl, T, X, logs = solve(G, C, w, probe, eps)
        res["flags"] |= fl
        res["per_f"].append(fl)
        res["t"][f] = T
        res["x"][f] = X
        res["logs"].append(logs)
    return res


def _interp(f0, f1, t):
    return f0 * np.exp(t * np.log(f1 / f0))


def margins(freqs, T):
    """freqs [F] Hz, strictly increasing and positive; T complex [F] -> (array [4] = PM, fc, GM, f180 (NaN where not
    found), found bits)"""
    freqs = np.asarray(freqs, dtype=np.float64)
    T = np.asarray(T, dtype=np.complex128)
    out = np.full(4, np.nan)
    found = 0
    prev = mp = gp = pp = None
    with np.errstate(all="ignore"):
        for k in range(len(T)):
            re, im = F64(T[k].real), F64(T[k].imag)
            if (re == 0.0 and im == 0.0) or not (np.isfinite(re) and np.isfinite(im)):
                break
            t1 = re * re
            t2 = im * im
            m = t1 + t2
            g = F64(10.0) * np.log10(m)
            if k == 0:
                p = np.arctan2(im, re)
            else:
                q = _mul((re, im), (prev[0], -prev[1]))
                d = np.arctan2(q[1], q[0])
                p = pp + d
                if not found & FOUND_UNITY and mp >= 1.0 and 1.0 > m:
                    u = gp / (gp - g)
                    out[1] = _interp(freqs[k - 1], freqs[k], u)
                    out[0] = F64(180.0) + (pp + u * d) * F64(180.0) / PI
                    found |= FOUND_UNITY
                if not found & FOUND_PHASE and pp > -PI and -PI >= p:
                    u = (pp + PI) / (pp - p)
                    out[3] = _interp(freqs[k - 1], freqs[k], u)
                    out[2] = -(gp + u * (g - gp))
                    found |= FOUND_PHASE
            prev, mp, gp, pp = (re, im), m, g, p
    return out, found
