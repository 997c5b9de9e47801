"""An independent statement of the complex solve of include/csim.h "AC analysis", for the tests of the AC sweep
kernels: (G + j w C) x = J by LU with partial pivoting.

Written from the specification, not from the engine's sources (it neither includes, parses nor calls ac_lu.hpp):

  pivot        the FIRST row with the largest re^2 + im^2 (strict '>'; a NaN candidate is never taken); a NaN
               diagonal keeps the pivot; a maximum below eps^2 fails the solve: zero vector, flag 0x4
  multiplier   l = a conj(p) (1 / (pr^2 + pi^2)), one true division
  elimination  a(i,j) -= l(i) u(j) for j > k and the right-hand side; a row whose multiplier is exactly zero is
               left alone
  back subst.  x(i) = (y(i) - sum over j > i, ascending, of U(i,j) x(j)) / U(i,i), the division as above

Real and imaginary parts live on separate float64 planes and every IEEE operation of the specification is one
numpy operation on them (a product, then a sum or difference as a second operation; nothing is evaluated over a
complex dtype), so no entry ever sees a fused multiply-add or a library's complex multiply / divide.  The
elimination of one column is vectorised over rows and columns (every entry still gets exactly its own
operations); the back substitution is scalar because its sum is ordered.
"""
import numpy as np

LU_TINY_PIVOT = 0x4
EPS = 1e-15


class PivotLog:
    """what one factorisation did: columns that exchanged rows, columns whose maximum was attained by more than
    one candidate row (the first was taken), multipliers that were exactly zero (rows skipped)"""

    def __init__(self):
        self.swaps = 0
        self.ties = 0
        self.skips = 0
        self.failed_at = -1
        self.pivots = []

    def __repr__(self):
        return "PivotLog(swaps=%d, ties=%d, skips=%d, failed_at=%d)" % (self.swaps, self.ties, self.skips, self.failed_at)


def _abs2(re, im):
    a = re * re
    b = im * im
    return a + b


def _div(ar, ai, pr, pi):
    """a / p as a conj(p) (1 / |p|^2)"""
    inv = np.float64(1.0) / _abs2(pr, pi)
    t1 = ar * pr
    t2 = ai * pi
    t3 = ai * pr
    t4 = ar * pi
    return (t1 + t2) * inv, (t3 - t4) * inv


def _mul(ar, ai, br, bi):
    t1 = ar * br
    t2 = ai * bi
    t3 = ar * bi
    t4 = ai * br
    return t1 - t2, t3 + t4


def solve(Ar, Ai, br, bi, eps=EPS):
    """One system.  Ar, Ai [n][n], br, bi [n] float64 -> (flags, xr [n], xi [n], PivotLog)."""
    n = len(br)
    ar = np.empty((n, n + 1), dtype=np.float64)
    ai = np.empty((n, n + 1), dtype=np.float64)
    ar[:, :n], ar[:, n] = Ar, br
    ai[:, :n], ai[:, n] = Ai, bi
    log = PivotLog()
    eps2 = np.float64(eps) * np.float64(eps)
    with np.errstate(all="ignore"):
        for k in range(n):
            v = _abs2(ar[k:, k], ai[k:, k])
            piv, maxv, tied = k, v[0], False
            if maxv == maxv:
                cand = np.where(np.isnan(v), -1.0, v)
                maxv = cand.max()
                piv = k + int(np.argmax(cand))                  # the first of equal maxima
                tied = np.count_nonzero(cand == maxv) > 1
            if maxv < eps2:
                log.failed_at = k
                return LU_TINY_PIVOT, np.zeros(n), np.zeros(n), log
            log.ties += int(tied)
            log.pivots.append(piv)
            if piv != k:
                log.swaps += 1
                ar[[k, piv]] = ar[[piv, k]]
                ai[[k, piv]] = ai[[piv, k]]
            if k + 1 == n:
                break
            lr, li = _div(ar[k + 1:, k], ai[k + 1:, k], ar[k, k], ai[k, k])
            upd = ~((lr == 0.0) & (li == 0.0))
            log.skips += int(np.count_nonzero(~upd))
            rows = k + 1 + np.nonzero(upd)[0]
            if len(rows) == 0:
                continue
            mr, mi = _mul(lr[upd][:, None], li[upd][:, None], ar[k, k + 1:][None, :], ai[k, k + 1:][None, :])
            ar[rows, k + 1:] = ar[rows, k + 1:] - mr
            ai[rows, k + 1:] = ai[rows, k + 1:] - mi
        xr = np.zeros(n)
        xi = np.zeros(n)
        for i in range(n - 1, -1, -1):
            sr, si = ar[i, n], ai[i, n]
            if i + 1 < n:
                pr, pi = _mul(ar[i, i + 1:n], ai[i, i + 1:n], xr[i + 1:], xi[i + 1:])
                for j in range(n - 1 - i):
                    sr = sr - pr[j]
                    si = si - pi[j]
            xr[i], xi[i] = _div(sr, si, ar[i, i], ai[i, i])
    return 0, xr, xi, log


def solve_sweep(G, C, J, omega, eps=EPS):
    """(G + j w C) x = J for every w of omega.  G, C [n][n] float64, J [n] complex.
    -> (flags OR-ed over the sweep, x complex128 [F][n], [flags per frequency], [PivotLog per frequency])"""
    G = np.asarray(G, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    J = np.asarray(J, dtype=np.complex128)
    n = len(J)
    x = np.zeros((len(omega), n), dtype=np.complex128)
    flags, per_f, logs = 0, [], []
    for f, w in enumerate(omega):
        with np.errstate(all="ignore"):
            Ai = np.float64(w) * C
        fl, xr, xi, log = solve(G, Ai, J.real.copy(), J.imag.copy(), eps)
        x[f].real = xr
        x[f].imag = xi
        flags |= fl
        per_f.append(fl)
        logs.append(log)
    return flags, x, per_f, logs


def backward_error(A, x, b):
    """normwise backward error  ||A x - b||inf / (||A||inf ||x||inf + ||b||inf), evaluated in numpy.longdouble"""
    A = np.asarray(A).astype(np.clongdouble)
    x = np.asarray(x).astype(np.clongdouble)
    b = np.asarray(b).astype(np.clongdouble)
    r = np.max(np.abs(A @ x - b))
    den = np.max(np.sum(np.abs(A), axis=1)) * np.max(np.abs(x)) + np.max(np.abs(b))
    return float(r / den) if den > 0 else 0.0
