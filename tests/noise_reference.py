"""An independent statement of include/csim.h "Noise analysis" for the tests of the noise kernels: output noise of
(G + j w C) by one adjoint solve per frequency.

Written from the specification, not from the engine's sources (it neither includes, parses nor calls ac_noise.hpp):

  adjoint      A^T y = d, A = G + j (w C) with w C one product, d real: +1 at out_p, -1 at out_m (-1: ground, no
               entry); solved by ac_reference.solve() on the transposed planes
  generator s  z = y[a] - y[b], ground = (0, 0);  contrib[s] = (z.re z.re + z.im z.im) psd[s]
  onoise       0.0 + contrib[0] + contrib[1] + ..., ascending
  gain         ("v", k): y[k];  ("i", a, b): y[a] - y[b]   (an I source between (p, m) passes a = m, b = p)
  failed LU    onoise, every contrib and the gain are +0.0, flag 0x4

As in ac_reference.py every IEEE operation of the specification is one numpy operation on float64 values.
"""
import numpy as np

import ac_reference

K_BOLTZMANN = 1.380649e-23


def kt4(temp_k):
    return np.float64(4.0) * np.float64(K_BOLTZMANN) * np.float64(temp_k)


def _at(yr, yi, eq):
    if eq < 0:
        return np.float64(0.0), np.float64(0.0)
    return yr[eq], yi[eq]


def _diff(yr, yi, a, b):
    ar, ai = _at(yr, yi, a)
    br, bi = _at(yr, yi, b)
    return ar - br, ai - bi


def solve(G, C, w, out, src_a, src_b, psd, gain_in=None, eps=ac_reference.EPS):
    """One system at one angular frequency.  G, C [n][n]; out = (out_p, out_m); src_a, src_b, psd [S].
    -> (flags, onoise, contrib [S], gain complex or None, y complex [n], PivotLog)"""
    G = np.asarray(G, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    n = G.shape[0]
    with np.errstate(all="ignore"):
        Ai = np.float64(w) * C
    d = np.zeros(n)
    d[out[0]] = 1.0
    if out[1] >= 0:
        d[out[1]] = -1.0
    fl, yr, yi, log = ac_reference.solve(G.T, Ai.T, d, np.zeros(n), eps)
    S = len(src_a)
    contrib = np.zeros(S)
    onoise = np.float64(0.0)
    with np.errstate(all="ignore"):
        for s in range(S):
            if not fl:
                zr, zi = _diff(yr, yi, int(src_a[s]), int(src_b[s]))
                t1 = zr * zr
                t2 = zi * zi
                contrib[s] = (t1 + t2) * np.float64(psd[s])
            onoise = onoise + contrib[s]
        gain = None
        if gain_in is not None:
            if fl:
                gain = complex(0.0, 0.0)
            elif gain_in[0] == "v":
                gr, gi = _at(yr, yi, int(gain_in[1]))
                gain = complex(gr, gi)
            else:
                gr, gi = _diff(yr, yi, int(gain_in[1]), int(gain_in[2]))
                gain = complex(gr, gi)
    y = np.zeros(n, dtype=np.complex128)
    y.real, y.imag = yr, yi
    return fl, float(onoise), contrib, gain, y, log


def solve_sweep(G, C, omega, out, src_a, src_b, psd, gain_in=None, eps=ac_reference.EPS):
    """-> dict(flags (OR-ed), per_f [F], onoise [F], contrib [F][S], gain complex [F] or None, y complex [F][n], logs)"""
    F, n, S = len(omega), np.asarray(G).shape[0], len(src_a)
    res = dict(flags=0, per_f=[], onoise=np.zeros(F), contrib=np.zeros((F, S)),
               gain=np.zeros(F, dtype=np.complex128) if gain_in is not None else None,
               y=np.zeros((F, n), dtype=np.complex128), logs=[])
    for f, w in enumerate(omega):
        fl, on, con, g, y, log = solve(G, C, w, out, src_a, src_b, psd, gain_in, eps)
        res["flags"] |= fl
        res["per_f"].append(fl)
        res["onoise"][f] = on
        res["contrib"][f] = con
        if gain_in is not None:
            res["gain"][f] = g
        res["y"][f] = y
        res["logs"].append(log)
    return res


def generators(rng, n, S):
    """a seeded generator table for an n x n system: terminals in -1 .. n-1 (ground and a == b among them), PSDs of
    the size of thermal noise -> (src_a [S] int32, src_b [S] int32, psd [S])"""
    a = rng.integers(-1, n, S).astype(np.int32)
    b = rng.integers(-1, n, S).astype(np.int32)
    if S >= 2:
        b[S // 2] = a[S // 2]                 # a generator across one node: z = y - y
    if S >= 3:
        a[0] = -1                             # one from ground
    return a, b, 1.6e-20 * rng.uniform(1e-6, 1.0, S)


def adjoint_case(c):
    """an ac_cases case with every system transposed.  The structured kinds place their feature (a tie, a zero or
    threshold column, a NaN) in the matrix that is FACTORED; the noise solve factors A^T, so it is handed A^T as
    its system and meets the feature exactly where the AC solve meets it."""
    out = dict(c)
    out["G"] = np.ascontiguousarray(np.transpose(c["G"], (0, 2, 1)))
    out["C"] = np.ascontiguousarray(np.transpose(c["C"], (0, 2, 1)))
    return out


def setup(kind_index, n, nsys=5, seed=20250117):
    """what goes with the ac_cases case (kind, n), whose systems share one generator table as the instances of a
    circuit do: -> dict(out, src_a, src_b, psd [nsys][S], gain_in).  S takes 0, 1, n, 3n and values between over
    the kinds and sizes."""
    rng = np.random.default_rng([seed, kind_index, n])
    out_p = int(rng.integers(0, n))
    out_m = -1
    if n > 1 and rng.random() < 0.5:
        out_m = int((out_p + 1 + rng.integers(0, n - 1)) % n)
    S = [0, n, 3 * n, int(rng.integers(0, 3 * n + 1)), 1][(kind_index + n) % 5]
    a, b, _ = generators(rng, n, S)
    psd = np.stack([generators(rng, n, S)[2] for _ in range(nsys)]) if S else np.zeros((nsys, 0))
    if rng.random() < 0.5:
        gain_in = ("v", int(rng.integers(0, n)))
    else:
        gain_in = ("i", int(rng.integers(-1, n)), int(rng.integers(-1, n)))
    return dict(out=(out_p, out_m), src_a=a, src_b=b, psd=psd, gain_in=gain_in)
