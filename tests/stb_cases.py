"""The seeded inputs of the loop-gain kernel tests, shared by the CPU test (tests/stb_reference.py against the
host-compiled ac_stb.hpp, tests/test_stb_cpu.py) and the GPU test (kernels against the reference,
tests/test_stb_kernels_gpu.py).

A case is a batch of B = 3 systems (G, C) of one size n that share one probe (x, y, k), as the instances of a circuit
do.  Random cases are dense complex-normal matrices: nearly every column exchanges rows.  Sizes: the smallest system
that has x, y and k (3), the ends of both kernel shapes and of the packed kernel's register classes (5, 31, 32, 33,
63).  Four angular frequencies, w = 0 among them; the margins of the random cases walk their T on an arbitrary
increasing grid (FREQS_HZ), which is ordinary data for the walk.  Beside them: a chain of three transconductor-RC
stages closed through the probe (three equal poles: closed forms for the margins), an LC tank that is singular at
exactly one frequency, and a resistive loop whose den is exactly zero.
"""
import numpy as np

OMEGA = np.array([1.0, 0.0, 2.5, 0.375])
FREQS_HZ = np.array([1.0, 2.0, 3.5, 4.0])                     # the grid the margins of a random case are walked on
B = 3
SIZES = (3, 5, 31, 32, 33, 63)


def case(n, seed=20261019):
    """-> dict(n, G [B][n][n], C [B][n][n], probe (x, y, k))"""
    rng = np.random.default_rng([seed, n])
    G = rng.standard_normal((B, n, n))
    C = rng.standard_normal((B, n, n))
    x, y, k = (int(v) for v in rng.permutation(n)[:3])
    if n == 63:
        x, y, k = 62, 0, 31                                   # the last row, the first, one in the middle
    return dict(n=n, G=G, C=C, probe=(x, y, k))


# ---- three equal poles: v1 = -(gm / Y) vy, v2 = -(gm / Y) v1, vx = -(gm / Y) v2 with Y = g + s c at every stage (the
# last stage's conductance is split: g - ga on the driving node x, ga on the receiving node y).  Unknowns v1, v2, x, y, k.
CHAIN_G, CHAIN_C = 1e-3, 1e-9                                 # pole p = g / c = 1e6 rad/s
CHAIN_GAIN = (1.5, 1.2, 1.9)                                  # gm / g per instance: A0 = 3.375, 1.728, 6.859 (all < 8)
CHAIN_GA = (0.25e-3, 0.0, 0.5e-3)
CHAIN_PROBE = (2, 3, 4)


def chain(gain=CHAIN_GAIN, ga=CHAIN_GA, reverse=0.0):
    """reverse: a conductance from y back to v2 added to make the loop bilateral (orientation test)"""
    nb = len(gain)
    G = np.zeros((nb, 5, 5))
    C = np.zeros((nb, 5, 5))
    for b in range(nb):
        gm = gain[b] * CHAIN_G
        G[b, 0, 0] = G[b, 1, 1] = CHAIN_G
        G[b, 2, 2] = CHAIN_G - ga[b]
        G[b, 3, 3] = ga[b]
        G[b, 0, 3] = G[b, 1, 0] = G[b, 2, 1] = gm             # each stage's transconductor
        G[b, 2, 4], G[b, 3, 4] = 1.0, -1.0                    # the branch current leaves x and enters y
        G[b, 4, 2], G[b, 4, 3] = 1.0, -1.0                    # vx - vy = V
        if reverse:
            G[b, 3, 3] += reverse
            G[b, 1, 1] += reverse
            G[b, 3, 1] -= reverse
            G[b, 1, 3] -= reverse
        C[b, 0, 0] = C[b, 1, 1] = C[b, 2, 2] = CHAIN_C
    return dict(n=5, G=G, C=C, probe=CHAIN_PROBE)


def chain_freqs(per_decade=10):
    """Hz, from p / 100 to 100 p"""
    p = CHAIN_G / CHAIN_C / (2.0 * np.pi)
    return p * 10.0 ** (np.arange(4 * per_decade + 1) / per_decade - 2.0)


def chain_closed_form(gain):
    """-> (PM degrees, fc Hz, GM dB, f180 Hz) of A0 / (1 + s / p)^3"""
    a0, p = gain ** 3, CHAIN_G / CHAIN_C
    u = np.sqrt(a0 ** (2.0 / 3.0) - 1.0)
    return 180.0 - 3.0 * np.degrees(np.arctan(u)), u * p / (2 * np.pi), 20.0 * np.log10(8.0 / a0), np.sqrt(3.0) * p / (2 * np.pi)


# ---- singular at exactly one frequency: a resistive loop (x, y, k) beside an LC tank [[j w, 1], [1, -j w]] whose
# elimination leaves an exact zero at w == 1.0
TANK_OMEGA = np.array([0.25, 1.0, 0.0, 2.0])
TANK_FAILS = (False, True, False, False)


def tank():
    G = np.zeros((5, 5))
    C = np.zeros((5, 5))
    G[:3, :3] = [[1.0, 0.0, 1.0], [2.0, 1.0, -1.0], [1.0, -1.0, 0.0]]
    G[3, 4] = G[4, 3] = 1.0
    C[3, 3], C[4, 4] = 1.0, -1.0
    return dict(n=5, G=G[None], C=C[None], probe=(0, 1, 2))


# ---- den exactly zero: gx = 1, gy = 3, gm = -2 gives Tv = -3, Ti = 1, Tv + Ti + 2 = 0 with vx = 1.5, vy = 0.5,
# ib = 0.5, every intermediate of the elimination a dyadic number; the fourth unknown is a decoupled RC
def zero_den():
    G = np.zeros((4, 4))
    C = np.zeros((4, 4))
    G[:3, :3] = [[1.0, 0.0, 1.0], [-2.0, 3.0, -1.0], [1.0, -1.0, 0.0]]
    G[3, 3] = 1.0
    C[3, 3] = 1.0
    return dict(n=4, G=G[None], C=C[None], probe=(0, 1, 2))


# Margins of the host-compiled header and of the device (their C library's atan2 / log10 / log / exp) against the
# reference (numpy's): |a - b| <= MARGIN_BOUND * max(|b|, 1) in degrees, Hz and dB.  Measured largest over every case
# of this file: 2.0e-15 on the CPU (host-compiled header, n = 31), 5.2e-15 on the GPU (both kernels, the chain), and
# 5.9e-16 on the GPU through the engine on the golden loops.  The bound is not ten times those figures, because they
# say what these two C libraries do on these inputs, not what another may: it allows four functions off by up to 4 ulp
# each (4.4e-16 relative); the unwrapped phase reaches a few pi and is scaled by 180 / pi, so that is below 1e-12
# degrees; the interpolation weight t = g / (g - g') amplifies an error of g by |g| / |g - g'|, below 1e3 on these
# cases, which gives 1e-12 relative in t and in the frequencies; ten times that.  It is 2000 times the largest measured
# and 7e5 times below the smallest interpolation error of DESIGN.md 8g (7.3e-6): no wrong unwrap or weight hides in it.
MARGIN_BOUND = 1e-11


def margins_close(got, want, bound=None):
    """-> largest |got - want| / max(|want|, 1), NaN only where both are; asserts the bound"""
    bound = MARGIN_BOUND if bound is None else bound
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    dev = float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0))) if ok.any() else 0.0
    assert dev <= bound, (got, want, dev)
    return dev


_cache = {}


def inputs(key):
    """key: a size of SIZES, "chain", "tank" or "zero_den" -> (case, omega [F], freqs_hz [F])"""
    if key == "chain":
        f = chain_freqs()
        return chain(), 2.0 * np.pi * f, f
    if key == "tank":
        return tank(), TANK_OMEGA, FREQS_HZ
    if key == "zero_den":
        return zero_den(), OMEGA, FREQS_HZ
    return case(key), OMEGA, FREQS_HZ


def reference(key):
    """stb_reference of every system of a case, computed once
    -> [dict(flags, per_f, t, x, logs, margins [4], found) per system]"""
    import stb_reference as sref
    if key not in _cache:
        c, omega, fhz = inputs(key)
        out = []
        for b in range(len(c["G"])):
            r = sref.solve_sweep(c["G"][b], c["C"][b], omega, c["probe"])
            r["margins"], r["found"] = sref.margins(fhz, r["t"])
            out.append(r)
        _cache[key] = out
    return _cache[key]
