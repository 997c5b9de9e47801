"""The seeded inputs of the distortion kernel tests, shared by the CPU test (tests/disto_reference.py against the
host-compiled ac_disto_solve(), tests/test_disto_cpu.py) and the GPU test (kernels against the reference,
tests/test_disto_kernels_gpu.py).

A case is a batch of B = 3 systems (G, C, J) of one size n that share one device table, as the instances of a circuit
do, with per-instance coefficients.  Dense complex-normal matrices: nearly every column exchanges rows.  Sizes: the
ends of both kernel shapes and of the packed kernel's register classes (1, 2, 5, 31, 32, 33, 63).  Device counts:
0, 1, 3 at every size and 65 at n = 5, where many devices meet on one node and the kernels' rounds of 64 and of 32
devices are both crossed.  Device tables hold a grounded source, a grounded gate, d == s and g == d.
"""
import numpy as np

OMEGA = np.array([1.0, 0.0, 2.5, 0.375])
B = 3
SIZES = (1, 2, 5, 31, 32, 33, 63)
CASES = [(n, M) for n in SIZES for M in (0, 1, 3)] + [(5, 65)]


def case(n, M, seed=20260119):
    """-> dict(n, M, G [B][n][n], C [B][n][n], J [B][n] complex, dev_d, dev_g, dev_s [M] int32, coef [B][M][7], out)"""
    rng = np.random.default_rng([seed, n, M])
    G = rng.standard_normal((B, n, n))
    C = rng.standard_normal((B, n, n))
    J = rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))
    d = rng.integers(-1, n, M).astype(np.int32)
    g = rng.integers(-1, n, M).astype(np.int32)
    s = rng.integers(-1, n, M).astype(np.int32)
    if M >= 1:
        d[0], g[0], s[0] = 0, n - 1, -1                       # grounded source
    if M >= 3:
        d[1], s[1] = n - 1, n - 1                             # d == s: subtracts, then adds, at one entry
        d[2], g[2] = 0, 0                                     # diode-connected: g == d
    if M >= 8:
        d[3:M:2] = 0                                          # every other device has its drain on equation 0 ...
        s[4:M:4] = 0                                          # ... and some their source
        g[5] = -1                                             # a grounded gate
        d[7] = -1                                             # a grounded drain
    coef = rng.standard_normal((B, M, 7))
    out_p = int(rng.integers(0, n))
    out_m = -1 if n == 1 or rng.random() < 0.5 else int((out_p + 1 + rng.integers(0, n - 1)) % n)
    return dict(n=n, M=M, G=G, C=C, J=J, dev_d=d, dev_g=g, dev_s=s, coef=coef, out=(out_p, out_m))


# The LC tank: A(w) = [[j w, 1], [1, -j w]], det = w^2 - 1, singular exactly where k w == 1.0; a diode-connected
# device on equation 0.  1.0 / 3.0 rounds so that 3.0 * (1.0 / 3.0) == 1.0.
TANK_OMEGA = np.array([0.25, 0.5, 1.0, 1.0 / 3.0, 0.0])
TANK_FAILS_AT = (0, 2, 1, 3, 0)                               # first failing order per frequency, 0 = none


def tank():
    G = np.array([[0.0, 1.0], [1.0, 0.0]])
    C = np.array([[1.0, 0.0], [0.0, -1.0]])
    J = np.array([0.5 + 0.0j, 0.25j])
    coef = np.array([[0.3, -0.2, 0.15, 0.05, -0.04, 0.03, -0.02]])
    return dict(n=2, M=1, G=G[None], C=C[None], J=J[None], dev_d=np.array([0], dtype=np.int32),
                dev_g=np.array([0], dtype=np.int32), dev_s=np.array([-1], dtype=np.int32), coef=coef[None], out=(0, 1))


_cache = {}


def reference(key):
    """disto_reference.solve_sweep of every system of a case, computed once: key (n, M) or "tank"
    -> [dict(flags, per_f, h, hd, logs) per system]"""
    import disto_reference as dref
    if key not in _cache:
        c, omega = (tank(), TANK_OMEGA) if key == "tank" else (case(*key), OMEGA)
        _cache[key] = [dref.solve_sweep(c["G"][b], c["C"][b], c["J"][b], omega, c["dev_d"], c["dev_g"], c["dev_s"],
                                        c["coef"][b], c["out"]) for b in range(len(c["G"]))]
    return _cache[key]
