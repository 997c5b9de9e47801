"""The inputs of the intermodulation kernel tests, shared by the CPU test (tests/imd_reference.py against the
host-compiled ac_imd_solve(), tests/test_imd_cpu.py) and the GPU test (kernels against the reference,
tests/test_imd_kernels_gpu.py).

The systems, device tables and coefficients are those of tests/disto_cases.py (n in {1, 2, 5, 31, 32, 33, 63}, 0, 1, 3
and 65 devices, a batch of 3).  Added here: four tone pairs -- an ordinary one, w2 = 0, w1 == w2 (A(w1 - w2) = G) and
w1 < w2 (w1 - w2 negative) -- and a second excitation J2 != J1 for the cases of J2_CASES.  The LC tank of disto_cases
is singular exactly where w == 1: six pairs, each of which puts a different one of the six solves there first.
"""
import numpy as np

import disto_cases as dc

OMEGA1 = np.array([1.0, 2.5, 0.375, 0.75])
OMEGA2 = np.array([0.5, 0.0, 0.375, 1.25])
B = dc.B
CASES = dc.CASES
J2_CASES = [(2, 1), (5, 65), (32, 3), (63, 3)]

# (w1, w2): w1; w2; w1 + w2; w1 - w2; 2 w1; 2 w1 - w2 is 1.0, and no earlier one is (all values exact in binary)
TANK_OMEGA1 = np.array([1.0, 1.5, 0.75, 1.5, 0.5, 0.75])
TANK_OMEGA2 = np.array([0.5, 1.0, 0.25, 0.5, 0.25, 0.5])
TANK_FAILS_AT = (0, 1, 2, 3, 4, 5)                            # first failing solve per pair

case = dc.case
tank = dc.tank


def second_excitation(n, M, seed=20261021):
    """J2 [B][n] complex of case (n, M), drawn apart from the case so that the case itself stays as it is"""
    rng = np.random.default_rng([seed, n, M])
    return rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))


_cache = {}


def reference(key):
    """imd_reference.solve_sweep of every system of a case, computed once: key (n, M), (n, M, "j2") or "tank"
    -> [dict(flags, per_f, h, im) per system]"""
    import imd_reference as iref
    if key not in _cache:
        if key == "tank":
            c, w1, w2, J2 = tank(), TANK_OMEGA1, TANK_OMEGA2, None
        else:
            c, w1, w2 = case(key[0], key[1]), OMEGA1, OMEGA2
            J2 = second_excitation(key[0], key[1]) if len(key) == 3 else None
        _cache[key] = [iref.solve_sweep(c["G"][b], c["C"][b], c["J"][b], None if J2 is None else J2[b], w1, w2, c["dev_d"],
                                        c["dev_g"], c["dev_s"], c["coef"][b], c["out"]) for b in range(len(c["G"]))]
    return _cache[key]
