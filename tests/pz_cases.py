"""Inputs of the pole-kernel tests (tests/test_pz_kernels_gpu.py on the GPU, tests/test_pz_cpu.py for what must hold of
them without one): seeded systems G = diagonally dominant random, C = random of rank ceil(n / 2), and an fmax per batch
at which numpy's eigenvalues keep clear of the cut (pz_host.gap_ok); then the singular, C = 0 and right-half-plane
systems."""
import numpy as np

import pz_host as ph

SIZES = (1, 2, 3, 31, 32, 33, 63)       # one eigenvalue, a 2 x 2 block, the first real bulge, the odd-LD change points
#                                         (LD = n | 1: 31, 33, 33, 63), the LDS maximum
BATCHES = (1, 2, 65)                    # one wave, two, more than one wave per SIMD of a compute unit
NB = max(BATCHES)


def systems(n, nb=NB, seed=20261021):
    rng = np.random.default_rng(seed + n)
    r = (n + 1) // 2
    G = rng.uniform(-1.0, 1.0, (nb, n, n))
    for b in range(nb):
        G[b][np.diag_indices(n)] = (np.abs(G[b]).sum(axis=1) + 1.0) * rng.choice([-1.0, 1.0], n)
    C = np.einsum("bik,bjk->bij", rng.uniform(-1.0, 1.0, (nb, n, r)), rng.uniform(-1.0, 1.0, (nb, n, r))) * 1e-9
    return G, C


def pick_fmax(mus):
    """an fmax for a batch from numpy's eigenvalues of every instance: the cut 8 times below the slowest eigenvalue of
    the upper cluster, which is everything within 1e-8 of the batch's largest magnitude (the rank deficiency of C
    leaves the others at rounding level; case() asserts the gap)"""
    a = np.abs(np.concatenate(mus))
    lo = a[a > 1e-8 * a.max()].min()
    return 1.0 / (2.0 * np.pi * (lo / 8.0))


_cache = {}


def case(n):
    """-> dict(G, C [NB][n][n], fmax, mu: numpy's eigenvalues per instance, M); the gap condition asserted"""
    if n not in _cache:
        G, C = systems(n)
        pairs = [ph.numpy_mu(G[b], C[b]) for b in range(NB)]
        mus = [p[1] for p in pairs]
        fmax = pick_fmax(mus)
        for mu in mus:
            assert ph.gap_ok(mu, fmax), (n, "an eigenvalue of the fixture lies too close to the cut")
        _cache[n] = dict(G=G, C=C, fmax=fmax, mu=mus, M=[p[0] for p in pairs])
    return _cache[n]


_ref = {}


def reference(n):
    """the host-compiled statement on all NB instances of case(n), computed once"""
    if n not in _ref:
        c = case(n)
        _ref[n] = ph.poles_batch(c["G"], c["C"], c["fmax"])
    return _ref[n]


def special():
    """n = 3, four instances at fmax = 1e6: singular A0 (a zero row of G where C has none either), C = 0, a negative
    conductance (one pole in the right half plane), and an ordinary RC for company"""
    G = np.zeros((4, 3, 3))
    C = np.zeros((4, 3, 3))
    G[0] = [[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 0.0]]
    C[0] = np.diag([1e-3, 2e-3, 0.0])
    G[1] = np.diag([1.0, 2.0, 3.0])
    G[2] = [[-1.0, 0.0, 0.0], [0.0, 2.0, -1.0], [0.0, -1.0, 1.0]]
    C[2] = np.diag([1e-3, 1e-3, 0.0])
    G[3] = [[2.0, -1.0, 0.0], [-1.0, 2.0, -1.0], [0.0, -1.0, 1.0]]
    C[3] = np.diag([1e-3, 2e-3, 3e-3])
    return dict(G=G, C=C, fmax=1e6, want_flags=[ph.PZ_SINGULAR, 0, 0, 0], want_n=[0, 0, 2, 3], want_rhp=[0, 0, 1, 0])
