"""The seeded inputs of the AC sweep kernel tests, shared by the CPU test (reference against the host-compiled
ac_lu_solve(), tests/test_ac_cpu.py) and the GPU test (kernels against the reference, tests/test_ac_kernels_gpu.py).

A case is a batch of five systems (G, C, J) of one size n and one kind; the GPU test runs its first B systems
for B in BATCHES.  Every sweep uses OMEGA: the matrix is G + jC at w = 1, G alone at w = 0, G + 2.5jC after it.

Structured kinds place their feature at column k of the elimination with a block form: rows k.. are zero in the
columns before k, so their multipliers there are exactly zero, the rows are skipped and reach column k untouched;
the leading block is diagonally dominant in G, so it never takes a pivot from below.
"""
import numpy as np

OMEGA = np.array([1.0, 0.0, 2.5])
BATCHES = (1, 2, 3, 5)
NSYS = 5
SIZES = tuple(range(1, 64))
SIZE_CLASSES = ((1, 8), (9, 16), (17, 24), (25, 32), (33, 63))
TIE = (5.0, 3.0 + 4.0j, -5.0j, -4.0 + 3.0j)              # re^2 + im^2 == 25 exactly

KINDS = ("dense", "mna", "reversed", "shift_up", "shift_down", "tie_diag", "tie_rows", "sing_first", "sing_mid",
         "sing_last", "sing_dc_only", "thr_below", "thr_above", "thr_both", "nan_diag", "nan_below")
SINGULAR = ("sing_first", "sing_mid", "sing_last", "thr_below")     # flagged at every frequency
HAS_NAN = ("nan_diag", "nan_below")


def _cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _dominant(rng, n):
    """dense complex, the diagonal dominant in the real part (so at w = 0 as well)"""
    A = _cplx(rng, n, n)
    A[np.arange(n), np.arange(n)] = (2.0 * n + 2.0) * rng.choice([-1.0, 1.0], n) + 1j * rng.standard_normal(n)
    return A


def _blocked(rng, n, k):
    """dominant leading k x k block, zero below it, dense elsewhere"""
    A = _cplx(rng, n, n)
    A[:k, :k] = _dominant(rng, k)
    A[k:, :k] = 0.0
    return A


def _column(rng, n):
    return int(rng.choice([0, n // 2, n - 1, int(rng.integers(0, n))]))


def _mna(rng, n):
    """node block: conductance / capacitance Laplacians with a gmin on the diagonal; branch rows: +-1 incidence
    pairs with a zero diagonal (voltage source) or -L on the C diagonal (inductor); 60-90 % exact zeros where the
    size allows it"""
    nb = n // 4
    nn = n - nb
    G = np.zeros((n, n))
    C = np.zeros((n, n))

    def stamp(M, a, b, v):
        M[a, a] += v
        M[b, b] += v
        M[a, b] -= v
        M[b, a] -= v
    for M, lo, hi in ((G, 1e-4, 1e-1), (C, 1e-4, 1.0)):    # w is of order 1 here: w C of the size of G
        for a in range(nn - 1):
            stamp(M, a, a + 1, rng.uniform(lo, hi))
        want = (1.0 - rng.uniform(0.6, 0.9)) * n * n
        tries = 0
        while np.count_nonzero(M) + 4 * nb + 4 <= want and tries < 4 * n * n and nn > 2:
            a, b = rng.integers(0, nn, 2)
            if a != b:
                stamp(M, int(a), int(b), rng.uniform(lo, hi))
            tries += 1
    G[np.arange(nn), np.arange(nn)] += 1e-6
    J = np.zeros(n, dtype=complex)
    for s in range(nb):
        r = nn + s
        G[r, s] = G[s, r] = 1.0
        if nn > nb and rng.random() < 0.5:
            m = nb + s % (nn - nb)
            G[r, m] = G[m, r] = -1.0
        if rng.random() < 0.3:
            C[r, r] = -rng.uniform(0.1, 2.0)
        else:
            J[r] = _cplx(rng)[()]
    if nb == 0 or rng.random() < 0.5:
        J[int(rng.integers(0, nn))] += _cplx(rng)[()]
    return G + 1j * C, J


def _system(rng, kind, n):
    """-> (A complex [n][n] = G + jC, J complex [n]) or None when the size has no room for the feature"""
    J = _cplx(rng, n)
    if kind == "dense":
        return _cplx(rng, n, n), J
    if kind == "mna":
        return _mna(rng, n)
    if kind in ("reversed", "shift_up", "shift_down"):
        A = _dominant(rng, n)
        order = {"reversed": np.arange(n)[::-1], "shift_up": np.roll(np.arange(n), -1),
                 "shift_down": np.roll(np.arange(n), 1)}[kind]
        return A[order], J[order]
    if kind in ("tie_diag", "tie_rows"):
        need = 2 if kind == "tie_diag" else 3
        if n < need:
            return None
        k = min(_column(rng, n), n - need)
        A = _blocked(rng, n, k)
        col = 0.5 * _cplx(rng, n - k)                       # |.|^2 of these stays far below 25
        col = col / np.maximum(1.0, np.abs(col))
        later = np.sort(rng.choice(np.arange(1, n - k), need - 1, replace=False))
        if kind == "tie_diag":                              # the diagonal ties with a later row (and the last row)
            col[0] = TIE[0]
            col[later[0]] = TIE[1]
            col[n - k - 1] = TIE[3]
        else:                                               # two later rows tie, the diagonal is smaller
            col[later[0]] = TIE[2]
            col[later[1]] = TIE[3]
        A[k:, k] = col
        return A, J
    if kind in ("sing_first", "sing_mid", "sing_last"):
        k = {"sing_first": 0, "sing_mid": n // 2, "sing_last": n - 1}[kind]
        A = _blocked(rng, n, k)
        A[k:, k] = 0.0
        return A, J
    if kind == "sing_dc_only":                              # one row lives in C alone
        A = _dominant(rng, n)
        r = int(rng.integers(0, n))
        A[r] = 1j * (np.abs(A[r].imag) + 0.5) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        return A, J
    if kind in ("thr_below", "thr_above", "thr_both"):
        k = _column(rng, n)
        A = _blocked(rng, n, k)
        top = {"thr_below": 0.99e-15, "thr_above": 1.01e-15, "thr_both": 0.8e-15 + 0.8e-15j}[kind]
        col = np.zeros(n - k, dtype=complex)
        col[0] = 0.5 * top
        col[int(rng.integers(0, n - k))] = top
        A[k:, k] = col
        return A, J
    if kind == "nan_diag":
        k = _column(rng, n)
        A = _blocked(rng, n, k)
        A[k, k] = complex(np.nan, A[k, k].imag)
        return A, J
    if kind == "nan_below":
        if n < 2:
            return None
        k = min(_column(rng, n), n - 2)
        A = _blocked(rng, n, k)
        r = int(rng.integers(k + 1, n))
        A[r, k] = complex(np.nan, 0.0) if rng.random() < 0.5 else complex(A[r, k].real, np.nan)
        return A, J
    raise ValueError(kind)


def case(kind, n, seed=20240607):
    """-> dict(kind, n, G [5][n][n], C [5][n][n], J [5][n] complex) or None"""
    rng = np.random.default_rng([seed, KINDS.index(kind), n])
    sys = [_system(rng, kind, n) for _ in range(NSYS)]
    if any(s is None for s in sys):
        return None
    A = np.stack([s[0] for s in sys])
    return dict(kind=kind, n=n, G=np.ascontiguousarray(A.real), C=np.ascontiguousarray(A.imag),
                J=np.stack([s[1] for s in sys]))


def all_cases(sizes=SIZES, kinds=KINDS):
    for n in sizes:
        for kind in kinds:
            c = case(kind, n)
            if c is not None:
                yield c


def reference(c):
    """the reference's answer to a case: -> (flags [5] uint32, x [5][F][n] complex, per-frequency flags [5][F],
    pivot logs [5][F])"""
    import ac_reference
    res = [ac_reference.solve_sweep(c["G"][s], c["C"][s], c["J"][s], OMEGA) for s in range(NSYS)]
    return (np.array([r[0] for r in res], dtype=np.uint32), np.stack([r[1] for r in res]),
            [r[2] for r in res], [r[3] for r in res])


class Coverage:
    """per size class, the number of systems whose factorisation (at any frequency of the sweep) exchanged rows in
    at least n/2 columns, took the first of tied rows, skipped a row for an exactly zero multiplier"""

    def __init__(self):
        self.swaps = [0] * len(SIZE_CLASSES)
        self.ties = [0] * len(SIZE_CLASSES)
        self.skips = [0] * len(SIZE_CLASSES)

    def add(self, n, logs):
        """logs: the pivot logs of ONE system, one per frequency"""
        c = size_class(n)
        self.swaps[c] += any(2 * g.swaps >= n for g in logs)
        self.ties[c] += any(g.ties > 0 for g in logs)
        self.skips[c] += any(g.skips > 0 for g in logs)

    def __str__(self):
        names = ["n<=%d" % hi for _, hi in SIZE_CLASSES]
        return "; ".join("%s: swaps %d ties %d skips %d" % (names[i], self.swaps[i], self.ties[i], self.skips[i])
                         for i in range(len(names)))

    def check(self):
        assert all(v > 0 for v in self.swaps + self.ties + self.skips), str(self)


def size_class(n):
    for i, (lo, hi) in enumerate(SIZE_CLASSES):
        if lo <= n <= hi:
            return i
    raise ValueError(n)
