"""numpy restatement of the periodic-steady-state analysis (include/csim.h "Periodic steady state") on top of the
oracle binding: oracle.tran gives PHI (K steps of the reference's transient from a state), oracle.stamp_tran the matrix
J_k at a converged iterate and the right-hand side whose differences in xprev are Hm.  The DFT, the closure test and the
update are written as engine/pss.hpp writes them, operation by operation, so they agree with it bit for bit; the
sensitivity goes through numpy.linalg.solve and agrees to rounding."""
import numpy as np

from oracle import binding as oracle

ST_TRAN_NONFINITE, ST_TRAN_NONCONV, ST_LU_TINY_PIVOT = 0x1, 0x2, 0x4
ST_PSS_NONCONV, ST_PSS_SINGULAR = 0x200, 0x400


def twiddles(K):
    """the table as pss.hpp's pss_twiddles makes it (the tests take the library's own and compare it with this one)"""
    j = np.arange(K, dtype=np.float64)
    ang = 2.0 * 3.14159265358979323846 * j / float(K)
    return np.cos(ang), np.sin(ang)


def dft(xs, c, s, H, probes=None):
    """xs [K][N]: the states after steps 1 .. K.  -> complex [H+1][n_probe], the sums in pss.hpp's order"""
    K = len(c)
    assert xs.shape[0] == K
    x = xs if probes is None else xs[:, list(probes)]
    out = np.zeros((H + 1, x.shape[1]), dtype=complex)
    for m in range(H + 1):
        re = np.zeros(x.shape[1])
        im = np.zeros(x.shape[1])
        for k in range(1, K + 1):
            j = (m * k) % K
            pc = x[k - 1] * c[j]
            ps = x[k - 1] * s[j]
            re = re + pc
            im = im + ps
        scale = (1.0 if m == 0 else 2.0) / float(K)
        out[m].real = scale * re                    # the parts are stored, not summed: a zero keeps its sign
        out[m].imag = np.zeros_like(im) if m == 0 else -(scale * im)
    return out


def hm_matrix(ir, N, params, b, h):
    """Hm = d(right-hand side)/d(xprev): the history currents are linear in xprev, so a difference is exact up to the
    rounding of the sum with the sources; a step of 2^20 in xprev makes that rounding relative to Hm itself"""
    z = np.zeros(N)
    _, base = oracle.stamp_tran(ir, params, b, z, z, h, h)
    Hm = np.zeros((N, N))
    big = 2.0 ** 20
    for l in range(N):
        e = np.zeros(N)
        e[l] = big
        _, I = oracle.stamp_tran(ir, params, b, z, e, h, h)
        Hm[:, l] = (I - base) / big
    return Hm


def period(ir, N, params, b, h, K, x0):
    """-> (states [K+1][N] with row 0 = x0, status) of K steps of the reference's transient from x0"""
    r = oracle.tran(ir, N, params, b, h, (K + 0.25) * h, 0.0, x0=np.asarray(x0, dtype=np.float64))
    assert r["n_steps"] == K
    rows = r["rows"]
    if rows.shape[0] != K + 1:                  # the reference threw (a state that is not finite)
        return None, r["status"] | ST_TRAN_NONFINITE
    return rows[:, 1:].copy(), r["status"]


def sensitivity(ir, N, params, b, h, xs, Hm):
    """W_K = prod J_k^-1 Hm along the trajectory xs [K+1][N]"""
    W = np.eye(N)
    for k in range(1, xs.shape[0]):
        J, _ = oracle.stamp_tran(ir, params, b, xs[k], xs[k - 1], float(k) * h, h)
        W = np.linalg.solve(J, Hm @ W)
    return W


def shoot(ir, N, params, b, h, K, x0, tol, max_rounds, H, probes=None, table=None):
    """-> dict(x0, harm complex [H+1][n_probe], rounds, status, W: the last round's W_K, closure: its ||x_K - x0||_inf,
    xs [K+1][N]: its trajectory)"""
    c, s = table if table is not None else twiddles(K)
    Hm = hm_matrix(ir, N, params, b, h)
    x0 = np.array(x0, dtype=np.float64)
    status, rounds, harm, W, nrm, traj = 0, 0, None, None, np.inf, None
    while True:
        xs, st = period(ir, N, params, b, h, K, x0)
        status |= st
        rounds += 1
        if xs is None or not np.all(np.isfinite(xs)):
            status |= ST_TRAN_NONFINITE
            break
        traj = xs
        W = sensitivity(ir, N, params, b, h, xs, Hm)
        harm = dft(xs[1:], c, s, H, probes)
        r = xs[K] - x0
        nrm = float(np.max(np.abs(r)))
        if nrm < tol:
            break
        if rounds >= max_rounds:
            status |= ST_PSS_NONCONV
            break
        A = np.where(np.eye(N, dtype=bool), 1.0, 0.0) - W
        x0 = x0 + np.linalg.solve(A, r)
    return dict(x0=x0, harm=harm, rounds=rounds, status=status, W=W, closure=nrm, xs=traj)


def linear_recursion(ir, N, params, b, h, K):
    """A linear circuit's transient step is x_k = A x_{k-1} + b_k with A = J^-1 Hm, b_k = J^-1 (sources at t_k), solved
    exactly.  -> (A, b [K][N]) in numpy.longdouble (the inverse by Newton refinement of numpy's double one)"""
    LD = np.longdouble
    z = np.zeros(N)
    J, _ = oracle.stamp_tran(ir, params, b, z, z, h, h)
    Hm = hm_matrix(ir, N, params, b, h)
    Jl = J.astype(LD)
    Ji = np.linalg.inv(J).astype(LD)
    for _ in range(3):
        Ji = Ji + Ji @ (np.eye(N, dtype=LD) - Jl @ Ji)
    A = Ji @ Hm.astype(LD)
    src = np.zeros((K, N), dtype=LD)
    for k in range(1, K + 1):
        _, I = oracle.stamp_tran(ir, params, b, z, z, float(k) * h, h)
        src[k - 1] = Ji @ I.astype(LD)
    return A, src


def _inv_ld(M):
    LD = np.longdouble
    n = M.shape[0]
    Mi = np.linalg.inv(M.astype(np.float64)).astype(LD)
    for _ in range(3):
        Mi = Mi + Mi @ (np.eye(n, dtype=LD) - M @ Mi)
    return Mi


def closed_form(A, src):
    """x0* = (I - A^K)^-1 sum_k A^(K-k) b_k and the orbit x_1 .. x_K from it, numpy.longdouble
    -> (x0*, orbit [K][N], (I - A^K)^-1)"""
    LD = np.longdouble
    K, N = src.shape
    acc = np.zeros(N, dtype=LD)
    P = np.eye(N, dtype=LD)
    for k in range(K, 0, -1):                   # P = A^(K-k)
        acc = acc + P @ src[k - 1]
        P = P @ A
    Minv = _inv_ld(np.eye(N, dtype=LD) - P)     # P = A^K
    x0 = Minv @ acc
    orbit = np.zeros((K, N), dtype=LD)
    x = x0
    for k in range(1, K + 1):
        x = A @ x + src[k - 1]
        orbit[k - 1] = x
    return x0, orbit, Minv


def step_floor(A, K, consts_alpha=0.45, consts_tol=1e-6):
    """What one period of the damped iteration may differ from the exact recursion by, in the infinity norm.  A step
    stops at ||alpha (x_raw - x)||_2 < tol; what is then left of the distance to x_raw is (1 - alpha) / alpha of the
    last update, below (1 - alpha) / alpha * tol in every component.  A period carries the error of step k through
    A^(K-k)."""
    LD = np.longdouble
    delta = LD((1.0 - consts_alpha) / consts_alpha * consts_tol)
    total = LD(0.0)
    P = np.eye(A.shape[0], dtype=LD)
    for _ in range(K):
        total = total + np.max(np.sum(np.abs(P), axis=1)) * delta
        P = P @ A
    return float(total)


def agreement_bounds(ir, N, params, b, h, r, tol, alpha=0.45, step_tol=1e-6):
    """How far two states that both close within tol may lie apart, and their harmonics, from the restatement's own last
    round r (a shoot() result).  PHI is smooth only between the points where a step's iteration count changes; there it
    jumps by up to delta = (1 - alpha) / alpha * step_tol in step k, which reaches x_K through S_K .. S_(k+1),
    S_k = J_k^-1 Hm.  So PHI(x) - x = r1, PHI(y) - y = r2 give |x - y| <= ||(I - W_K)^-1|| (2 tol + floor),
    floor = delta sum_k ||S_K .. S_(k+1)||; a state x_k of the orbit moves by at most max_k ||S_k .. S_1|| |x - y| + floor
    and a peak phasor by twice that.  -> (state bound, harmonic bound), infinity norms"""
    xs = r["xs"]
    K = xs.shape[0] - 1
    Hm = hm_matrix(ir, N, params, b, h)
    S = []
    for k in range(1, K + 1):
        J, _ = oracle.stamp_tran(ir, params, b, xs[k], xs[k - 1], float(k) * h, h)
        S.append(np.linalg.solve(J, Hm))
    delta = (1.0 - alpha) / alpha * step_tol
    floor, P = 0.0, np.eye(N)
    for k in range(K, 0, -1):
        floor += norm_inf(P) * delta
        P = P @ S[k - 1]
    grow, P = 1.0, np.eye(N)
    for k in range(1, K + 1):
        P = S[k - 1] @ P
        grow = max(grow, norm_inf(P))
    minv = norm_inf(np.linalg.inv(np.eye(N) - r["W"]))
    state = minv * (2.0 * tol + floor)
    return state, 2.0 * (grow * state + floor)


TOL, MAX_ROUNDS = 2e-6, 20         # the engine's defaults (pss_tol, pss_max_rounds)
_CACHE = {}


def setup(name):
    """-> (netlist, tstep, K, n_harm) of a case of tests/pss_cases.py or of a shipped netlist"""
    import pss_cases as pc
    if name in pc.CASES or name in pc.EXTRA:
        return pc.netlist(name), pc.tstep(name), pc.case(name)[1], pc.case(name)[2]
    c = pc.SHIPPED[name]
    return pc.shipped(name), c["tstep"], c["K"], c["n_harm"]


def reference(name, B, tol=None):
    """The restatement for every instance of a batch of B from its DC operating point, computed once per (name, B, tol)
    and shared by the tests: -> (params [P][B], [shoot() result per instance])"""
    import pss_cases as pc
    if tol is not None and tol != TOL:
        if (name, B, tol) not in _CACHE:
            nl, h, K, H = setup(name)
            p = pc.params(nl, B)
            _CACHE[(name, B, tol)] = (p, [shoot(nl.ir_ptr, nl.n_unknowns, p, b, h, K, oracle.dc(nl.ir_ptr, nl.n_unknowns, p, b)[0],
                                                tol, MAX_ROUNDS, H) for b in range(B)])
        return _CACHE[(name, B, tol)]
    if (name, B) not in _CACHE:
        nl, h, K, H = setup(name)
        p = pc.params(nl, B)
        res = []
        for b in range(B):
            x0, _, _ = oracle.dc(nl.ir_ptr, nl.n_unknowns, p, b)
            res.append(shoot(nl.ir_ptr, nl.n_unknowns, p, b, h, K, x0, TOL, MAX_ROUNDS, H))
        _CACHE[(name, B)] = (p, res)
    return _CACHE[(name, B)]


def norm_inf(M):
    return float(np.max(np.sum(np.abs(np.asarray(M, dtype=np.longdouble)), axis=1)))
