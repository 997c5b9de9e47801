"""numpy restatement of the periodic noise analysis (include/csim.h "Periodic noise analysis") on top of
tests/pac_reference.py and tests/pss_reference.py: the orbit is pss_reference.period's, J_k pac_reference.jacobians',
Hm and W_K pss_reference's.  The product Hm^T q, the step's right-hand side z g + d, the closure entries, the generators'
sigma and the transfer sums with their outputs are written as engine/pnoise.hpp writes them, operation by operation, so
they agree with it bit for bit; the closure goes through ac_reference.solve, the step solves through numpy.linalg.solve
on J_k^T and agree to rounding.  dense_transfers() is an independent statement: the K N block-cyclic FORWARD system,
solved with one modulated right-hand side per (generator, sideband)."""
import ctypes as C

import numpy as np

import ac_reference
import noise_reference as nref
import pac_reference as par
import pss_reference as pr
from oracle import binding as oracle

ST_PAC_SINGULAR = par.ST_PAC_SINGULAR
KIND_R, KIND_V, KIND_I, KIND_NMOS, KIND_PMOS = 0, 3, 4, 5, 6


def selector(N, out_p, out_m):
    d = np.zeros(N)
    d[out_p] = 1.0
    if out_m >= 0:
        d[out_m] = -1.0
    return d


def records(nl):
    """-> [(kind, [4 equations], branch equation, parameter slot)] per element"""
    ir = C.cast(nl.ir_ptr, C.POINTER(par._IR)).contents
    return [(ir.kind[e], [ir.eq[4 * e + i] for i in range(4)], ir.branch_eq[e], ir.param_slot[e]) for e in range(ir.n_elems)]


def gain_terminals(nl, src_elem):
    """the unit excitation of the input source as a generator's (a, b): a V source's branch equation against ground, an
    I source (p, m) as q[m] - q[p]"""
    kind, q, br, _ = records(nl)[src_elem]
    if kind == KIND_V:
        return br, -1
    assert kind == KIND_I
    return q[1], q[0]


def mos_gg(isP, Vth, K, lam, Vd, Vg, Vs):
    """gate transconductance of the level-1 model, one numpy operation per IEEE operation: gg = gm0 (1 + lambda Vds)"""
    p = np.float64(-1.0 if isP else 1.0)
    Vgs = p * (Vg - Vs)
    Vds = p * (Vd - Vs)
    gm0 = np.float64(0.0)
    if Vgs > Vth and Vds >= 0.0:
        Vov = Vgs - Vth
        gm0 = K * Vds if Vds < Vov else K * Vov
    factor = np.float64(1.0) + lam * Vds
    if factor < 0.0:
        factor = np.float64(0.0)
    return gm0 * factor


def sigmas(nl, params, b, xs, kT4):
    """sigma_{s,k} = sqrt(psd_{s,k}) at the states xs [K+1][N] -> [K][S], row k - 1 for step k"""
    recs = records(nl)
    gens = nl.noise_sources
    K = xs.shape[0] - 1
    out = np.zeros((K, len(gens)))
    kT4 = np.float64(kT4)
    for s, (e, _, _) in enumerate(gens):
        kind, q, _, slot = recs[e]
        for k in range(1, K + 1):
            if kind == KIND_R:
                R = np.float64(params[slot, b])
                psd = np.float64(0.0) if R == 0.0 else kT4 * (np.float64(1.0) / R)
            else:
                assert kind in (KIND_NMOS, KIND_PMOS)
                v = [np.float64(xs[k, t]) if t >= 0 else np.float64(0.0) for t in q[:3]]
                gg = mos_gg(kind == KIND_PMOS, np.float64(params[slot, b]), np.float64(params[slot + 1, b]),
                            np.float64(params[slot + 2, b]), v[0], v[1], v[2])
                psd = kT4 * (np.float64(2.0 / 3.0) * np.abs(gg))
            out[k - 1, s] = np.sqrt(psd)
    return out


def hmT_product(Hm, qr, qi):
    """g = Hm^T q: row i over the non-zero Hm(l, i), l ascending; qr, qi [N][F]"""
    return par.hm_product(np.ascontiguousarray(Hm.T), qr, qi)


def step_rhs(zr, zi, gr, gi, d):
    """z g + d with a real d: im = (zr gi + zi gr) + 0.0"""
    return par.step_rhs(zr, zi, gr, gi, d, np.zeros_like(d))


def close_matrix(W, zK):
    """I - z_K W^T entry by entry -> (Ar, Ai)"""
    return par.close_matrix(np.ascontiguousarray(W.T), zK)


def recursion(Js, Hm, d, z, gK):
    """J_k^T q_k = z g_k + d, g_{k-1} = Hm^T q_k, k = K .. 1, from gK complex [N][F]
    -> (qs complex [K][N][F] with q_k at index k - 1, g_0 complex [N][F])"""
    zr, zi = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    g_r, g_i = np.ascontiguousarray(gK.real), np.ascontiguousarray(gK.imag)
    F = len(z)
    qs = np.zeros((len(Js),) + gK.shape, dtype=complex)
    for k in range(len(Js), 0, -1):
        re, im = step_rhs(zr, zi, g_r, g_i, d)
        sol = np.linalg.solve(Js[k - 1].T, np.concatenate([re, im], axis=1))
        q_r, q_i = np.ascontiguousarray(sol[:, :F]), np.ascontiguousarray(sol[:, F:])
        qs[k - 1].real = q_r
        qs[k - 1].imag = q_i
        g_r, g_i = hmT_product(Hm, q_r, q_i)
    return qs, g_r + 1j * g_i


def _at(plane, eq):
    return plane[eq] if eq >= 0 else np.zeros_like(plane[0])


def transfer_sums(qs, sig, terms, c, s, M):
    """qs complex [K][N][F], sig [K][G], terms [(a, b)] * G -> T complex [F][2 M + 1][G], the sums in pnoise.hpp's order:
    k = K .. 1, w = sigma (q[a] - q[b]), re += wr c - wi s, im += wi c + wr s, the scale 1/K on the finished sums"""
    K, _, F = qs.shape
    G = len(terms)
    out = np.zeros((F, 2 * M + 1, G), dtype=complex)
    scale = 1.0 / float(K)
    Qr, Qi = np.ascontiguousarray(qs.real), np.ascontiguousarray(qs.imag)
    for g, (a, b) in enumerate(terms):
        dr = [_at(Qr[k], a) - _at(Qr[k], b) for k in range(K)]
        di = [_at(Qi[k], a) - _at(Qi[k], b) for k in range(K)]
        for m in range(-M, M + 1):
            re = np.zeros(F)
            im = np.zeros(F)
            for k in range(K, 0, -1):
                j = ((m * k) % K + K) % K
                wr = sig[k - 1, g] * dr[k - 1]
                wi = sig[k - 1, g] * di[k - 1]
                t = wr * c[j] - wi * s[j]
                re = re + t
                v = wi * c[j] + wr * s[j]
                im = im + v
            out[:, m + M, g].real = scale * re
            out[:, m + M, g].imag = scale * im
    return out


def abs2(T):
    return T.real * T.real + T.imag * T.imag


def outputs(T):
    """T complex [F][2 M + 1][S] -> (contrib [F][S], side [F][2 M + 1], onoise [F]) in pnoise.hpp's order"""
    F, nsb, S = T.shape
    p = abs2(T)
    contrib = np.zeros((F, S))
    for m in range(nsb):
        contrib = contrib + p[:, m, :]
    side = np.zeros((F, nsb))
    for s in range(S):
        side = side + p[:, :, s]
    onoise = np.zeros(F)
    for s in range(S):
        onoise = onoise + contrib[:, s]
    return contrib, side, onoise


def pnoise(nl, params, b, h, K, f0, freqs, M, out, src_elem, kT4, orbit, table=None):
    """The analysis of instance b around the orbit (xs [K+1][N], W_K).
    -> dict(T complex [F][2 M + 1][S], gain complex [F][2 M + 1], contrib [F][S], side [F][2 M + 1], onoise [F],
            status [F], qs [K][N][F], gK, sig [K][S], terms, d, xs, Js, Hm, W, z, zK)"""
    ir, N = nl.ir_ptr, nl.n_unknowns
    c, s = table if table is not None else pr.twiddles(K)
    xs, W = orbit
    Hm = pr.hm_matrix(ir, N, params, b, h)
    Js = par.jacobians(ir, params, b, h, xs)
    zs = [par.z_consts(float(f), h, f0) for f in freqs]
    z = np.array([v[0] for v in zs])
    zK = np.array([v[1] for v in zs])
    F = len(freqs)
    d = selector(N, out[0], out[1])
    _, r = recursion(Js, Hm, d, z, np.zeros((N, F), dtype=complex))
    gK = np.zeros((N, F), dtype=complex)
    status = np.zeros(F, dtype=np.uint32)
    for f in range(F):
        Ar, Ai = close_matrix(W, zK[f])
        fl, xr, xi, _ = ac_reference.solve(Ar, Ai, r[:, f].real.copy(), r[:, f].imag.copy())
        if fl:
            status[f] |= ST_PAC_SINGULAR
        gK[:, f].real = xr
        gK[:, f].imag = xi
    qs, _ = recursion(Js, Hm, d, z, gK)
    gens = nl.noise_sources
    terms = [(a, b_) for _, a, b_ in gens]
    sig = sigmas(nl, params, b, xs, kT4)
    T = transfer_sums(qs, sig, terms, c, s, M)
    T[status != 0] = 0.0
    contrib, side, onoise = outputs(T)
    gain = None
    if src_elem >= 0:
        gain = transfer_sums(qs, np.ones((K, 1)), [gain_terminals(nl, src_elem)], c, s, M)[:, :, 0]
        gain[status != 0] = 0.0
    return dict(T=T, gain=gain, contrib=contrib, side=side, onoise=onoise, status=status, qs=qs, gK=gK, sig=sig,
                terms=terms, d=d, xs=xs, Js=Js, Hm=Hm, W=W, z=z, zK=zK)


def dense_system(Js, Hm, z):
    """the block-cyclic forward operator of one frequency, complex [K N][K N]: (A p)_k = J_k p_k - z Hm p_{k-1}, p_0 = p_K"""
    K, N = len(Js), Hm.shape[0]
    A = np.zeros((K * N, K * N), dtype=complex)
    for k in range(K):
        A[k * N:(k + 1) * N, k * N:(k + 1) * N] = Js[k]
        kp = (k - 1) % K
        A[k * N:(k + 1) * N, kp * N:(kp + 1) * N] += -z * Hm
    return A


def dense_transfers(Js, Hm, z, d, sig, terms, M):
    """T_{s,m} of one frequency from the FORWARD system: the source sigma_{s,k} (e_a - e_b) e^{+j 2 pi m k / K} at step k
    (a unit white source at f + m f0 modulated by the orbit), the response p solved densely, its component at f read as
    the mean of d^T p_k.  -> (T complex [2 M + 1][G], cond_2 of the system)"""
    K, N = len(Js), Hm.shape[0]
    A = dense_system(Js, Hm, z)
    G = len(terms)
    rhs = np.zeros((K * N, (2 * M + 1) * G), dtype=complex)
    for g, (a, b) in enumerate(terms):
        for m in range(-M, M + 1):
            for k in range(1, K + 1):
                ph = np.exp(2j * np.pi * ((m * k) % K) / K) * sig[k - 1, g]
                if a >= 0:
                    rhs[(k - 1) * N + a, (m + M) * G + g] += ph
                if b >= 0:
                    rhs[(k - 1) * N + b, (m + M) * G + g] -= ph
    p = np.linalg.solve(A, rhs).reshape(K, N, 2 * M + 1, G)
    T = np.einsum("n,knmg->mg", d, p) / K
    return T, float(np.linalg.cond(A))


def closed_form_linear(J, Hm, z, d, a, b):
    """d^T (J - z Hm)^-1 (e_a - e_b) of a linear circuit, numpy.clongdouble by Newton refinement of numpy's inverse"""
    CL = np.clongdouble
    A = J.astype(CL) - CL(z) * Hm.astype(CL)
    Ai = np.linalg.inv(A.astype(complex)).astype(CL)
    for _ in range(3):
        Ai = Ai + Ai @ (np.eye(A.shape[0], dtype=CL) - A @ Ai)
    e = np.zeros(A.shape[0], dtype=CL)
    if a >= 0:
        e[a] += 1
    if b >= 0:
        e[b] -= 1
    return d.astype(CL) @ (Ai @ e)


def transfer_bound(r, f, sigma_max=None):
    """How far two evaluations of the adjoint recursion in float64 may lie apart in a transfer T at frequency index f of a
    pnoise() result, derived as pac_reference.agreement_bound for the transposed recursion.  The rounding of one step's
    solve, 2^-52 cond(J_k) |q|, reaches q_1 through U_1 .. U_(k-1), U_k = J_k^-T Hm^T, and the periodic start through
    (I - z_K W_K^T)^-1.  A transfer is the mean over the steps of sigma (q[a] - q[b]) times a number of modulus one: two
    entries of q, hence the factor 2, times the largest sigma:
        2 sigma_max 2^-52 ||(I - z_K W_K^T)^-1||_inf  sum_k ||U_1 .. U_(k-1)||_inf  max_k cond_inf(J_k^T)  max |q|"""
    N = r["Hm"].shape[0]
    U = [np.linalg.solve(J.T, r["Hm"].T) for J in r["Js"]]
    total, Pm = 0.0, np.eye(N)
    for k in range(1, len(U) + 1):
        total += pr.norm_inf(Pm)
        Pm = Pm @ U[k - 1]
    cond = max(pr.norm_inf(J.T) * pr.norm_inf(np.linalg.inv(J.T)) for J in r["Js"])
    Ar, Ai = close_matrix(r["W"], r["zK"][f])
    minv = float(np.max(np.sum(np.abs(np.linalg.inv(Ar + 1j * Ai)), axis=1)))
    sm = float(np.max(r["sig"])) if sigma_max is None else sigma_max
    return 2.0 * sm * 2.0 ** -52 * minv * total * cond * float(np.max(np.abs(r["qs"][:, :, f])))


def squared_bound(Q, delta, terms):
    """a sum Q of `terms` squared moduli whose transfers are each within delta: 2 sqrt(Q) delta sqrt(terms) + terms delta^2"""
    return 2.0 * np.sqrt(Q) * delta * np.sqrt(terms) + terms * delta * delta


_CACHE = {}


def setup(name):
    """-> (netlist, tstep, K, (out_p, out_m), src_elem) of a case of tests/pnoise_cases.py"""
    import pnoise_cases as pn
    op, om, src = pn.output_and_source(name)
    return pn.netlist(name), pn.tstep(name), pn.CASES[name][1], (op, om), src


def orbits(name, B):
    """-> (params [P][B], [pss_reference.shoot result]) -- pac_reference.reference's for its cases (shared cache)"""
    import pac_cases as ac
    import pnoise_cases as pn
    if name in ac.CASES:
        p, orb, _ = par.reference(name, B)
        return p, orb
    if ("orbit", name, B) not in _CACHE:
        nl, h, K = pn.netlist(name), pn.tstep(name), pn.CASES[name][1]
        N = nl.n_unknowns
        p = pn.params(nl, B)
        orb = []
        for b in range(B):
            xdc, _, _ = oracle.dc(nl.ir_ptr, N, p, b)
            orb.append(pr.shoot(nl.ir_ptr, N, p, b, h, K, xdc, pr.TOL, pr.MAX_ROUNDS, 0))
        _CACHE[("orbit", name, B)] = (p, orb)
    return _CACHE[("orbit", name, B)]


def reference(name, B, M=None):
    """The steady state and the analysis around it for every instance of a batch of B at pnoise_cases.freqs(name),
    computed once per (name, B) and shared by the tests -> (params [P][B], [shoot() result], [pnoise() result])"""
    import pnoise_cases as pn
    M = pn.N_SIDE if M is None else M
    if (name, B, M) not in _CACHE:
        nl, h, K, out, src = setup(name)
        p, orb = orbits(name, B)
        kT4 = nref.kt4(pn.TEMP)
        res = [pnoise(nl, p, b, h, K, pn.F0, pn.freqs(name), M, out, src, kT4, (o["xs"], o["W"])) for b, o in enumerate(orb)]
        _CACHE[(name, B, M)] = (p, orb, res)
    return _CACHE[(name, B, M)]
