"""Two checks of the intermodulation analysis that know nothing of Volterra series, on the one-MOSFET stage of
tests/disto_timedomain.py (VDD - RD - d, MOSFET (d, g, s), s - RS - ground, the gate driven by an ideal source).

  torus()       no capacitances, vg = vg0 + a cos(theta1) + a cos(theta2): the stage is stepped statically on a
                theta1 x theta2 grid in numpy.longdouble and transformed by a 2-D DFT.  The bins (1, 0), (0, 1), (1, 1),
                (1, -1), (2, 0) and (2, -1) are the six solutions of the analysis, whatever the two frequencies are.
  collocation() a capacitor CL from d to ground and CGD from g to d, tones at 7 f0 and 5 f0: the periodic solution of
                C dx/dt + G x + i(x) = J(t) by Newton on the 64-sample Fourier collocation.  All products up to third
                order fall on distinct bins; the bins 7, 5, 12, 2, 14 and 9 are the six solutions.  A wrong conjugate or
                a wrong frequency in the solves at w1 - w2 and 2 w1 - w2 shows here and not on the torus.

Used by tests/test_imd_cpu.py (against tests/imd_reference.py) and tests/test_imd_gpu.py (against the engine)."""
import numpy as np

from disto_timedomain import AMP, LD, _ids, _newton

TORUS_BINS = ((1, 0), (0, 1), (1, 1), (1, -1), (2, 0), (2, -1))
TONES = (7, 5)                                                # multiples of f0
COLLOCATION_BINS = (7, 5, 12, 2, 14, 9)
# Relative bounds on |solution - bin| at AMP = 1 mV.  The two differ by the next term of the series, O((a / Vov)^2).
# Measured on the CPU on the four stages of tests/test_imd_cpu.py (NMOS and PMOS, saturation and triode), largest over
# the six solutions and both nodes.  torus(): 5.02e-7 in saturation (the solve at 2 w1), 6.62e-6 in triode (the solve
# at 2 w1 - w2).  collocation(): 3.88e-7 in saturation, 3.69e-6 in triode.  Two tones of 1 mV compress three times as
# much as the one tone of disto_timedomain.PHYSICS_BOUND.  Ten times the largest, to cover other bias points.
PHYSICS_BOUND = 6.7e-5
MEMORY_BOUND = 3.7e-5


def torus(isP, vth, k, lam, rd, rs, op, amp=AMP, gmin=0.0, nt=16):
    """-> (phasors complex [6][2] of (vd, vs) at TORUS_BINS, region)"""
    vd0, vg0, vs0 = (LD(v) for v in op)
    i_op, _, _, region = _ids(isP, vth, k, lam, vd0, vg0, vs0)
    gd_lin, gs_lin = 1 / LD(rd) + LD(gmin), 1 / LD(rs) + LD(gmin)

    def resid(vd, vs, i):
        return (vd - vd0) * gd_lin + (i - i_op), (vs - vs0) * gs_lin - (i - i_op), gd_lin, gs_lin
    theta = 2 * np.pi * np.arange(nt, dtype=LD) / nt
    samples = np.zeros((nt, nt, 2), dtype=LD)
    for a in range(nt):
        for b in range(nt):
            vg = vg0 + LD(amp) * np.cos(theta[a]) + LD(amp) * np.cos(theta[b])
            vd, vs, reg = _newton(isP, vth, k, lam, rd, rs, vg, vd0, vs0, resid)
            assert reg == region, "the stage changed region on the torus"
            samples[a, b] = vd - vd0, vs - vs0
    ph = np.zeros((len(TORUS_BINS), 2), dtype=complex)
    for q, (p1, p2) in enumerate(TORUS_BINS):
        arg = p1 * theta[:, None] + p2 * theta[None, :]
        re = 2 * (samples * np.cos(arg)[:, :, None]).sum(axis=(0, 1)) / (nt * nt)
        im = -2 * (samples * np.sin(arg)[:, :, None]).sum(axis=(0, 1)) / (nt * nt)
        ph[q] = re.astype(np.float64) + 1j * im.astype(np.float64)
    return ph, region


def collocation(isP, vth, k, lam, rd, rs, cl, cgd, w0, op, amp=AMP, gmin=0.0, nt=64):
    """One period 2 pi / w0 of vg = vg0 + amp cos(7 w0 t) + amp cos(5 w0 t).  Unknowns: the deviations of vd and vs from
    the operating point at nt equidistant times; d/dt is the spectral derivative of the trigonometric interpolant.
    Residuals in numpy.longdouble, Newton steps by a float64 solve.
    -> (phasors complex [6][2] of (vd, vs) at COLLOCATION_BINS, region)"""
    vd0, vg0, vs0 = (LD(v) for v in op)
    i_op, _, _, region = _ids(isP, vth, k, lam, vd0, vg0, vs0)
    gd_lin, gs_lin = 1 / LD(rd) + LD(gmin), 1 / LD(rs) + LD(gmin)
    cl, cgd, w0, amp = LD(cl), LD(cgd), LD(w0), LD(amp)
    theta = 2 * np.pi * np.arange(nt, dtype=LD) / nt
    delta = theta[:, None] - theta[None, :]
    D = np.zeros((nt, nt), dtype=LD)
    for h in range(1, nt // 2):
        D -= h * np.sin(h * delta)
    D *= w0 * 2 / nt
    dvg = sum(amp * np.cos(m * theta) for m in TONES)
    dvg_dt = sum(-amp * m * w0 * np.sin(m * theta) for m in TONES)
    vd, vs = np.zeros(nt, dtype=LD), np.zeros(nt, dtype=LD)
    for _ in range(50):
        i, did, dis = np.zeros(nt, dtype=LD), np.zeros(nt, dtype=LD), np.zeros(nt, dtype=LD)
        for t in range(nt):
            i[t], did[t], dis[t], reg = _ids(isP, vth, k, lam, vd0 + vd[t], vg0 + dvg[t], vs0 + vs[t])
            assert reg == region, "the stage changed region within the period"
        f1 = (cl + cgd) * (D @ vd) - cgd * dvg_dt + vd * gd_lin + (i - i_op)
        f2 = vs * gs_lin - (i - i_op)
        jac = np.zeros((2 * nt, 2 * nt))
        jac[:nt, :nt] = ((cl + cgd) * D).astype(np.float64) + np.diag((gd_lin + did).astype(np.float64))
        jac[:nt, nt:] = np.diag(dis.astype(np.float64))
        jac[nt:, :nt] = np.diag((-did).astype(np.float64))
        jac[nt:, nt:] = np.diag((gs_lin - dis).astype(np.float64))
        step = np.linalg.solve(jac, np.concatenate([f1, f2]).astype(np.float64))
        vd, vs = vd - step[:nt], vs - step[nt:]
        if np.max(np.abs(step)) < 1e-18:                   # the rounding of vd0 + vd in longdouble
            break
    else:
        raise AssertionError("the collocation did not converge")
    samples = np.stack([vd, vs], axis=1)
    ph = np.zeros((len(COLLOCATION_BINS), 2), dtype=complex)
    for q, h in enumerate(COLLOCATION_BINS):
        re = 2 * (samples * np.cos(h * theta)[:, None]).sum(axis=0) / nt
        im = -2 * (samples * np.sin(h * theta)[:, None]).sum(axis=0) / nt
        ph[q] = re.astype(np.float64) + 1j * im.astype(np.float64)
    return ph, region
