"""A time-domain check of the distortion analysis that knows nothing of Volterra series: the one-MOSFET stage
VDD - RD - d, MOSFET (d, g, s), s - RS - ground, without capacitances, driven at the gate by vg0 + a cos(theta), stepped
statically through one period in numpy.longdouble and transformed.  Used by tests/test_disto_cpu.py (against
tests/disto_reference.py) and tests/test_disto_gpu.py (against the engine)."""
import numpy as np

LD = np.longdouble
AMP = 1e-3
# Relative bound on |phasor - harmonic| at AMP.  The two differ by the next term of the series, O((a / Vov)^2).  Measured
# on the CPU on the four stages of tests/test_disto_cpu.py (NMOS and PMOS, saturation and triode), largest over the
# three orders and both nodes: 1.41e-7 in saturation, 1.99e-6 in triode (third order).  Ten times the largest, to cover
# other bias points.
PHYSICS_BOUND = 2.0e-5


def _ids(isP, vth, k, lam, Vd, Vg, Vs):
    """level-1 drain current (drain -> source) and its derivatives in Vd and Vs at fixed Vg; the conducting regions only"""
    p = LD(-1.0 if isP else 1.0)
    Vgs, Vds = p * (Vg - Vs), p * (Vd - Vs)
    Vov = Vgs - LD(vth)
    assert Vgs > vth and Vds >= 0, "the stage left the conducting regions"
    fac = 1 + LD(lam) * Vds
    if Vds < Vov:
        i0, gds0, gm0, region = LD(k) * (Vov * Vds - Vds * Vds / 2), LD(k) * (Vov - Vds), LD(k) * Vds, "triode"
    else:
        i0, gds0, gm0, region = LD(k) * Vov * Vov / 2, LD(0), LD(k) * Vov, "sat"
    gd = gds0 * fac + i0 * LD(lam)
    gg = gm0 * fac
    return p * i0 * fac, gd, -(gd + gg), region


def _newton(isP, vth, k, lam, rd, rs, vg, vd, vs, resid):
    """solve resid(vd, vs, i) = (f1, f2) = 0 with df1/dvd = gd_lin + dI/dvd, ...: damped Newton from (vd, vs)"""
    for _ in range(200):
        i, did, dis, region = _ids(isP, vth, k, lam, vd, vg, vs)
        f1, f2, g1, g2 = resid(vd, vs, i)
        a, b, c, d = g1 + did, dis, -did, g2 - dis
        det = a * d - b * c
        dvd, dvs = (f1 * d - b * f2) / det, (a * f2 - f1 * c) / det
        damp = min(LD(1.0), LD(0.2) / max(abs(dvd), abs(dvs), LD(1e-30)))      # no step leaves the conducting regions
        vd, vs = vd - damp * dvd, vs - damp * dvs
        if abs(dvd) + abs(dvs) < 1e-18:
            return vd, vs, region
    raise AssertionError("the static solve did not converge")


def dc_point(isP, vth, k, lam, vdd, rd, rs, vg):
    """operating point of the stage -> (vd, vs, region), numpy.longdouble"""
    def resid(vd, vs, i):
        return (vd - LD(vdd)) / LD(rd) + i, vs / LD(rs) - i, 1 / LD(rd), 1 / LD(rs)
    return _newton(isP, vth, k, lam, rd, rs, LD(vg), LD(vdd) / 2, LD(0.0), resid)


def harmonics(isP, vth, k, lam, rd, rs, op, amp=AMP, gmin=0.0, nt=64):
    """One period of vg = vg0 + amp cos(theta) around the operating point op = (vd0, vg0, vs0), stepped statically: the
    deviation (dvd, dvs) solves the circuit equations minus their value at op, with the conductance gmin from d and
    from s to ground that the small-signal matrix carries.  -> (phasors complex [3][2] of (vd, vs) at the first three
    harmonics: the bins 1 .. 3 of the DFT of the samples, evaluated in numpy.longdouble; region)"""
    vd0, vg0, vs0 = (LD(v) for v in op)
    i_op, _, _, region = _ids(isP, vth, k, lam, vd0, vg0, vs0)
    gd_lin, gs_lin = 1 / LD(rd) + LD(gmin), 1 / LD(rs) + LD(gmin)

    def resid(vd, vs, i):
        return (vd - vd0) * gd_lin + (i - i_op), (vs - vs0) * gs_lin - (i - i_op), gd_lin, gs_lin
    theta = 2 * np.pi * np.arange(nt, dtype=LD) / nt
    samples = np.zeros((nt, 2), dtype=LD)
    for t in range(nt):
        vd, vs, reg = _newton(isP, vth, k, lam, rd, rs, vg0 + LD(amp) * np.cos(theta[t]), vd0, vs0, resid)
        assert reg == region, "the stage changed region within the period"
        samples[t] = vd - vd0, vs - vs0
    ph = np.zeros((3, 2), dtype=complex)
    for h in (1, 2, 3):
        re = 2 * (samples * np.cos(h * theta)[:, None]).sum(axis=0) / nt
        im = -2 * (samples * np.sin(h * theta)[:, None]).sum(axis=0) / nt
        ph[h - 1] = re.astype(np.float64) + 1j * im.astype(np.float64)
    return ph, region
