"""Generated netlists for the mid-size legs of tools/ac_bench.py and tools/noise_bench.py (--circuit): the amplifier
line and the RC ladder the README quotes for the time domain, with an AC source and a .NOISE card."""


def amplifier_line(stages):
    """Resistively loaded NMOS stages, RC coupled and DC biased: 2 * stages + 5 unknowns"""
    t = ["* amplifier line", "VDD vdd 0 DC 2.5", "Vin in 0 DC 0.9 AC 1", "Rg in g0 100"]
    for k in range(stages):
        t += ["MN%d d%d g%d 0 n 4e-6 1e-6 2" % (k, k, k), "RD%d vdd d%d %g" % (k, k, 4000 + 100 * k),
              "RC%d d%d g%d %g" % (k, k, k + 1, 3000 + 50 * k), "RB%d g%d 0 %g" % (k, k + 1, 6000 + 100 * k),
              "CG%d g%d 0 %ge-15" % (k, k + 1, 10 + k)]
    t += [".MODEL 2 VT 0.55 MU 3e-2 COX 2e-3 LAMBDA 0.04 CJ0 1e-14", ".TRAN 5e-12 2e-9",
          ".noise v(d%d) vin dec 10 1k 10g" % (stages - 1)]
    return "\n".join(t) + "\n"


def rc_ladder(N):
    """RC ladder with N unknowns: N - 2 sections and the source's branch current"""
    S = N - 2
    t = ["* RC ladder of %d sections" % S, "V1 n0 0 AC 1 0"]
    for k in range(1, S + 1):
        t += ["R%d n%d n%d 10" % (k, k - 1, k), "C%d n%d 0 1p" % (k, k)]
    t += [".noise v(n%d) v1 dec 10 1k 10g" % S]
    return "\n".join(t) + "\n"


CIRCUITS = {
    "amp65": lambda: amplifier_line(30),
    "amp95": lambda: amplifier_line(45),
    "ladder63": lambda: rc_ladder(63),
    "ladder257": lambda: rc_ladder(257),
}
