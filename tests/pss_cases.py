"""Circuits of the periodic-steady-state tests (tests/test_pss_cpu.py, tests/test_pss_gpu.py,
tests/test_pss_kernels_gpu.py), as netlist text, with the step and tone each is shot at.

  rc       RC low-pass (tests/golden/pss_rc.sp), tau = R C = 200 us = 200 periods of the 1 MHz tone, K = 32: linear and
           slow to settle.  The output's steady state is -(A / (w tau)) cos(w t); from the DC point 0 V the transient
           decays by A / (w tau) / 200 = 4e-6 A per period, so the amplitude is 100 V to put three periods of plain
           transient 4e-4 from closure, beyond 100 tol
  rlc      series R-L-C with the inductor's branch equation, resonance 1.125 MHz, R = 100 Ohm (Q = 0.7), K = 48.  What the
           first Newton update of a linear circuit leaves is the truncation offset of the damped step iteration
           (up to 1.2e-6 a step) carried through the powers of A; a resonant circuit amplifies it (with R = 10 Ohm,
           Q = 7, the reference is 2.6e-5 from closure after the first update and needs a third round, DESIGN.md
           8h), so the case that pins "two rounds" is the damped one
  cs       one-MOSFET common-source stage with a load capacitor and CJ0 > 0; the gate swings 0.4 V .. 2.0 V, which takes
           the device from cut-off through saturation into triode within the period (VT = 0.5 V, 2 mA of saturation
           current against 3 V / 2 kOhm), K = 64
  divider  two resistors: no state, W == 0, closed after one round, K = 16
"""
import os

import numpy as np

from conftest import GOLDEN

F0 = 1e6

RC = open(os.path.join(GOLDEN, "pss_rc.sp")).read()      # the one case with .TRAN and .HB cards: pss_host's defaults

RLC = """* series RLC
V1 in 0 SIN 0 1 1e6 0
R1 in a 100
L1 a b 10u
C1 b 0 2n
"""

CS = """* common-source stage driven from cut-off into triode
VDD vdd 0 DC 3
Vin g 0 SIN 1.2 0.8 1e6 0
RD vdd d 2k
CL d 0 100p
M1 d g 0 n 10e-6 1e-6 2
.MODEL 2 VT 0.5 MU 3e-2 COX 6e-3 LAMBDA 0.05 CJ0 4.0e-14
"""

DIVIDER = """* resistive divider
V1 in 0 SIN 0 1 1e6 0
R1 in out 1k
R2 out 0 1k
"""

# name -> (netlist text, K, n_harm)
CASES = {
    "rc": (RC, 32, 3),
    "rlc": (RLC, 48, 5),
    "cs": (CS, 64, 7),
    "divider": (DIVIDER, 16, 2),
}
LINEAR = ("rc", "rlc", "divider")
# the resonant RLC (R = 10 Ohm, Q = 7) beside the damped one: linear, and a third round is what it takes (above)
EXTRA = {"rlc_q7": (RLC.replace("R1 in a 100", "R1 in a 10"), 48, 5)}
assert "R1 in a 10\n" in EXTRA["rlc_q7"][0]
BATCHES = (1, 3, 65)            # 65 is no multiple of anything the kernels pack by

# The shipped netlists at B = 3, with a step coarse enough that K <= 200.  buffer.sp at its own 10 MHz input and its
# own .TRAN step: K = 100.  dbmixer.sp at its .hb fundamental of 100 MHz with h = 50 ps: K = 200 (22 samples per
# period of the 900 MHz LO).  With both steps the transient of the parent commit over that period from DC reports no
# CSIM_ST_TRAN_NONCONV for the three instances (asserted by the GPU test before it shoots).
SHIPPED = {
    "buffer.sp": dict(tstep=1e-9, f0=10e6, n_harm=3, K=100),
    "dbmixer.sp": dict(tstep=5e-11, f0=100e6, n_harm=5, K=200),
}
MC_SEED, MC_SIGMA = 20261020, 0.03


def case(name):
    return CASES[name] if name in CASES else EXTRA[name]


def tstep(name):
    return 1.0 / (F0 * case(name)[1])


def netlist(name):
    from circuitsimulator_amd import Netlist
    return Netlist.from_text(case(name)[0])


def shipped(name):
    from circuitsimulator_amd import Netlist
    return Netlist.from_file(os.path.join(GOLDEN, name))


def params(nl, B):
    """[P][B] Monte-Carlo table, instance 0 nominal"""
    return np.ascontiguousarray(nl.mc_params_host(MC_SEED, MC_SIGMA, 0, B))
