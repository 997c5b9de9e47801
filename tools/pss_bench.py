#!/usr/bin/env python3
"""Periodic-steady-state benchmark: Monte-Carlo instances of a netlist, DC operating point, then Engine.pss at a tone
and a step, against the plain transient of the general kernel on the same B and K.

Prints one JSON line:
  round_ms              one shooting round (max_rounds = 1: the period kernel with its sensitivity and DFT, the update
                        kernel, the table upload and the counter read-back)
  tran_period_ms        K steps of the general kernel's transient from the same states (Engine.tran, no waveform)
  round_over_tran       their ratio: what the N-column elimination per step costs on top of the step
  pss_ms, rounds        the whole analysis at the engine's pss_tol, and the rounds the instances took
  tran_periods_to_close periods of plain transient from DC until every instance that shooting closed is within --tol
                        of closure (counted first, untimed, capped at --max-periods); tran_to_close_ms: that many
                        periods as one transient call
Times are medians over --repeats after one warm-up, host wall clock around calls that end synchronised (the analysis
waits on its stream by definition).  DESIGN.md 8h has what was measured.

    python tools/pss_bench.py --netlist tests/golden/dbmixer.sp --f0 100e6 --tstep 5e-11 --B 4096
    python tools/pss_bench.py --netlist tests/golden/buffer.sp --f0 10e6 --tstep 1e-9 --B 64
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--netlist", default=os.path.join(ROOT, "tests", "golden", "dbmixer.sp"))
    ap.add_argument("--f0", type=float, default=100e6)
    ap.add_argument("--tstep", type=float, default=5e-11)
    ap.add_argument("--n-harm", type=int, default=5)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-periods", type=int, default=400)
    ap.add_argument("--sigma", type=float, default=0.03)
    ap.add_argument("--tol", type=float, default=2e-6, help="closure asked of both (the engine's pss_tol by default)")
    a = ap.parse_args()
    tol = a.tol

    import torch
    from circuitsimulator_amd import Engine, Netlist, pss_num_steps

    nl = Netlist.from_file(a.netlist)
    eng = Engine(nl, 0)
    eng.set_kernel("general")
    B, N = a.B, nl.n_unknowns
    K = pss_num_steps(a.tstep, a.f0)
    params = eng.mc_params(12345, a.sigma, 0, B)
    x_dc, _, _ = eng.dc(params)
    probes = nl.probes if nl.probes else None
    torch.cuda.synchronize()
    dev = x_dc.device

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), ms

    out = {}

    def one_round():
        out["round"] = eng.pss(params, x_dc, tstep=a.tstep, f0=a.f0, n_harm=a.n_harm, probes=probes, max_rounds=1)

    def whole():
        out["pss"] = eng.pss(params, x_dc, tstep=a.tstep, f0=a.f0, n_harm=a.n_harm, probes=probes, tol=tol)

    def tran_period(x=None, periods=1):
        x = x_dc.clone() if x is None else x
        it = torch.zeros(B, dtype=torch.int64, device=dev)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        eng.tran(params, x, a.tstep, 0, periods * K, it, st)
        return x

    res = {"netlist": os.path.basename(a.netlist), "B": B, "N": N, "K": K, "f0": a.f0, "tstep": a.tstep}
    for name, fn in (("round", one_round), ("tran_period", tran_period), ("pss", whole)):
        ms, allms = timed(fn)
        res[name + "_ms"], res[name + "_ms_all"] = ms, allms
    res["round_over_tran"] = res["round_ms"] / res["tran_period_ms"]
    r = out["pss"]
    rounds = r["rounds"].cpu().numpy()
    status = r["status"].cpu().numpy()
    res["rounds"] = dict(min=int(rounds.min()), median=float(np.median(rounds)), max=int(rounds.max()))
    res["pss_nonconv_instances"] = int(((status & 0x200) != 0).sum())
    res["pss_singular_instances"] = int(((status & 0x400) != 0).sum())
    res["tran_nonconv_instances"] = int(((status & 0x2) != 0).sum())
    res["tol"] = tol
    closed = torch.from_numpy((status & 0x600) == 0).to(dev)
    # the plain transient to the same closure.  First, untimed, how many periods it takes: period after period from DC,
    # each restarted at step 0 (the sources' periodic extension, as the analysis defines it).  Then that many periods
    # as one transient call, timed like the others: no copies, no read-backs between the periods.
    x = x_dc.clone()
    periods, worst = 0, float("inf")
    while periods < a.max_periods:
        prev = x.clone()
        x = tran_period(x)
        periods += 1
        worst = float((x - prev).abs().amax(dim=0)[closed].max().item()) if bool(closed.any()) else 0.0
        if worst < tol:
            break
    res["tran_to_close_ms"], res["tran_to_close_ms_all"] = timed(lambda: tran_period(periods=periods))
    res["tran_periods_to_close"] = periods
    res["tran_closure_reached"] = worst
    res["tran_to_close_over_pss"] = res["tran_to_close_ms"] / res["pss_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
