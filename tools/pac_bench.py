#!/usr/bin/env python3
"""Periodic-AC benchmark: the conversion gain of a mixer over Monte-Carlo instances.  By default dbmixer.sp with its RF
port rewritten in text into the AC excitation (RF1+/- `DC 0.6 AC 0.5 0|180`, RF2+/- `DC 0`), the LO at 900 MHz as the
orbit (K = 40), 16 input frequencies around 800 MHz, n_side = 1: DC operating point, Engine.pss, then Engine.pac, timed
against one shooting round of the periodic steady state on the same circuit and batch.

Prints one JSON line per batch size:
  pss_round_ms          one shooting round (Engine.pss, max_rounds = 1), the unit the analysis is counted in
  pac_ms                the whole Engine.pac call: the W_K launch, then per frequency chunk two period passes and the
                        closure solve, table uploads and the final wait
  pac_over_round        their ratio (expected near 3 for F <= 32: three integrations of the period)
  gain_db               20 log10 of |P_-1| between the .PLOTNV nodes at the --report frequency: min, median, max over
                        the instances; gain_first: the first instances' values as numbers
Times are medians over --repeats after one warm-up, host wall clock around calls that end synchronised (both analyses
wait on their stream by definition).  DESIGN.md 8i has what was measured.

    python tools/pac_bench.py --B 4096 64
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

RF_REWRITE = (("Vrf1+ 112 212 SIN 0.6 0.01 800e6 180", "Vrf1+ 112 212 DC 0.6 AC 0.5 0"),
              ("Vrf2+ 212 0 SIN 0  0.01 600e6 180", "Vrf2+ 212 0 DC 0"),
              ("Vrf1- 113 213 SIN 0.6  0.01 800e6 0", "Vrf1- 113 213 DC 0.6 AC 0.5 180"),
              ("Vrf2- 213 0 SIN 0 0.01 600e6 0", "Vrf2- 213 0 DC 0"))


def mixer_text():
    text = open(os.path.join(ROOT, "tests", "golden", "dbmixer.sp")).read()
    for old, new in RF_REWRITE:
        if old not in text:
            raise SystemExit("dbmixer.sp no longer has the line %r" % old)
        text = text.replace(old, new, 1)
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--netlist", default=None, help="a netlist with AC sources and .PLOTNV nodes (default: the dbmixer variant)")
    ap.add_argument("--f0", type=float, default=900e6)
    ap.add_argument("--K", type=int, default=40)
    ap.add_argument("--fcenter", type=float, default=800e6)
    ap.add_argument("--fspan", type=float, default=20e6)
    ap.add_argument("--F", type=int, default=16)
    ap.add_argument("--n-side", type=int, default=1)
    ap.add_argument("--B", type=int, nargs="+", default=[4096, 64])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.03)
    a = ap.parse_args()

    import torch
    from circuitsimulator_amd import Engine, Netlist

    nl = Netlist.from_file(a.netlist) if a.netlist else Netlist.from_text(mixer_text())
    if len(nl.probes) < 2:
        raise SystemExit("the netlist needs two .PLOTNV nodes (the differential output)")
    eng = Engine(nl, 0)
    eng.set_kernel("general")
    h = 1.0 / (a.f0 * a.K)
    freqs = np.linspace(a.fcenter - a.fspan / 2, a.fcenter + a.fspan / 2, a.F) if a.F > 1 else np.array([a.fcenter])
    report = int(np.argmin(np.abs(freqs - a.fcenter)))
    probes = list(nl.probes[:2])

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

    for B in a.B:
        params = eng.mc_params(12345, a.sigma, 0, B)
        x_dc, _, _ = eng.dc(params)
        s = eng.pss(params, x_dc, tstep=h, f0=a.f0, n_harm=0, probes=probes)
        torch.cuda.synchronize()
        out = {}

        def one_round():
            out["round"] = eng.pss(params, x_dc, tstep=h, f0=a.f0, n_harm=0, probes=probes, max_rounds=1)

        def pac():
            out["pac"] = eng.pac(params, s["x0"], freqs=freqs, n_side=a.n_side, tstep=h, f0=a.f0, probes=probes)

        res = {"netlist": os.path.basename(a.netlist) if a.netlist else "dbmixer.sp (RF port as AC excitation)", "B": B,
               "N": nl.n_unknowns, "K": a.K, "f0": a.f0, "F": len(freqs), "n_side": a.n_side}
        res["pss_round_ms"], res["pss_round_ms_all"] = timed(one_round)
        res["pac_ms"], res["pac_ms_all"] = timed(pac)
        res["pac_over_round"] = res["pac_ms"] / res["pss_round_ms"]
        rounds = s["rounds"].cpu().numpy()
        st = (s["status"] | out["pac"]["status"]).cpu().numpy()
        res["pss_rounds"] = dict(min=int(rounds.min()), median=float(np.median(rounds)), max=int(rounds.max()))
        res["flagged_instances"] = int((st != 0).sum())
        p = out["pac"]["p"].cpu().numpy()                       # [F][2 n_side + 1][2][B]
        g = np.abs(p[report, a.n_side - 1, 0, :] - p[report, a.n_side - 1, 1, :]) if a.n_side >= 1 else np.zeros(B)
        ok = g[st == 0] if np.any(st == 0) else g
        db = 20.0 * np.log10(np.maximum(ok, 1e-300))
        res["report_hz"] = float(freqs[report])
        res["gain_db"] = dict(min=float(db.min()), median=float(np.median(db)), max=float(db.max()))
        res["gain_first"] = [float(v) for v in g[:8]]
        print(json.dumps(res))


if __name__ == "__main__":
    main()
