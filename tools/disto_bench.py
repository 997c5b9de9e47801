#!/usr/bin/env python3
"""Distortion sweep benchmark: Monte-Carlo instances of a netlist, DC operating point, then the distortion sweep over
the grid of a .DISTO card and, in the same run, the AC sweep (Engine.ac, every unknown) on the same B, F and operating
points.

Prints one JSON line: (instance x frequency) per second of both sweeps and their ratio, per kernel.  One distortion
point is three loads and factorisations plus O(M) work, so the ratio is expected near one third.  Times are medians
over --repeats after one warm-up, taken with device events around the enqueue-only calls.  Kernel times come from a
profiler run of its own:
    rocprofv3 --kernel-trace --stats -d out -- python tools/disto_bench.py ...

    python tools/disto_bench.py --netlist tests/golden/dbmixer.sp --ac-source "Vrf1+ 112 212 SIN" \\
        --card ".DISTO V(102,103) DEC 10 1k 10g" --B 4096
    python tools/disto_bench.py --netlist tests/golden/buffer.sp --ac-source "Vin 101 0 SIN" \\
        --card ".DISTO V(118) DEC 10 1k 10g" --B 4096
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--netlist", default=os.path.join(ROOT, "tests", "golden", "dbmixer.sp"))
    ap.add_argument("--ac-source", default="Vrf1+ 112 212 SIN",
                    help="text of the source line to give `AC 1` (inserted before its SIN); '' = the netlist's own")
    ap.add_argument("--card", default=".DISTO V(102,103) DEC 10 1k 10g",
                    help="the .DISTO card added to the netlist ('' = the netlist's own)")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-phasors", action="store_true", help="HD2 and HD3 only: do not write x1, x2, x3")
    a = ap.parse_args()

    import torch
    from circuitsimulator_amd import Engine, Netlist

    text = open(a.netlist).read()
    if a.ac_source:
        assert a.ac_source in text, "source line not found: %s" % a.ac_source
        text = text.replace(a.ac_source, a.ac_source.replace(" SIN", " AC 1 SIN"), 1)
    if a.card:
        text = text.rstrip("\n") + "\n" + a.card + "\n"
    nl = Netlist.from_text(text)
    assert nl.disto is not None, "no .DISTO card"
    eng = Engine(nl, 0)
    B, N = a.B, nl.n_unknowns
    f = nl.disto_freqs()
    F, M = len(f), len(nl.disto_devices)
    params = eng.mc_params(12345, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    torch.cuda.synchronize()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), ms

    res = {"netlist": os.path.basename(a.netlist), "card": a.card, "B": B, "N": N, "F": F, "M": M, "systems": B * F,
           "phasors": not a.no_phasors}
    outs = {}
    kernels = ["wave", "packed"] if N <= 32 else ["wave"]
    for k in kernels:
        eng.set_option("ac_kernel", k)

        def disto():
            outs["disto_" + k] = eng.disto(params, x, want_h=not a.no_phasors)

        def ac():
            outs["ac_" + k] = eng.ac(params, x, freqs=f)
        for name, fn in (("disto", disto), ("ac", ac)):
            ms, allms = timed(fn)
            res["%s_%s_ms" % (name, k)] = ms
            res["%s_%s_ms_all" % (name, k)] = allms
            res["%s_%s_points_per_s" % (name, k)] = B * F / (ms * 1e-3)
        res["disto_over_ac_%s" % k] = res["disto_%s_points_per_s" % k] / res["ac_%s_points_per_s" % k]
    eng.set_option("ac_kernel", "auto")
    if len(kernels) == 2:
        res["wave_packed_identical"] = bool(torch.equal(outs["disto_wave"]["hd"], outs["disto_packed"]["hd"]))
    best = kernels[-1]
    res["disto_points_per_s"] = res["disto_%s_points_per_s" % best]
    res["ac_points_per_s"] = res["ac_%s_points_per_s" % best]
    res["disto_over_ac"] = res["disto_over_ac_%s" % best]
    hd = outs["disto_" + best]["hd"]
    res["tiny_pivot_instances"] = int(((outs["disto_" + best]["status"] & 0x4) != 0).sum())
    res["hd2_median"], res["hd3_median"] = float(hd[:, 0].median()), float(hd[:, 1].median())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
