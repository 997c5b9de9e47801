#!/usr/bin/env python3
"""Noise sweep benchmark: Monte-Carlo instances of a netlist, DC operating point, then the noise sweep over the grid
of a .NOISE card and, in the same run, the AC sweep (Engine.ac, every unknown) on the same B, F and operating points.

Prints one JSON line: (instance x frequency) per second of both sweeps and their ratio, per kernel.  Times are
medians over --repeats after one warm-up, taken with device events around the enqueue-only calls.  Kernel times come
from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d out -- python tools/noise_bench.py ...

    python tools/noise_bench.py --netlist tests/golden/dbmixer.sp --ac-source "Vrf1+ 112 212 SIN" \\
        --card ".NOISE V(102,103) Vrf1+ DEC 10 1k 10g" --B 4096

The opt-in block kernel (ac_kernel=block, up to 1024 unknowns) on the generated mid-size circuits (their own card):
    python tools/noise_bench.py --circuit amp65 --kernel block --B 4096
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_circuits import CIRCUITS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--netlist", default=os.path.join(ROOT, "tests", "golden", "dbmixer.sp"))
    ap.add_argument("--ac-source", default="Vrf1+ 112 212 SIN",
                    help="text of the source line to give `AC 1` (inserted before its SIN), for the AC sweep")
    ap.add_argument("--card", default=".NOISE V(102,103) Vrf1+ DEC 10 1k 10g",
                    help="the .NOISE card added to the netlist ('' = the netlist's own)")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--contrib", action="store_true", help="also write the per-generator contributions")
    ap.add_argument("--circuit", choices=sorted(CIRCUITS), help="a generated netlist (with its card) instead of --netlist")
    ap.add_argument("--kernel", choices=["block"], help="time this sweep kernel instead of wave / packed")
    ap.add_argument("--points", type=int, default=0, help="with --circuit: points per decade of its card (0 = 10)")
    a = ap.parse_args()

    import torch
    from circuitsimulator_amd import Engine, Netlist

    if a.circuit:
        text = CIRCUITS[a.circuit]()
        if a.points:
            text = text.replace(" dec 10 ", " dec %d " % a.points)
        a.card = [ln for ln in text.splitlines() if ln.startswith(".noise")][0]
    else:
        text = open(a.netlist).read()
        if a.ac_source:
            assert a.ac_source in text, "source line not found: %s" % a.ac_source
            text = text.replace(a.ac_source, a.ac_source.replace(" SIN", " AC 1 SIN"), 1)
        if a.card:
            text = text.rstrip("\n") + "\n" + a.card + "\n"
    nl = Netlist.from_text(text)
    assert nl.noise is not None, "no .NOISE card"
    eng = Engine(nl, 0)
    B, N = a.B, nl.n_unknowns
    f = nl.noise_freqs()
    F, S = len(f), len(nl.noise_sources)
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

    res = {"netlist": a.circuit or os.path.basename(a.netlist), "card": a.card, "B": B, "N": N, "F": F, "S": S, "systems": B * F,
           "contrib": bool(a.contrib)}
    outs = {}
    kernels = [a.kernel] if a.kernel else (["wave", "packed"] if N <= 32 else ["wave"])
    for k in kernels:
        eng.set_option("ac_kernel", k)

        def noise():
            outs["noise_" + k] = eng.noise(params, x, contrib=a.contrib)

        def ac():
            outs["ac_" + k] = eng.ac(params, x, freqs=f)
        for name, fn in (("noise", noise), ("ac", ac)):
            ms, allms = timed(fn)
            res["%s_%s_ms" % (name, k)] = ms
            res["%s_%s_ms_all" % (name, k)] = allms
            res["%s_%s_solves_per_s" % (name, k)] = B * F / (ms * 1e-3)
        res["noise_over_ac_%s" % k] = res["noise_%s_solves_per_s" % k] / res["ac_%s_solves_per_s" % k]
    eng.set_option("ac_kernel", "auto")
    if len(kernels) == 2:
        res["wave_packed_identical"] = bool(torch.equal(outs["noise_wave"]["onoise"], outs["noise_packed"]["onoise"]))
    best = kernels[-1]
    res["noise_solves_per_s"] = res["noise_%s_solves_per_s" % best]
    res["ac_solves_per_s"] = res["ac_%s_solves_per_s" % best]
    res["noise_over_ac"] = res["noise_over_ac_%s" % best]
    on = outs["noise_" + best]["onoise"]
    res["tiny_pivot_instances"] = int(((outs["noise_" + best]["status"] & 0x4) != 0).sum())
    res["onoise_min"], res["onoise_max"] = float(on.min()), float(on.max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
