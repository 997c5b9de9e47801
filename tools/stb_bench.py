#!/usr/bin/env python3
"""Loop-gain sweep benchmark: Monte-Carlo instances of a netlist with a .STB card, DC operating point, then the loop-gain
sweep with margins over the card's grid and, in the same run, the AC sweep (Engine.ac, every unknown) on the same B, F
and operating points (the AC stimulus is an `AC 1` given to the probe, which the loop-gain analysis ignores).

Prints one JSON line: milliseconds and (instance x frequency) per second of both sweeps and their ratio, per kernel, the
sweep with and without margins (their difference holds the margins kernel and the allocation of its outputs), and the
distribution of the phase margin.  One loop-gain point is one load and factorisation with one more right-hand side and one
more back substitution than an AC point, and a scalar stored instead of N values; DESIGN.md 8g has what was measured.
Times are medians over --repeats after one warm-up, taken with device events around the
enqueue-only calls.  Kernel times come from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d out -- python tools/stb_bench.py ...

    python tools/stb_bench.py --netlist tests/golden/stb_cs_loop.sp --B 4096
    python tools/stb_bench.py --netlist tests/golden/stb_cs_loop.sp --B 64
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
    ap.add_argument("--netlist", default=os.path.join(ROOT, "tests", "golden", "stb_cs_loop.sp"))
    ap.add_argument("--probe-line", default="Vprobe d fb DC 0",
                    help="text of the probe's line, given `AC 1` for the AC sweep beside it")
    ap.add_argument("--card", default="", help="a .STB card added to the netlist ('' = the netlist's own)")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()

    import torch
    from circuitsimulator_amd import Engine, Netlist

    text = open(a.netlist).read()
    assert a.probe_line in text, "probe line not found: %s" % a.probe_line
    text = text.replace(a.probe_line, a.probe_line + " AC 1", 1)
    if a.card:
        text = text.rstrip("\n") + "\n" + a.card + "\n"
    nl = Netlist.from_text(text)
    assert nl.stb is not None, "no .STB card"
    eng = Engine(nl, 0)
    B, N = a.B, nl.n_unknowns
    f = nl.stb_freqs()
    F = len(f)
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

    res = {"netlist": os.path.basename(a.netlist), "B": B, "N": N, "F": F, "systems": B * F}
    outs = {}
    kernels = ["wave", "packed"] if N <= 32 else ["wave"]
    for k in kernels:
        eng.set_option("ac_kernel", k)

        def stb():
            outs["stb_" + k] = eng.stb(params, x)

        def stb_plain():
            outs["plain_" + k] = eng.stb(params, x, margins=False)

        def ac():
            outs["ac_" + k] = eng.ac(params, x, freqs=f)
        for name, fn in (("stb", stb), ("stb_no_margins", stb_plain), ("ac", ac)):
            ms, allms = timed(fn)
            res["%s_%s_ms" % (name, k)] = ms
            res["%s_%s_ms_all" % (name, k)] = allms
            res["%s_%s_points_per_s" % (name, k)] = B * F / (ms * 1e-3)
        # a difference of two medians: the margins kernel plus the allocation and zeroing of its two output tensors,
        # not the kernel's own time (that comes from the profiler run above)
        res["with_minus_without_margins_%s_ms" % k] = res["stb_%s_ms" % k] - res["stb_no_margins_%s_ms" % k]
        res["stb_over_ac_ms_%s" % k] = res["stb_%s_ms" % k] / res["ac_%s_ms" % k]
    eng.set_option("ac_kernel", "auto")
    if len(kernels) == 2:
        res["wave_packed_identical"] = bool(torch.equal(torch.view_as_real(outs["stb_wave"]["t"]),
                                                        torch.view_as_real(outs["stb_packed"]["t"])))
    best = kernels[-1]
    res["stb_ms"], res["ac_ms"], res["stb_over_ac_ms"] = res["stb_%s_ms" % best], res["ac_%s_ms" % best], res["stb_over_ac_ms_%s" % best]
    r = outs["stb_" + best]
    pm = r["pm"][(r["found"] & 1) != 0].cpu().numpy()
    res["tiny_pivot_instances"] = int(((r["status"] & 0x4) != 0).sum())
    res["unity_crossings_found"] = int(len(pm))
    res["phase_crossings_found"] = int(((r["found"] & 2) != 0).sum())
    if len(pm):
        res["pm_deg"] = dict(min=float(pm.min()), p05=float(np.percentile(pm, 5)), median=float(np.median(pm)),
                             p95=float(np.percentile(pm, 95)), max=float(pm.max()))
        res["share_pm_above_60"] = float(np.mean(pm > 60.0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
