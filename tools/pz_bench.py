#!/usr/bin/env python3
"""Pole analysis benchmark: Monte-Carlo instances of a netlist, DC operating point, then the poles of every instance
(Engine.pz) and, in the same run, the AC sweep (Engine.ac, every unknown) at 16 frequencies on the same instances and
operating points.

Prints one JSON line per B: milliseconds of both calls (medians of --repeats after one warm-up, device events around the
enqueue-only calls), their ratio, the kernel's dynamic LDS and how many of its workgroups that lets a compute unit
hold, and what the poles say (how many, how many instances have one in the right half plane, the spread of the
dominant pole).  DESIGN.md 8k has what was measured.  Kernel times come from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d out -- python tools/pz_bench.py ...

    python tools/pz_bench.py                                  # dbmixer.sp at B = 64 and B = 4096
    python tools/pz_bench.py --netlist tests/golden/ac_rc_ladder.sp --ac-source "" --B 4096 --fmax 1e12
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LDS_PER_CU = 160 * 1024


def pz_lds_bytes(N):
    """kernels_pz.hip: two planes of N rows at the odd leading dimension N | 1, five vectors of 64 doubles"""
    return 8 * (2 * N * (N | 1) + 5 * 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--netlist", default=os.path.join(ROOT, "tests", "golden", "dbmixer.sp"))
    ap.add_argument("--ac-source", default="Vrf1+ 112 212 SIN",
                    help="text of the source line to give `AC 1` for the AC sweep (inserted before its SIN); '' = the netlist's own")
    ap.add_argument("--B", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--fmax", type=float, default=1e12)
    ap.add_argument("--sigma", type=float, default=0.03, help="relative Monte-Carlo spread")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()

    import torch
    from circuitsimulator_amd import Engine, Netlist

    text = open(a.netlist).read()
    if a.ac_source:
        assert a.ac_source in text, "source line not found: %s" % a.ac_source
        text = text.replace(a.ac_source, a.ac_source.replace(" SIN", " AC 1 SIN"), 1)
    nl = Netlist.from_text(text)
    eng = Engine(nl, 0)
    N = nl.n_unknowns
    f = np.logspace(6, 10, 16)

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

    for B in a.B:
        params = eng.mc_params(12345, a.sigma, 0, B)
        x, _, _ = eng.dc(params)
        torch.cuda.synchronize()
        out = {}

        def pz():
            out["pz"] = eng.pz(params, x, fmax=a.fmax)

        def ac():
            out["ac"] = eng.ac(params, x, freqs=f)
        res = {"netlist": os.path.basename(a.netlist), "B": B, "N": N, "fmax": a.fmax, "ac_F": len(f),
               "lds_bytes": pz_lds_bytes(N), "workgroups_per_cu_by_lds": LDS_PER_CU // pz_lds_bytes(N)}
        res["pz_ms"], res["pz_ms_all"] = timed(pz)
        res["ac_ms"], res["ac_ms_all"] = timed(ac)
        res["pz_over_ac_ms"] = res["pz_ms"] / res["ac_ms"]
        res["pz_us_per_instance"] = 1e3 * res["pz_ms"] / B
        r = out["pz"]
        st, npo = r["status"].cpu().numpy(), r["n_poles"].cpu().numpy()
        res["flagged_instances"] = int((st != 0).sum())
        res["n_poles"] = dict(min=int(npo.min()), max=int(npo.max()))
        res["instances_with_rhp_pole"] = int((r["n_rhp"] > 0).sum())
        dom = r["poles"][0].cpu().numpy()
        dom = dom[~np.isnan(dom.real)]
        if len(dom):
            res["dominant_pole_re"] = dict(min=float(dom.real.min()), median=float(np.median(dom.real)), max=float(dom.real.max()))
        print(json.dumps(res))


if __name__ == "__main__":
    main()
