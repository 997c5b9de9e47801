#!/usr/bin/env python3
"""Periodic-noise benchmark: the output noise and noise figure of a mixer over Monte-Carlo instances.  By default
dbmixer.sp with its RF port rewritten in text into the AC excitation (as tools/pac_bench.py does, so that Engine.pac can be
timed on the same circuit) and a card `.PNOISE V(102,103) Vrf1+ LIN 16 90meg 110meg 1`: the LO at 900 MHz as the orbit
(K = 40), 16 output frequencies around the 100 MHz IF, n_side = 1.  DC operating point, Engine.pss, then Engine.pnoise,
timed against Engine.pac at 16 input frequencies around 800 MHz and against one shooting round of the periodic steady state,
all on the same circuit and batch.

Prints one JSON line per batch size:
  pss_round_ms          one shooting round (Engine.pss, max_rounds = 1), the unit the analyses are counted in
  pac_ms, pnoise_ms     the whole Engine.pac and Engine.pnoise calls (table uploads, every launch, the final wait)
  pnoise_over_round, pnoise_over_pac
  orbit_store_bytes     chunk K N 8 of the largest instance chunk, orbit_chunk its instances
  onoise                V^2/Hz between the output nodes at the --report frequency: min, median, max over the instances
  nf_db                 single-sideband noise figure 10 log10(onoise / (|gain_m|^2 4 k T Rs)) for m = -1 (the RF band
                        below the LO, f - f0) and m = +1 (above it, f + f0), from the source --src alone with its series
                        resistance --rs: min, median, max over the instances.  The port is driven differentially: against
                        both halves (twice the resistance, the same gain by symmetry) the figure is 3 dB lower.
Times are medians over --repeats after one warm-up, host wall clock around calls that end synchronised (the analyses
wait on their stream by definition).  DESIGN.md 8j has what was measured.

    python tools/pnoise_bench.py --B 4096 64
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
PNOISE_ORBIT_BUDGET = 256 << 20         # engine/pnoise.hpp


def mixer_text(src):
    text = open(os.path.join(ROOT, "tests", "golden", "dbmixer.sp")).read()
    for old, new in RF_REWRITE:
        if old not in text:
            raise SystemExit("dbmixer.sp no longer has the line %r" % old)
        text = text.replace(old, new, 1)
    return text.replace(".end", ".PNOISE V(102,103) %s LIN 16 90meg 110meg 1\n.end" % src, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--netlist", default=None, help="a netlist with AC sources and a .PNOISE card (default: the dbmixer variant)")
    ap.add_argument("--src", default="Vrf1+", help="the source of the default netlist's card")
    ap.add_argument("--rs", type=float, default=25.0, help="its series resistance, for the noise figure")
    ap.add_argument("--f0", type=float, default=900e6)
    ap.add_argument("--K", type=int, default=40)
    ap.add_argument("--pac-fcenter", type=float, default=800e6)
    ap.add_argument("--pac-fspan", type=float, default=20e6)
    ap.add_argument("--n-side", type=int, default=1)
    ap.add_argument("--temp", type=float, default=290.0)
    ap.add_argument("--B", type=int, nargs="+", default=[4096, 64])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.03)
    a = ap.parse_args()

    import torch
    from circuitsimulator_amd import Engine, Netlist

    nl = Netlist.from_file(a.netlist) if a.netlist else Netlist.from_text(mixer_text(a.src))
    card = nl.pnoise
    if card is None or card[0] < 0 or card[2] < 0:
        raise SystemExit("the netlist needs a .PNOISE card that names an output and a source")
    eng = Engine(nl, 0)
    eng.set_kernel("general")
    h = 1.0 / (a.f0 * a.K)
    freqs = nl.pnoise_freqs()
    F = len(freqs)
    pac_freqs = np.linspace(a.pac_fcenter - a.pac_fspan / 2, a.pac_fcenter + a.pac_fspan / 2, F) if F > 1 else np.array([a.pac_fcenter])
    report = F // 2
    probes = [e for e in card[:2] if e >= 0]
    kT4 = 4.0 * 1.380649e-23 * a.temp

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
            out["pac"] = eng.pac(params, s["x0"], freqs=pac_freqs, n_side=a.n_side, tstep=h, f0=a.f0, probes=probes)

        def pnoise():
            out["pnoise"] = eng.pnoise(params, s["x0"], n_side=a.n_side, tstep=h, f0=a.f0, temp=a.temp, contrib=True, side=True)

        res = {"netlist": os.path.basename(a.netlist) if a.netlist else "dbmixer.sp (RF port as AC excitation)", "B": B,
               "N": nl.n_unknowns, "S": len(nl.noise_sources), "K": a.K, "f0": a.f0, "F": F, "n_side": a.n_side, "temp": a.temp}
        res["pss_round_ms"], res["pss_round_ms_all"] = timed(one_round)
        res["pac_ms"], res["pac_ms_all"] = timed(pac)
        res["pnoise_ms"], res["pnoise_ms_all"] = timed(pnoise)
        res["pac_over_round"] = res["pac_ms"] / res["pss_round_ms"]
        res["pnoise_over_round"] = res["pnoise_ms"] / res["pss_round_ms"]
        res["pnoise_over_pac"] = res["pnoise_ms"] / res["pac_ms"]
        per = a.K * nl.n_unknowns * 8
        chunk = max(1, min(min(B, int(eng.stat("ac_chunk"))), PNOISE_ORBIT_BUDGET // per))
        res["orbit_chunk"], res["orbit_store_bytes"] = chunk, chunk * per
        st = (s["status"] | out["pnoise"]["status"]).cpu().numpy()
        res["flagged_instances"] = int((st != 0).sum())
        good = st == 0 if np.any(st == 0) else np.ones(B, dtype=bool)
        on = out["pnoise"]["onoise"].cpu().numpy()[report][good]
        res["report_hz"] = float(freqs[report])
        spread = lambda v: dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)))     # noqa: E731
        res["onoise"] = spread(on)
        if a.n_side >= 1:
            g = out["pnoise"]["gain"].cpu().numpy()[report]
            res["nf_db"] = {}
            for m in (-1, 1):
                g2 = np.abs(g[m + a.n_side][good]) ** 2
                res["nf_db"]["m%+d" % m] = spread(10.0 * np.log10(on / np.maximum(g2 * kT4 * a.rs, 1e-300)))
                res["gain_abs_m%+d" % m] = spread(np.sqrt(g2))
        print(json.dumps(res))


if __name__ == "__main__":
    main()
