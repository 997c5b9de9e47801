#!/usr/bin/env python3
"""AC small-signal sweep benchmark: Monte-Carlo instances of a netlist, DC operating point, then the AC sweep, and
as a baseline the same systems as 2N x 2N real-equivalent systems [[G, -wC], [wC, G]] through csim_lu_solve_batch.

Prints one JSON line.  Times are medians over --repeats after one warm-up, taken with device events around the
enqueue-only calls (DC, AC sweep per kernel).  The baseline goes through the host-pointer csim_lu_solve_batch
(copies included) and is timed on the host; its kernel time is read from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d out -- python tools/ac_bench.py ...

    python tools/ac_bench.py --netlist tests/golden/dbmixer.sp --ac-source "Vrf1+ 112 212 SIN" --B 4096

The opt-in block kernel (ac_kernel=block, up to 1024 unknowns) on the generated mid-size circuits, with ac_lu_solve()
on one host core beside it (--host-solves systems through a g++ -O2 -ffp-contract=off build of ac_lu.hpp):
    python tools/ac_bench.py --circuit amp65 --kernel block --B 4096 --points 2 --no-baseline
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_circuits import CIRCUITS  # noqa: E402

HOST_DRIVER = r"""
#include <chrono>
#include <cstdio>
#include <vector>
#include "ac_lu.hpp"
// stdin: int32 n, count; then count systems of G [n][n], C [n][n] column-major, J re [n], J im [n], w.  stdout: seconds
int main()
{
    int32_t hd[2];
    if (std::fread(hd, sizeof(int32_t), 2, stdin) != 2) return 1;
    const int n = hd[0], count = hd[1], ld = n + 1;
    const size_t per = (size_t)2 * n * n + 2 * n + 1;
    std::vector<double> in(per * count), ar((size_t)n * ld), ai((size_t)n * ld), xr(n), xi(n);
    if (std::fread(in.data(), sizeof(double), in.size(), stdin) != in.size()) return 1;
    double sink = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < count; ++s) {
        const double *G = in.data() + per * s, *C = G + (size_t)n * n, *J = C + (size_t)n * n, w = J[2 * n];
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j) { ar[i * ld + j] = G[(size_t)j * n + i]; ai[i * ld + j] = w * C[(size_t)j * n + i]; }
            ar[i * ld + n] = J[i];
            ai[i * ld + n] = J[n + i];
        }
        csim::ac_lu_solve(n, ld, ar.data(), ai.data(), 1e-15, xr.data(), xi.data());
        sink += xr[n - 1];
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%.9g %g\n", sec, sink);
    return 0;
}
"""


def host_solves_per_s(G, Cm, J, omega, count):
    """ac_lu_solve() on one host core over `count` (instance, frequency) systems (load included) -> solves per second"""
    import subprocess
    import tempfile
    eng_dir = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine")
    B, n = J.shape
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "drv.cpp"), os.path.join(d, "drv")
        open(cpp, "w").write(HOST_DRIVER)
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-w", "-I" + eng_dir,
                        "-I" + os.path.join(ROOT, "include"), cpp, "-o", exe], check=True)
        blob = [np.array([n, count], dtype=np.int32).tobytes()]
        for s in range(count):
            b, w = s % B, omega[(s // B) % len(omega)]
            blob += [np.ascontiguousarray(G[b].T).tobytes(), np.ascontiguousarray(Cm[b].T).tobytes(),
                     np.ascontiguousarray(J[b].real).tobytes(), np.ascontiguousarray(J[b].imag).tobytes(),
                     np.array([w]).tobytes()]
        out = subprocess.run([exe], input=b"".join(blob), capture_output=True, check=True).stdout.decode()
    return count / float(out.split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--netlist", default=os.path.join(ROOT, "tests", "golden", "dbmixer.sp"))
    ap.add_argument("--ac-source", default="Vrf1+ 112 212 SIN",
                    help="text of the source line to give `AC 1` (inserted before its SIN)")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--points", type=int, default=10, help="points per decade")
    ap.add_argument("--fstart", type=float, default=1e3)
    ap.add_argument("--fstop", type=float, default=1e10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-freqs", type=int, default=71, help="frequencies solved by the real-equivalent baseline")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--circuit", choices=sorted(CIRCUITS), help="a generated netlist instead of --netlist")
    ap.add_argument("--kernel", choices=["block"], help="time this sweep kernel instead of wave / packed")
    ap.add_argument("--host-solves", type=int, default=0,
                    help="with --kernel block: that many (instance, frequency) systems through ac_lu_solve() on one host core")
    a = ap.parse_args()

    import torch
    from circuitsimulator_amd import Engine, Netlist, lu_solve_batch
    from circuitsimulator_amd.engine import ac_freqs

    if a.circuit:
        text = CIRCUITS[a.circuit]()
    else:
        text = open(a.netlist).read()
        if a.ac_source:
            assert a.ac_source in text, "source line not found: %s" % a.ac_source
            text = text.replace(a.ac_source, a.ac_source.replace(" SIN", " AC 1 SIN"), 1)
    nl = Netlist.from_text(text)
    eng = Engine(nl, 0)
    B, N = a.B, nl.n_unknowns
    f = ac_freqs("dec", a.points, a.fstart, a.fstop)
    F = len(f)
    params = eng.mc_params(12345, 0.05, 0, B)

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

    x = {}

    def dc():
        x["x"], _, x["st"] = eng.dc(params)
    dc_ms, dc_all = timed(dc)
    res = {"netlist": a.circuit or os.path.basename(a.netlist), "B": B, "N": N, "F": F, "systems": B * F, "dc_ms": dc_ms,
           "dc_ms_all": dc_all}
    outs = {}
    kernels = [a.kernel] if a.kernel else (["wave", "packed"] if N <= 32 else ["wave"])
    for k in kernels:
        eng.set_option("ac_kernel", k)

        def sweep():
            outs[k] = eng.ac(params, x["x"], freqs=f)
        ms, allms = timed(sweep)
        res["ac_%s_ms" % k] = ms
        res["ac_%s_ms_all" % k] = allms
        res["ac_%s_solves_per_s" % k] = B * F / (ms * 1e-3)
    eng.set_option("ac_kernel", "auto")
    if len(kernels) == 2:
        res["wave_packed_identical"] = bool(torch.equal(torch.view_as_real(outs["wave"][0]),
                                                        torch.view_as_real(outs["packed"][0])))
    res["ac_ms"] = min(res["ac_%s_ms" % k] for k in kernels)
    res["tiny_pivot_instances"] = int(((outs[kernels[0]][1] & 0x4) != 0).sum())

    if a.kernel and a.host_solves > 0:
        G, Cm, J = eng.ac_system(params[:, :min(B, 8)].contiguous(), x["x"][:, :min(B, 8)].contiguous())
        res["host_core_solves_per_s"] = host_solves_per_s(G.cpu().numpy(), Cm.cpu().numpy(), J.cpu().numpy(),
                                                          2.0 * math.pi * f, a.host_solves)

    if not a.no_baseline:
        G, Cm, J = eng.ac_system(params, x["x"])
        G, Cm, J = G.cpu().numpy(), Cm.cpu().numpy(), J.cpu().numpy()
        nb = min(a.baseline_freqs, F)
        pick = np.linspace(0, F - 1, nb).round().astype(int)
        rhs = np.concatenate([J.real, J.imag], axis=1)
        t_host = 0.0
        worst = 0.0
        ref = outs[kernels[-1]][0]
        for fi in pick:
            wC = (2.0 * math.pi * f[fi]) * Cm
            A = np.block([[G, -wC], [wC, G]])
            t0 = time.perf_counter()
            xs, _ = lu_solve_batch(A, rhs)
            t_host += time.perf_counter() - t0
            z = xs[:, :N] + 1j * xs[:, N:]
            r = ref[fi].cpu().numpy().T
            worst = max(worst, float(np.max(np.abs(r - z) / np.maximum(np.abs(z), 1e-15))))
        res["baseline_freqs"] = int(nb)
        res["baseline_host_ms_per_freq"] = 1e3 * t_host / nb
        res["baseline_max_rel_diff"] = worst
    print(json.dumps(res))


if __name__ == "__main__":
    main()
