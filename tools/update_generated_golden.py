#!/usr/bin/env python3
"""Record the md5 of the kernel generator's output together with kGeneratorRevision (tests/golden/generated_source.json):
source_md5 for the shipped schedules, family_md5 for further generator option sets and circuits that reach every
other kernel family, the linear ones included.  tests/test_codegen_cpu.py compares: emitted code that changes without a new revision would let a stale JIT
cache entry pass for a current one."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "circuitsimulator_amd", "csrc")


def revision():
    text = open(os.path.join(CSRC, "engine", "codegen.hpp")).read()
    return int(re.search(r"kGeneratorRevision\s*=\s*(\d+)", text).group(1))


# (name, netlist text or fixture name, schedule text, generator options)
def shipped_cases():
    return [(name, name + ".sp", open(os.path.join(CSRC, "schedules", name + ".sched")).read(), [])
            for name in ("buffer", "dbmixer")]


# Every other kernel family the generator emits.  The linear circuits carry a DC schedule too, so that the linear DC
# kernel is emitted; their schedules need not be realistic, only reach the code paths.
def family_cases():
    from circuitsimulator_amd.workloads import rc_ladder_netlist
    linear = "-\ndc -\n"
    dbmixer = open(os.path.join(CSRC, "schedules", "dbmixer.sched")).read()
    out = [("gate_only_node", "gate_only_node.sp", "-", []),
           ("pulse_pwl", "pulse_pwl.sp", "-", [])]
    for opts in (["pipeline_mos=0", "stage_ahead=-1"], ["place_search=0"], ["group4=0"], ["near_band=0"]):
        out.append(("dbmixer " + " ".join(opts), "dbmixer.sp", dbmixer, opts))
    out += [("rc_ladder64", rc_ladder_netlist(64), linear, []),        # sixteen-lane linear kernel + its factor kernel
            ("rc_ladder600", rc_ladder_netlist(600), linear, []),      # lane-per-instance linear kernel
            ("rlc_mesh", "rlc_mesh.sp", linear, [])]                   # inductors, PULSE / PWL / SIN sources
    return out


def _digests(cases):
    out = {}
    gen = os.path.join(CSRC, "build", "csim_codegen")
    for name, netlist, sched, opts in cases:
        with tempfile.TemporaryDirectory() as d:
            if not netlist.endswith(".sp"):
                open(os.path.join(d, "x.sp"), "w").write(netlist)
                netlist = os.path.join(d, "x.sp")
            else:
                netlist = os.path.join(ROOT, "tests", "golden", netlist)
            sp = os.path.join(d, "x.sched")
            open(sp, "w").write(sched)
            hip = os.path.join(d, "x.hip")
            args = [a for o in opts for a in ("--opt", o)]
            subprocess.check_call([gen] + args + [netlist, sp, hip], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            out[name] = hashlib.md5(open(hip, "rb").read()).hexdigest()
    return out


def digests():
    return _digests(shipped_cases())


def family_digests():
    return _digests(family_cases())


if __name__ == "__main__":
    rec = {"generator_revision": revision(), "source_md5": digests(), "family_md5": family_digests()}
    path = os.path.join(ROOT, "tests", "golden", "generated_source.json")
    json.dump(rec, open(path, "w"), indent=1, sort_keys=True)
    print("wrote", path, rec)
    sys.exit(0)
