#!/usr/bin/env python3
"""Record the md5 of the kernel generator's output with the options every library that runs is generated from
(csim_codegen --engine-defaults = GeneratorOptions::engineDefaults, codegen.hpp) together with kGeneratorRevision:
tests/golden/shipped_emission.json, compared by tests/test_shipped_emission_cpu.py.  tools/update_generated_golden.py
does the same for the generator's own defaults."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circuitsimulator_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shipped_emission.json")


def revision():
    text = open(os.path.join(CSRC, "engine", "codegen.hpp")).read()
    return int(re.search(r"kGeneratorRevision\s*=\s*(\d+)", text).group(1))


def generate(name, flags=("--engine-defaults",)):
    """-> (topology hash, source text) of a shipped circuit with its shipped schedule file"""
    gen = os.path.join(CSRC, "build", "csim_codegen")
    with tempfile.TemporaryDirectory() as d:
        hip = os.path.join(d, "x.hip")
        p = subprocess.run([gen] + list(flags) + [os.path.join(ROOT, "tests", "golden", name + ".sp"),
                                                  os.path.join(CSRC, "schedules", name + ".sched"), hip],
                           capture_output=True, text=True, check=True)
        return p.stdout.strip(), open(hip).read()


def digests():
    return {name: hashlib.md5(generate(name)[1].encode()).hexdigest() for name in ("buffer", "dbmixer")}


if __name__ == "__main__":
    rec = {"generator_revision": revision(), "source_md5": digests()}
    json.dump(rec, open(GOLDEN, "w"), indent=1, sort_keys=True)
    print("wrote", GOLDEN, rec)
    sys.exit(0)
