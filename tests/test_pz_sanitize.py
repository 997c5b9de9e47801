"""engine/pz.hpp under AddressSanitizer and UBSan: tests/sanitize/pz_sanitize_check.cpp, a stand-alone program with its
own main() and exactly sized heap buffers, compiled for the host and run once.  Nothing is preloaded and nothing is
loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_sequential_pole_routine_is_clean_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "sanitize", "pz_sanitize_check.cpp")
    exe = tmp_path / "pz_sanitize_check"
    c = subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-std=c++17",
                        "-I" + os.path.join(ROOT, "circuitsimulator_amd", "csrc", "engine"),
                        "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    assert len(p.stdout.splitlines()) == 3
