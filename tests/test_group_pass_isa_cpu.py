"""What hipcc makes of the group kernels' Newton pass, checkable without a GPU: the register allocation of both group
kernels as the shipped libraries and the engine's JIT generate them (csim_codegen --engine-defaults: cover_mos=2) and
with the generator's own defaults, and where the pass waits for the LDS with and without wait_at_use."""
import os
import re
import subprocess

import pytest

from conftest import ROOT, netlist_path

CODEGEN = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "build", "csim_codegen")
SCHED = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "schedules")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def codegen():
    if not os.path.exists(CODEGEN):
        import __graft_entry__ as g
        g.build()
    assert os.path.exists(CODEGEN)
    return CODEGEN


def _isa(codegen, d, opts):
    """dbmixer with the shipped schedule and these generator options -> (kernel metadata, ISA text)"""
    d.mkdir()
    hip, asm = d / "x.hip", d / "x.s"
    args = [o for o in opts if o.startswith("--")] + [a for o in opts if not o.startswith("--") for a in ("--opt", o)]
    p = subprocess.run([codegen] + args + [netlist_path("dbmixer.sp"), os.path.join(SCHED, "dbmixer.sched"), str(hip)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    c = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", str(hip),
                        "-o", str(asm)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    text = asm.read_text()
    meta, name = {}, None
    for line in text.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.(private_segment_fixed_size|vgpr_spill_count|vgpr_count):\s+(\d+)", line)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return meta, text


def _newton_block(text, kernel="csim_tran_group_kernel"):
    """The Newton loop's body: the largest basic block of the kernel that lies in a loop of depth 2, and the lines from
    its label to the loop's backward branch"""
    lines = text.splitlines()
    a = lines.index(next(l for l in lines if l.startswith(kernel + ":")))
    b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[a:b]
    starts = [i for i, l in enumerate(body) if re.match(r"\.LBB\d+_\d+:", l) or re.match(r"; %bb\.\d+:", l)] + [len(body)]
    blocks = [(starts[k + 1] - starts[k], starts[k]) for k in range(len(starts) - 1) if "Depth=2" in body[starts[k]]]
    size, at = max(blocks)
    label = body[at].split(":")[0]
    assert size > 400, size                                  # the pass is one block of several hundred instructions
    # the back edge: the first conditional branch after the block that jumps to its label
    end = next(i for i in range(at + size, len(body)) if re.search(r"s_cbranch_\w+\s+" + re.escape(label) + r"\b", body[i]))
    return body[at:end + 1]


def _waits_after_last_staging_read(block):
    last = max(i for i, l in enumerate(block) if "ds_read2_b64" in l)
    return [l.strip() for l in block[last + 1:] if "s_waitcnt" in l and "lgkmcnt(0)" in l]


@pytest.mark.parametrize("opts", [["--engine-defaults"], []], ids=["shipped", "generator-defaults"])
def test_group_kernels_keep_their_register_allocation(codegen, tmp_path, opts):
    meta, text = _isa(codegen, tmp_path / "isa", opts)
    assert ("pivot checks' ballot above ran under the reads of the MOSFET inputs" in open(tmp_path / "isa" / "x.hip").read()) == bool(opts)
    for k in ("csim_tran_group_kernel", "csim_tran_group4_kernel"):
        assert meta[k]["private_segment_fixed_size"] == 0 and meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
    lean = meta["csim_tran_sched_kernel"]                    # the bounds of test_generated_dbmixer_kernel_register_allocation
    assert lean["private_segment_fixed_size"] <= 320 and lean["vgpr_spill_count"] <= 80, lean


def test_wait_at_use_leaves_no_full_lds_wait_in_front_of_the_back_edge(codegen, tmp_path):
    """With wait_at_use the staging rows are waited for inside the next pass's elimination: between the last staging
    read and the loop's back edge nothing waits for the LDS to drain.  Without it that wait is there -- which shows
    that this test can see it."""
    meta, text = _isa(codegen, tmp_path / "on", ["wait_at_use=1"])
    for k in ("csim_tran_group_kernel", "csim_tran_group4_kernel"):
        assert meta[k]["private_segment_fixed_size"] == 0 and meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
    assert _waits_after_last_staging_read(_newton_block(text)) == []
    _, text = _isa(codegen, tmp_path / "off", ["wait_at_use=0"])
    assert _waits_after_last_staging_read(_newton_block(text)) != []
