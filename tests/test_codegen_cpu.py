"""Host side of the kernel generator (no GPU): schedule-file parsing, what the generated
translation unit contains, and that a schedule which contradicts the circuit's constant entries
is turned into an unconditional fall-back instead of wrong code."""
import os
import subprocess

import pytest

from conftest import ROOT, netlist_path

CODEGEN = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "build", "csim_codegen")
SCHED = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "schedules")


@pytest.fixture(scope="module")
def codegen():
    if not os.path.exists(CODEGEN):
        import __graft_entry__ as g
        g.build()
    assert os.path.exists(CODEGEN)
    return CODEGEN


def _run(codegen, netlist, sched_text, tmp_path):
    sched = tmp_path / "x.sched"
    sched.write_text(sched_text)
    out = tmp_path / "x.hip"
    p = subprocess.run([codegen, netlist, str(sched), str(out)], capture_output=True, text=True)
    return p, (out.read_text() if out.exists() else "")


def test_shipped_schedule_files_generate_both_kernels(codegen, tmp_path):
    text = open(os.path.join(SCHED, "dbmixer.sched")).read()
    p, src = _run(codegen, netlist_path("dbmixer.sp"), text, tmp_path)
    assert p.returncode == 0, p.stderr
    topo = p.stdout.strip()
    assert len(topo) == 16 and os.path.exists(os.path.join(ROOT, "circuitsimulator_amd", "libcsim_sched_%s.so" % topo))
    for sym in ("csim_tran_sched_kernel(", "csim_dc_sched_kernel(", "csim_sched_launch(", "csim_sched_dc_launch(",
                "csim_sched_alts(", "csim_sched_dc_alts(", "csim_sched_topology(", "csim_sched_hash("):
        assert sym in src, sym
    assert "*nAlts = 1;" in src                      # one transient and one DC sequence
    # buffer.sched has several transient alternatives and no "dc" line: no DC kernel, a stub launcher
    text = open(os.path.join(SCHED, "buffer.sched")).read()
    p, src = _run(codegen, netlist_path("buffer.sp"), text, tmp_path)
    assert p.returncode == 0, p.stderr
    assert "csim_dc_sched_kernel(" not in src and "return -1;" in src
    assert src.count("// alternative schedule") >= 6


def test_group_plan_self_test_on_the_shipped_schedules(codegen):
    """The sixteen-lanes-per-instance plan (row placement, lane masks, staging rows, substitution order; for
    buffer.sp ten schedules over the FIRST one's placement, pivot rows at arbitrary lanes) run through its host
    interpreter on random term values against a dense elimination with the same pivots: csim_codegen
    --selftest-group exits 0 when every schedule agrees to 1e-9 and no all-lane candidate test could see a row it
    must not."""
    for flag in ("--selftest-group", "--selftest-group4"):          # sixteen and four lanes per instance
        for name in ("buffer", "dbmixer"):
            p = subprocess.run([codegen, flag, netlist_path(name + ".sp"), os.path.join(SCHED, name + ".sched")],
                               capture_output=True, text=True)
            assert p.returncode == 0, (flag, name, p.stdout[-400:], p.stderr[-400:])
            assert "group plan self test: worst relative difference" in p.stdout
            if flag.endswith("4"):
                # the four-lane kernel's rows are placed by a local search on the planned instruction count (generator
                # option place_search, bit 0); the interpreter above ran on THAT placement
                before, after = (float(v) for v in p.stdout.split("(weighted over the schedules) ")[1].split("\n")[0].split(" -> "))
                assert after < before, (name, before, after)
            else:
                assert "placement search" not in p.stdout
        assert p.stdout.count("group plan alt") >= 1
    p = subprocess.run([codegen, "--opt", "place_search=0", "--selftest-group4", netlist_path("dbmixer.sp"),
                        os.path.join(SCHED, "dbmixer.sched")], capture_output=True, text=True)
    assert p.returncode == 0 and "placement search" not in p.stdout and "fma=292" in p.stdout      # position-cyclic


def test_generated_library_carries_the_four_lane_kernel(codegen, tmp_path):
    """Circuits of up to 32 unknowns get the four-lanes-per-instance form of the group kernel too (16 instances
    per wavefront, tables in their own namespace, csim_sched_launch variant 4); its LDS image per instance is padded
    to 4 (mod 8) doubles so that the instances of a wavefront start on different banks."""
    for name in ("buffer", "dbmixer"):
        text = open(os.path.join(SCHED, name + ".sched")).read()
        p, src = _run(codegen, netlist_path(name + ".sp"), text, tmp_path)
        assert p.returncode == 0, p.stderr
        assert "csim_tran_group4_kernel(" in src and "namespace csim_q4 {" in src
        assert "csim_sched_group4_lanes(void) { return 4; }" in src and "if (variant == 4) {" in src
        per_inst = int(src.split("__shared__ double lds[16 * ")[1].split("]")[0])
        assert per_inst % 8 == 4 and per_inst * 16 * 8 <= 40 * 1024, per_inst       # four workgroups per CU
        assert "csim_sched_group4_per_cu(void) { return 64; }" in src          # ... which the engine's choice of kernel relies on
    p = subprocess.run([codegen, "--opt", "group4=0", netlist_path("dbmixer.sp"), os.path.join(SCHED, "dbmixer.sched"),
                        str(tmp_path / "no4.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    src = (tmp_path / "no4.hip").read_text()
    assert "csim_tran_group4_kernel(" not in src and "csim_sched_group4_lanes(void) { return 0; }" in src


def test_generator_options_are_part_of_the_library_identity(codegen, tmp_path):
    """--opt key=value changes the emitted code, so it must change the full hash a loaded library is checked
    against (the topology hash that names the file stays)."""
    sched = os.path.join(SCHED, "dbmixer.sched")
    outs = {}
    for opt in ("pipeline_mos=1", "pipeline_mos=0", "stage_ahead=5"):
        out = tmp_path / ("o_" + opt.replace("=", "_") + ".hip")
        p = subprocess.run([codegen, "--opt", opt, netlist_path("dbmixer.sp"), sched, str(out)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        src = out.read_text()
        full = src.split("csim_sched_hash(void) { return ")[1].split(";")[0]
        topo = src.split("csim_sched_topology(void) { return ")[1].split(";")[0]
        outs[opt] = (full, topo, src)
    assert len({v[0] for v in outs.values()}) == 3 and len({v[1] for v in outs.values()}) == 1
    # pipelined: the staging rows are loop-carried values read at the end of an iteration; otherwise named
    # constants read inside the elimination
    assert "double sv0 = ST[0 + g];" in outs["pipeline_mos=1"][2] and "const double sv0 = ST[0 + g];" not in outs["pipeline_mos=1"][2]
    assert "const double sv0 = ST[0 + g];" in outs["pipeline_mos=0"][2]


def test_schedule_file_syntax(codegen, tmp_path):
    nl = netlist_path("buffer.sp")
    ok = "0:9,1:10,5:11,7:12,8:12   # comment ; with a semicolon\n- ; 0:9\nDC 0:9,1:10\n"
    p, src = _run(codegen, nl, ok, tmp_path)
    assert p.returncode == 0, p.stderr
    assert "tried in this order: 0:9,1:10,5:11,7:12,8:12 ; - ; 0:9 ; dc 0:9,1:10" in src
    for bad in ("0:99\n",            # row out of range
                "5:3\n",             # pivot row above the diagonal
                "0;9\n",             # not column:row
                "# only a comment\n"):
        p, _ = _run(codegen, nl, bad, tmp_path)
        assert p.returncode != 0, bad


def test_schedule_contradicting_constant_entries_falls_back(codegen, tmp_path):
    """A schedule that demands a structurally ZERO pivot (buffer.sp: the branch row of inductor L2,
    position 12, has no entry in column 0 = node 103) must compile to 'always violated', not to a
    division by a zero that the code never materialised."""
    p, src = _run(codegen, netlist_path("buffer.sp"), "0:12\n", tmp_path)
    assert p.returncode == 0, p.stderr
    assert "scheduled pivot is a structural zero" in src


def test_generated_dbmixer_kernel_register_allocation(codegen, tmp_path):
    """Tripwire for the headline kernel's speed, checkable without a GPU: hipcc's register allocation of
    the 3000-instruction lane-per-instance body is fragile (one changed form of the pivot checks once
    took it from 46 to 243 spilled registers and halved the measured rate).  The shipped kernel must stay
    within a small scratch frame and must not lose the one-wave-per-SIMD register budget."""
    import re
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    text = open(os.path.join(SCHED, "dbmixer.sched")).read()
    p, src = _run(codegen, netlist_path("dbmixer.sp"), text, tmp_path)
    assert p.returncode == 0, p.stderr
    asm = tmp_path / "x.s"
    c = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        str(tmp_path / "x.hip"), "-o", str(asm)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    meta = {}
    name = None
    for line in asm.read_text().splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.(private_segment_fixed_size|vgpr_spill_count|vgpr_count):\s+(\d+)", line)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    lean = meta["csim_tran_sched_kernel"]
    assert lean["private_segment_fixed_size"] <= 320, lean         # bytes of scratch per lane (shipped: 180)
    assert lean["vgpr_spill_count"] <= 80, lean                    # shipped: 44
    assert meta["csim_dc_sched_kernel"]["private_segment_fixed_size"] == 0


def test_generated_source_changes_only_with_a_new_generator_revision(codegen):
    """kGeneratorRevision is part of the hash a cached / shipped library is checked against (codegen.cpp scheduleHash):
    emitted code that changes without a new revision would let a stale JIT cache entry pass for a current one.  The
    golden record (tools/update_generated_golden.py) holds the md5 of the generator's output for the two shipped
    schedules and the revision it was taken at."""
    import importlib.util
    import json
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("upd", os.path.join(ROOT, "tools", "update_generated_golden.py"))
    upd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(upd)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "generated_source.json")))
    now = upd.digests()
    if now != golden["source_md5"]:
        assert upd.revision() != golden["generator_revision"], \
            "the generator's output changed but kGeneratorRevision (codegen.hpp) did not: bump it"
        pytest.fail("generator output and revision changed: record them with tools/update_generated_golden.py")
    assert upd.revision() == golden["generator_revision"], "revision bumped without a change of the emitted code: re-record"


def test_every_kernel_family_changes_only_with_a_new_generator_revision(codegen):
    """As above, for the rest of the generator's output: the golden record's family_md5 holds the md5 for further
    generator option sets and for circuits that reach every other kernel family -- the gate-only-node and PULSE / PWL
    circuits, and linear circuits with a DC schedule (sixteen-lane and lane-per-instance linear kernels, linear DC)."""
    import importlib.util
    import json
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("upd", os.path.join(ROOT, "tools", "update_generated_golden.py"))
    upd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(upd)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "generated_source.json")))
    now = upd.family_digests()
    if now != golden["family_md5"]:
        assert upd.revision() != golden["generator_revision"], \
            "the generator's output changed but kGeneratorRevision (codegen.hpp) did not: bump it"
        pytest.fail("generator output and revision changed: record them with tools/update_generated_golden.py")
    assert upd.revision() == golden["generator_revision"], "revision bumped without a change of the emitted code: re-record"
