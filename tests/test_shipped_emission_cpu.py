"""The emission that runs: every shipped library and every library the engine specialises at run time is generated from
GeneratorOptions::engineDefaults (codegen.hpp), which differs from the generator's own defaults where a measured choice
was added without changing what the defaults emit.  tests/test_codegen_cpu.py ties the defaults' output to
kGeneratorRevision; this file does the same for the emission that runs, and checks that the shipped libraries are that
emission."""
import ctypes
import importlib.util
import json
import os

import pytest

from conftest import ROOT

CODEGEN = os.path.join(ROOT, "circuitsimulator_amd", "csrc", "build", "csim_codegen")


@pytest.fixture(scope="module")
def upd():
    if not os.path.exists(CODEGEN):
        import __graft_entry__ as g
        g.build()
    spec = importlib.util.spec_from_file_location("upd_shipped", os.path.join(ROOT, "tools", "update_shipped_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _full_hash(src):
    return int(src.split("csim_sched_hash(void) { return ")[1].split("ull;")[0], 16)


def test_shipped_emission_changes_only_with_a_new_generator_revision(upd):
    """Emitted code that changes without a new revision would let a stale JIT cache entry pass for a current one."""
    golden = json.load(open(upd.GOLDEN))
    now = upd.digests()
    if now != golden["source_md5"]:
        assert upd.revision() != golden["generator_revision"], \
            "the shipped emission changed but kGeneratorRevision (codegen.hpp) did not: bump it"
        pytest.fail("shipped emission and revision changed: record them with tools/update_shipped_golden.py")
    assert upd.revision() == golden["generator_revision"], "revision bumped without a change of the emitted code: re-record"


@pytest.mark.parametrize("name", ["buffer", "dbmixer"])
def test_shipped_libraries_are_the_engine_defaults_emission(upd, name):
    """The build generates the shipped libraries with csim_codegen --engine-defaults and the engine loads them by
    topology hash: the library in the tree must report the full hash of exactly that emission, and that hash must not be
    the one of the generator's own defaults (another identity in a JIT cache) wherever the two emissions differ."""
    topo, src = upd.generate(name)
    topo_plain, src_plain = upd.generate(name, flags=())
    assert topo == topo_plain and len(topo) == 16
    lib = ctypes.CDLL(os.path.join(ROOT, "circuitsimulator_amd", "libcsim_sched_%s.so" % topo))
    lib.csim_sched_hash.restype = ctypes.c_ulonglong
    lib.csim_sched_topology.restype = ctypes.c_ulonglong
    assert lib.csim_sched_topology() == int(topo, 16)
    assert lib.csim_sched_hash() == _full_hash(src)
    assert _full_hash(src) != _full_hash(src_plain)
    body = lambda s: s.replace("0x%016xull" % _full_hash(s), "")
    assert body(src) != body(src_plain) or name == "buffer"     # buffer.sp: ten solve bodies carry their ballots themselves
    if name == "dbmixer":
        assert "pivot checks' ballot above ran under the reads of the MOSFET inputs" in src
        assert "pivot checks' ballot above ran under the reads of the MOSFET inputs" not in src_plain
