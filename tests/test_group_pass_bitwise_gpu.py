"""The group kernels' Newton pass as the shipped libraries and the engine's JIT generate it (codegen.hpp
GeneratorOptions::engineDefaults: cover_mos=2) against the emission with the generator options wait_at_use and cover_mos off.  The options move
waits and bookkeeping only: every floating-point operation keeps its operands and its order, so the two
emissions must agree bit for bit -- state, per-instance NR totals, per-step NR counts, status -- for
sixteen and for four lanes per instance (test_group_pass_isa_cpu.py looks at wait_at_use, which is off by default, in
the ISA).  The shapes are the smallest at which the change can go wrong: a partial wave,
a batch that is no multiple of the 4 / 16 instances per wave, several waves, a second launch (the pipelined MOSFET
prologue runs on the first step of a launch only), a circuit with several solve bodies over the same staging rows,
PULSE / PWL per-step source phases, and the hand-over of a group whose pivot checks fail."""
import ctypes as C
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import has_gpu, netlist_path

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

OLD = "wait_at_use=0,cover_mos=0"        # the emission before these options existed
FALLBACK = 0x20


def _have_hipcc():
    return bool(shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"))


def _pair(text_or_path, jit_dir, plan=None, jit_dir_old=None):
    """-> (netlist, engine with the default emission, engine with the options off), same schedules in both.
    plan = (params seed, steps): a circuit without a shipped library is specialised from its first steps.
    jit_dir_old: a JIT directory of its own for the second engine's library."""
    from circuitsimulator_amd import Engine, Netlist
    if not _have_hipcc():
        pytest.skip("hipcc not available for the JIT")
    nl = Netlist.from_file(text_or_path) if os.path.exists(text_or_path) else Netlist.from_text(text_or_path)
    new, old = Engine(nl, 0), Engine(nl, 0)
    new.set_option("jit_dir", jit_dir)
    old.set_option("jit_dir", jit_dir_old or jit_dir)
    if plan is not None:
        assert new.tran_kernel == "general"
        new.jit_scheduled(new.mc_params(plan[0], 0.05, 0, 8), plan_steps=plan[1])
    assert new.tran_kernel == "scheduled"
    sched, dc_sched = new.loaded_schedules()
    old.set_option("jit_gen_opts", OLD)
    old.jit_with_schedules(sched, dc_sched)
    assert old.tran_kernel == "scheduled" and old.loaded_schedules() == (sched, dc_sched)
    return nl, new, old


@pytest.fixture(scope="module")
def jit_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("jit"))


@pytest.fixture(scope="module")
def dbmixer(jit_dir):
    return _pair(netlist_path("dbmixer.sp"), jit_dir)


@pytest.fixture(scope="module")
def buffer(jit_dir):
    return _pair(netlist_path("buffer.sp"), jit_dir)


@pytest.fixture(scope="module")
def pulse_pwl(jit_dir):
    return _pair(netlist_path("pulse_pwl.sp"), jit_dir, plan=(3, 20))


def _run(eng, nl, lanes, B, calls, seed=12345):
    """DC, then one tran() per (step_first, n_steps) on the same buffers -> the bits of everything a caller sees"""
    import torch
    eng.set_option("lanes_per_instance", lanes)
    assert eng.lanes_for_batch(B) == lanes
    params = eng.mc_params(seed, 0.05, 0, B)
    x, _, st = eng.dc(params)
    iters = torch.zeros(B, dtype=torch.int64, device=x.device)
    total = sum(n for _, n in calls)
    si = torch.full((total, B), -1, dtype=torch.int32, device=x.device)
    row = 0
    for first, n in calls:
        eng.tran(params, x, nl.tstep, first, n, iters, st, step_iters=si[row:row + n])
        row += n
    torch.cuda.synchronize()
    eng.set_option("lanes_per_instance", 0)
    return dict(x=x.cpu().numpy(), iters=iters.cpu().numpy(), status=st.cpu().numpy(), step_iters=si.cpu().numpy())


def _same_bits(a, b):
    for k in ("x", "iters", "step_iters", "status"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k                 # == on the bits: -0.0 and NaN payloads count too
    assert (a["step_iters"] > 0).all()                             # every step was run and counted


@pytest.mark.parametrize("lanes", [16, 4])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_dbmixer_two_launches(dbmixer, lanes, B):
    nl, new, old = dbmixer
    calls = [(0, 3), (3, 2)]
    _same_bits(_run(new, nl, lanes, B, calls), _run(old, nl, lanes, B, calls))


@pytest.mark.parametrize("lanes", [16, 4])
def test_buffer_alternative_bodies(buffer, lanes):
    nl, new, old = buffer
    assert len(new.loaded_schedules()[0]) == 10
    a, b = _run(new, nl, lanes, 5, [(0, 40)]), _run(old, nl, lanes, 5, [(0, 40)])
    _same_bits(a, b)


@pytest.mark.parametrize("lanes", [16, 4])
def test_pulse_pwl_source_phase(pulse_pwl, lanes):
    nl, new, old = pulse_pwl
    _same_bits(_run(new, nl, lanes, 5, [(0, 20)]), _run(old, nl, lanes, 5, [(0, 20)]))


class _Aux(C.Structure):       # csim_sched_aux (engine_internal.hpp)
    _fields_ = [("fallback", C.c_void_p), ("done", C.c_void_p), ("flags", C.c_void_p), ("work", C.c_void_p),
                ("nearX", C.c_void_p), ("nearStep", C.c_void_p), ("nearIt", C.c_void_p), ("nearItAfter", C.c_void_p)]


def _launch_group(lib_path, variant, params, x0, st0, tstep, n_steps):
    """One launch of a generated library's group kernel on buffers of this test: -> what the kernel hands the engine"""
    import torch
    lib = C.CDLL(lib_path)
    fn = lib.csim_sched_launch
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int, C.c_int,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_Aux), C.c_void_p, C.c_int]
    dev = params.device
    N, B = x0.shape
    x, st = x0.clone(), st0.clone()
    iters = torch.zeros(B, dtype=torch.int64, device=dev)
    si = torch.full((n_steps, B), -1, dtype=torch.int32, device=dev)
    fallback = torch.zeros(B, dtype=torch.uint8, device=dev)
    done = torch.zeros(B, dtype=torch.int32, device=dev)
    flags = torch.zeros(8, dtype=torch.int32, device=dev)
    near_x = torch.zeros((N, B), dtype=torch.float64, device=dev)
    near_step = torch.zeros(B, dtype=torch.int32, device=dev)
    near_it = torch.zeros(B, dtype=torch.int32, device=dev)
    near_after = torch.zeros(B, dtype=torch.int64, device=dev)
    aux = _Aux(fallback.data_ptr(), done.data_ptr(), flags.data_ptr(), None, near_x.data_ptr(), near_step.data_ptr(),
               near_it.data_ptr(), near_after.data_ptr())
    torch.cuda.synchronize()
    rc = fn(params.data_ptr(), B, float(tstep), 0, n_steps, None, 0, 1, None, x.data_ptr(), iters.data_ptr(),
            st.data_ptr(), si.data_ptr(), C.byref(aux), None, variant)
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(x=x, status=st, iters=iters, step_iters=si, fallback=fallback, done=done,
                                                 flags=flags[:2]).items()}


@pytest.fixture(scope="module")
def handover(tmp_path_factory):
    """The schedule-violating construction: a kernel specialised from the quiet start of a switching circuit (buffer.sp
    with one more element, so that no shipped library fits) -- three steps show it one pivot sequence only."""
    d_new, d_old = str(tmp_path_factory.mktemp("jit_handover_new")), str(tmp_path_factory.mktemp("jit_handover_old"))
    text = open(netlist_path("buffer.sp")).read().replace("Rin 101 102 10", "Rin 101 102 11")
    nl, new, old = _pair(text + "\nRextra 118 0 1e9\n", d_new, plan=(5, 3), jit_dir_old=d_old)
    libs = [glob.glob(os.path.join(d, "libcsim_sched_*.so")) for d in (d_new, d_old)]
    assert [len(l) for l in libs] == [1, 1]                        # each engine built one library, in its own directory
    libs = [l[0] for l in libs]
    assert os.path.basename(libs[0]) != os.path.basename(libs[1])  # two identities: the emissions differ
    return nl, new, old, libs


@pytest.mark.parametrize("lanes", [16, 4])
def test_hand_over_progress(handover, lanes):
    """The running circuit meets factorisations that none of the kernel's schedules fits: the group's pivot checks
    fail, and the kernel stops the instance at the start of that step.  Both emissions must stop every instance at the
    same step (done), flag the same instances, and hand over the same state -- this is where the pivot checks' ballot,
    which cover_mos moves, decides."""
    nl, new, old, libs = handover
    B, steps = 5, 300
    params = new.mc_params(5, 0.05, 0, B)
    x0, _, st0 = new.dc(params)
    a = _launch_group(libs[0], lanes, params, x0, st0, nl.tstep, steps)
    b = _launch_group(libs[1], lanes, params, x0, st0, nl.tstep, steps)
    assert (a["done"] < steps).any() and a["fallback"].any() and a["flags"][0] == 1       # the hand-over really happened
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    # and through the engine's ladder the two emissions end in the same bits
    ra, rb = _run(new, nl, lanes, B, [(0, steps)], seed=5), _run(old, nl, lanes, B, [(0, steps)], seed=5)
    _same_bits(ra, rb)
    assert (ra["status"] & FALLBACK).any()
