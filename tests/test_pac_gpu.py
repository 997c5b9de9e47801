"""Periodic AC analysis on the GPU (Engine.pac, csim_pac_batch_dev): agreement with the numpy restatement within a bound
derived per case and frequency, linear circuits against the closed form, chunking and batch independence bit for bit, the
cards' defaults, the conversion gain of the double-balanced mixer, the largest size, status and isolation, refusals.
Circuits, steps, frequencies and batches: tests/pac_cases.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pac_cases as ac
import pac_reference as par
from circuitsimulator_amd import CsimError, capi
from conftest import ROOT, has_gpu, netlist_path

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

M = ac.N_SIDE
ALL = [(n, B) for n in ac.CASES for B in ac.BATCHES]
_RUNS = {}


def _bits(v):
    a = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        return a.view(np.uint64).reshape(a.shape + (2,))
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _engine(nl):
    from circuitsimulator_amd import Engine
    eng = Engine(nl, 0)
    eng.set_kernel("general")
    return eng


def run(name, B):
    """Engine.pac of a (circuit, batch) around the RESTATEMENT's steady states, shared by the tests"""
    import torch
    if (name, B) not in _RUNS:
        nl, h, K = par.setup(name)
        p, orbits, ref = par.reference(name, B)
        eng = _engine(nl)
        params = eng.upload_params(p)
        x0 = torch.from_numpy(np.ascontiguousarray(np.stack([o["x0"] for o in orbits], axis=1))).to(params.device)
        r = eng.pac(params, x0, freqs=ac.freqs(name), n_side=M, tstep=h, f0=ac.F0)
        torch.cuda.synchronize()
        assert r["K"] == K and r["p"].shape == (len(ac.freqs(name)), 2 * M + 1, nl.n_unknowns, B)
        _RUNS[(name, B)] = dict(nl=nl, eng=eng, params=params, x0=x0, h=h, K=K, raw=r, p=r["p"].cpu().numpy(),
                                status=r["status"].cpu().numpy().astype(np.uint32), ref=ref, orbits=orbits)
    return _RUNS[(name, B)]


# ---- 1. agreement with the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", ALL)
def test_agreement_with_the_restatement(name, B):
    """Both integrate the same orbit (the start is the restatement's, the transient is bit-faithful), so only the step
    solves, the closure and their order differ: within pac_reference.agreement_bound per instance and frequency."""
    g = run(name, B)
    assert not np.any(g["status"]), sorted(set(g["status"].tolist()))
    worst = 0.0
    for b, r in enumerate(g["ref"]):
        for f in range(len(ac.freqs(name))):
            err = float(np.max(np.abs(g["p"][f, :, :, b] - r["P"][f])))
            bound = par.agreement_bound(r, f)
            worst = max(worst, err / bound)
            assert err <= bound, (name, b, f, err, bound)
    print("%s B=%d: largest |P - restatement| / bound %.3e" % (name, B, worst))


# ---- 2. linear circuits against the closed form, on the device ----------------------------------------------------------

@pytest.mark.parametrize("name", ac.LINEAR)
def test_linear_circuits_against_the_closed_form(name):
    """P_0 = (J - z Hm)^-1 u and nothing at the other sidebands; rc at f0 and 0.9 f0 is where the closure matters
    (||(I - z_K W_K)^-1|| = 200 at z_K = 1)"""
    g = run(name, 3)
    u = par.excitation(g["nl"])
    for b, r in enumerate(g["ref"]):
        for f, fr in enumerate(ac.freqs(name)):
            want = par.closed_form_linear(r["Js"][0], r["Hm"], u, r["z"][f]).astype(complex)
            err = float(np.max(np.abs(g["p"][f, M, :, b] - want)))
            bound = par.agreement_bound(r, f)
            side = float(np.max(np.abs(np.delete(g["p"][f, :, :, b], M, axis=0))))
            print("%s instance %d f %.3g: |P0 - closed form| %.3e, bound %.3e, sidebands %.3e" % (name, b, fr, err, bound, side))
            assert err <= bound
            assert side <= 1e-12 * float(np.max(np.abs(want)))


# ---- 3. chunking and batch independence, bit for bit --------------------------------------------------------------------

def test_thirty_three_frequencies_equal_one_by_one():
    """32 + 1: a full chunk and a chunk of one, against every frequency in a launch of its own"""
    import torch
    g = run("cs_rf", 3)
    f = np.linspace(0.07, 3.4, 33) * ac.F0
    every = g["eng"].pac(g["params"], g["x0"], freqs=f, n_side=M, tstep=g["h"], f0=ac.F0)
    torch.cuda.synchronize()
    assert not np.any(every["status"].cpu().numpy())
    for i in (0, 1, 16, 31, 32):
        one = g["eng"].pac(g["params"], g["x0"], freqs=f[i:i + 1], n_side=M, tstep=g["h"], f0=ac.F0)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(one["p"][0]), _bits(every["p"][i])), i
    # the frequencies of the shared run, as five of the thirty-three
    f5 = f.copy()
    f5[[2, 9, 17, 30, 32]] = ac.freqs("cs_rf")
    mixed = g["eng"].pac(g["params"], g["x0"], freqs=f5, n_side=M, tstep=g["h"], f0=ac.F0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(mixed["p"][[2, 9, 17, 30, 32]]), _bits(g["p"]))


@pytest.mark.parametrize("name", list(ac.CASES))
def test_results_do_not_depend_on_the_batch(name):
    big = run(name, 65)
    for B in (1, 3):
        small = run(name, B)
        assert np.array_equal(_bits(small["p"]), _bits(big["p"][..., :B])), (name, B)
        assert np.array_equal(small["status"], big["status"][:B])


def test_results_do_not_depend_on_the_instance_chunk():
    import torch
    g = run("cs_rf", 3)
    eng = _engine(g["nl"])
    eng.set_option("pss_chunk", 2)
    r = eng.pac(g["params"], g["x0"], freqs=ac.freqs("cs_rf"), n_side=M, tstep=g["h"], f0=ac.F0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(r["p"]), _bits(g["p"])) and not np.any(r["status"].cpu().numpy())


# ---- 4. the cards' defaults ---------------------------------------------------------------------------------------------

def test_pac_host_with_the_cards_alone_equals_pss_host_and_pac():
    """tests/golden/pac_switch_mixer.sp carries .TRAN 15.625n, .hb 1e6 3 and .PAC LIN 3 0.3e6 0.9e6 2"""
    import torch
    nl, _, K = par.setup("mixer")
    eng = _engine(nl)
    ph = np.ascontiguousarray(ac.params(nl, 3).T)
    r = eng.pac_host(params=ph)
    assert r["K"] == K and r["n_side"] == 2 and r["p"].shape == (3, 3, 5, nl.n_unknowns) and not np.any(r["status"])
    assert np.array_equal(r["freqs"], np.array([0.3e6, 0.6e6, 0.9e6]))
    s = eng.pss_host(params=ph)
    assert np.array_equal(_bits(s["x0"]), _bits(r["x0"])) and np.array_equal(s["rounds"], r["rounds"])
    params = eng.upload_params(np.ascontiguousarray(ph.T))
    x0 = torch.from_numpy(np.ascontiguousarray(s["x0"].T)).to(params.device)
    d = eng.pac(params, x0)
    torch.cuda.synchronize()
    assert d["n_side"] == 2 and np.array_equal(_bits(np.ascontiguousarray(np.moveaxis(r["p"], 0, 3))), _bits(d["p"]))
    assert np.array_equal(_bits(d["p"].cpu().numpy()[..., 0]), _bits(eng.pac_host(B=1)["p"][0]))    # nominal = instance 0
    one = eng.pac_host(params=ph, probes=[nl.node_eq("s")], n_side=1, freqs=[0.6e6])
    assert one["p"].shape == (3, 1, 3, 1)
    assert np.array_equal(_bits(one["p"][:, 0, :, 0]), _bits(r["p"][:, 1, 1:4, nl.node_eq("s")]))
    assert float(np.min(np.abs(one["p"][:, 0, 0, 0]))) > 0.05          # the switch does translate to f - f0


def test_cpp_batch_api_pac():
    """csim::BatchEngine::pac from C++ (csim_pac_demo) with the numbers of the golden netlist's cards handed over, against
    Engine.pac_host bit for bit; an empty frequency list is refused there, before the result is sized."""
    exe = os.path.join(ROOT, "circuitsimulator_amd", "csim_pac_demo")
    B = 3
    p = subprocess.run([exe, netlist_path("pac_switch_mixer.sp"), str(B)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    recs = [json.loads(ln) for ln in p.stdout.strip().splitlines()]
    assert len(recs) == B + 1 and recs[-1] == {"no_freqs_refused": True}
    nl, _, _ = par.setup("mixer")
    from circuitsimulator_amd import Engine
    want = Engine(nl, 0).pac_host(params=np.ascontiguousarray(nl.mc_params_host(12345, 0.05, 0, B).T))
    for r in recs[:B]:
        b = r["b"]
        assert (r["n_freq"], r["n_side"], r["n_probe"]) == (3, 2, nl.n_unknowns)
        assert r["rounds"] == want["rounds"][b] and r["status"] == want["status"][b] == 0
        v = np.array(r["p"])
        got = (v[:, 0] + 1j * v[:, 1]).reshape(want["p"][b].shape)
        assert np.array_equal(_bits(got), _bits(want["p"][b]))


# ---- 5. the conversion gain of the double-balanced mixer ------------------------------------------------------------------

def test_dbmixer_conversion_gain():
    """dbmixer.sp with its RF port turned into the AC excitation (pac_cases.dbmixer_variant_text), B = 3: the LO at
    900 MHz is the orbit, K = 40; an 800 MHz tone arrives at 100 MHz (sideband -1) with |P_-1| between 0.3 and 0.6 at the
    .PLOTNV nodes (the restatement gives 0.40 to 0.45 at either node, twice that between them)."""
    import torch
    from circuitsimulator_amd import Netlist
    nl = Netlist.from_text(ac.dbmixer_variant_text())
    N, K, f0, B = nl.n_unknowns, ac.DBMIXER_K, ac.DBMIXER_F0, 3
    h = 1.0 / (f0 * K)
    eng = _engine(nl)
    p = ac.params(nl, B)
    params = eng.upload_params(p)
    x_dc, _, _ = eng.dc(params)
    s = eng.pss(params, x_dc, tstep=h, f0=f0, n_harm=0)
    torch.cuda.synchronize()
    assert not np.any(s["status"].cpu().numpy()), s["status"]
    print("rounds", s["rounds"].cpu().numpy())
    out = [nl.node_eq("102"), nl.node_eq("103")]
    assert nl.probes == out
    r = eng.pac(params, s["x0"], freqs=[ac.DBMIXER_F], n_side=1, tstep=h, f0=f0, status=s["status"])
    torch.cuda.synchronize()
    assert not np.any(r["status"].cpu().numpy())
    got = r["p"].cpu().numpy()
    x0 = s["x0"].cpu().numpy()
    u = par.excitation(nl)
    gains = []
    for b in range(B):
        ref = par.pac(nl.ir_ptr, N, p, b, h, K, f0, x0[:, b], [ac.DBMIXER_F], 1, u)
        assert not np.any(ref["status"])
        bound = par.agreement_bound(ref, 0)
        err = float(np.max(np.abs(got[0, 0, :, b] - ref["P"][0, 0])))
        gains.append(float(np.max(np.abs(got[0, 0, out, b]))))
        print("instance %d: |P-1| %.4f (differential %.4f), |P - restatement| %.3e, bound %.3e"
              % (b, gains[-1], abs(got[0, 0, out[0], b] - got[0, 0, out[1], b]), err, bound))
        assert err <= bound
    assert 0.3 < max(gains) < 0.6


# ---- 6. sizes -------------------------------------------------------------------------------------------------------------

def _ladder(sections):
    """V source with an AC excitation and `sections` R-C sections: sections + 2 unknowns"""
    lines = ["* RC ladder", "V1 n0 0 AC 1 SIN 0 1 1e6 0"]
    for i in range(1, sections + 1):
        lines += ["R%d n%d n%d 100" % (i, i - 1, i), "C%d n%d 0 10p" % (i, i)]
    return "\n".join(lines) + "\n"


def test_64_unknowns_are_refused_and_63_run():
    import torch
    from circuitsimulator_amd import Engine, Netlist
    h, K = 1e-6 / 8, 8
    nl64 = Netlist.from_text(_ladder(62))
    assert nl64.n_unknowns == 64
    eng = Engine(nl64, 0)
    params = eng.upload_params(nl64.nominal_table(1))
    x, _, _ = eng.dc(params)
    with pytest.raises(CsimError) as e:
        eng.pac(params, x, freqs=[0.4e6], n_side=1, tstep=h, f0=1e6)
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
    # 63 unknowns: the largest size, the one whose workgroup needs more than 64 KB of LDS
    nl = Netlist.from_text(_ladder(61))
    assert nl.n_unknowns == 63
    eng = _engine(nl)
    p = np.ascontiguousarray(nl.mc_params_host(5, 0.03, 0, 2))
    params = eng.upload_params(p)
    fr = np.array([0.4e6, 1e6, 2.5e6])
    x0 = np.zeros((63, 2))                                      # linear: the analysis does not depend on the orbit
    r = eng.pac(params, torch.from_numpy(x0).to(params.device), freqs=fr, n_side=1, tstep=h, f0=1e6)
    torch.cuda.synchronize()
    assert not np.any(r["status"].cpu().numpy())
    got = r["p"].cpu().numpy()
    ref = par.pac(nl.ir_ptr, 63, p, 1, h, K, 1e6, x0[:, 1], fr, 1, par.excitation(nl))
    for f in range(len(fr)):
        err, bound = float(np.max(np.abs(got[f, :, :, 1] - ref["P"][f]))), par.agreement_bound(ref, f)
        print("63 unknowns f %.3g: |P - restatement| %.3e, bound %.3e" % (fr[f], err, bound))
        assert err <= bound
    assert float(np.max(np.abs(got[:, 1, 0, 1] - 1.0))) < 1e-12     # the driven node follows the source


# ---- 7. status and isolation ------------------------------------------------------------------------------------------------

def test_a_singular_closure_stops_its_instance_only():
    """A capacitor of 1e12 F holds its node for good: W_K(out, out) rounds to exactly 1 and I - z_K W_K is singular at
    z_K = 1 (f = f0).  That instance gets CSIM_ST_PAC_SINGULAR and zeros for the whole chunk of frequencies, its
    neighbours are untouched; in a chunk without f0 it runs like any other."""
    import torch
    g = run("rc", 3)
    nl, eng = g["nl"], g["eng"]
    p = ac.params(nl, 3).copy()
    slot = int(np.argmin(np.abs(nl.nominal_params / 200e-9 - 1.0)))
    assert abs(nl.nominal_params[slot] / 200e-9 - 1.0) < 1e-12
    p[slot, 1] = 1e12
    params = eng.upload_params(p)
    fr = np.array([0.5 * ac.F0, ac.F0])
    r = eng.pac(params, g["x0"], freqs=fr, n_side=1, tstep=g["h"], f0=ac.F0)
    torch.cuda.synchronize()
    st, got = r["status"].cpu().numpy().astype(np.uint32), r["p"].cpu().numpy()
    assert st[1] & capi.ST_PAC_SINGULAR and not np.any(got[..., 1]) and st[0] == 0 and st[2] == 0
    ref = par.pac(nl.ir_ptr, nl.n_unknowns, p, 1, g["h"], g["K"], ac.F0, g["x0"].cpu().numpy()[:, 1], fr, 1, par.excitation(nl))
    assert list(ref["status"]) == [0, par.ST_PAC_SINGULAR]
    clean = eng.pac(g["params"], g["x0"], freqs=fr, n_side=1, tstep=g["h"], f0=ac.F0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got[..., [0, 2]]), _bits(clean["p"].cpu().numpy()[..., [0, 2]]))
    half = eng.pac(params, g["x0"], freqs=fr[:1], n_side=1, tstep=g["h"], f0=ac.F0)
    torch.cuda.synchronize()
    assert not np.any(half["status"].cpu().numpy()) and np.all(np.abs(half["p"].cpu().numpy()[0, 1, nl.node_eq("in"), :] - 1.0) < 1e-12)


def test_a_start_that_is_not_finite_stops_its_instance_only():
    import torch
    g = run("cs_rf", 3)
    x = g["x0"].clone()
    x[2, 1] = float("nan")
    r = g["eng"].pac(g["params"], x, freqs=ac.freqs("cs_rf"), n_side=M, tstep=g["h"], f0=ac.F0)
    torch.cuda.synchronize()
    st, got = r["status"].cpu().numpy().astype(np.uint32), r["p"].cpu().numpy()
    assert st[1] & capi.ST_TRAN_NONFINITE and not np.any(got[..., 1]) and st[0] == 0 and st[2] == 0
    assert np.array_equal(_bits(got[..., [0, 2]]), _bits(g["p"][..., [0, 2]]))
    assert np.isnan(x[2, 1].item()) and np.array_equal(_bits(x[:, [0, 2]]), _bits(g["x0"][:, [0, 2]]))   # x0 is not written
    # an instance the steady state gave up arrives flagged: zeros, no new bit
    flagged = torch.zeros(3, dtype=torch.int32, device=x.device)
    flagged[2] = capi.ST_PSS_SINGULAR
    r = g["eng"].pac(g["params"], g["x0"], freqs=ac.freqs("cs_rf"), n_side=M, tstep=g["h"], f0=ac.F0, status=flagged)
    torch.cuda.synchronize()
    assert r["status"].cpu().numpy().tolist() == [0, 0, capi.ST_PSS_SINGULAR] and not np.any(r["p"].cpu().numpy()[..., 2])
    assert np.array_equal(_bits(r["p"].cpu().numpy()[..., :2]), _bits(g["p"][..., :2]))


def test_two_engines_on_two_streams_do_not_share_state():
    import torch
    want = {n: run(n, 3) for n in ("cs_rf", "rlc")}
    engs = {n: _engine(want[n]["nl"]) for n in want}
    streams = {n: torch.cuda.Stream() for n in want}
    got = {n: [] for n in want}
    for _ in range(2):
        for n in ("cs_rf", "rlc", "cs_rf"):
            g = want[n]
            with torch.cuda.stream(streams[n]):
                got[n].append(engs[n].pac(g["params"], g["x0"], freqs=ac.freqs(n), n_side=M, tstep=g["h"], f0=ac.F0))
    torch.cuda.synchronize()
    for n, rs in got.items():
        for r in rs:
            assert np.array_equal(_bits(r["p"]), _bits(want[n]["p"])), n


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_with_an_engine():
    import torch
    g = run("rc", 3)
    eng, nl = g["eng"], g["nl"]
    L = capi.lib()
    N = nl.n_unknowns
    fr = np.array([0.5e6, 1e6])
    out = torch.zeros((2, 31, N, 3, 2), dtype=torch.float64, device=g["x0"].device)     # room for the largest n_side below, 15
    st = torch.zeros(3, dtype=torch.int32, device=g["x0"].device)
    ok = dict(eng=eng._h, params=g["params"].data_ptr(), B=3, tstep=g["h"], f0=1e6, x0=g["x0"].data_ptr(), freqs=fr.ctypes.data,
              F=2, n_side=1, probe=None, n_probe=0, out=out.data_ptr(), status=st.data_ptr(), stream=None)

    def call(**ch):
        a = dict(ok, **ch)
        return L.csim_pac_batch_dev(*[a[k] for k in ok])
    ARG, CONFIG = capi.CSIM_ERR_ARG, capi.CSIM_ERR_CONFIG
    assert call() == capi.CSIM_OK
    for k in ("eng", "params", "x0", "freqs", "out", "status"):
        assert call(**{k: None}) == ARG, k
    assert call(B=0) == ARG and call(B=-1) == ARG and call(F=0) == ARG and call(F=-1) == ARG and call(n_side=-1) == ARG
    for bad in (float("nan"), float("inf")):
        assert call(tstep=bad) == ARG and call(f0=bad) == ARG
    for bad in (float("nan"), float("inf"), 0.0, -1e6):
        assert call(freqs=np.array([0.5e6, bad]).ctypes.data) == ARG, bad
    assert call(probe=(C.c_int32 * 1)(N), n_probe=1) == ARG and call(probe=(C.c_int32 * 1)(-1), n_probe=1) == ARG
    assert call(f0=0.0) == CONFIG and call(tstep=0.0) == CONFIG          # the device form has no cards to fall back on
    assert call(tstep=g["h"] * 1.001) == CONFIG                          # |K h f0 - 1| > 1e-9
    assert call(n_side=16) == CONFIG                                     # K = 32 < 2 * 16 + 1
    assert call(n_side=15) == capi.CSIM_OK
    assert call(tstep=1e-6 / (1 << 23)) == CONFIG                        # K > 2^22
    assert call(n_side=-1, f0=0.0) == ARG                                # the argument error comes first
    # no source with an AC magnitude
    import pss_cases as pc
    from circuitsimulator_amd import Engine
    plain = Engine(pc.netlist("rc"), 0)
    assert L.csim_pac_batch_dev(*[dict(ok, eng=plain._h)[k] for k in ok]) == CONFIG
    pp = plain.upload_params(pc.params(pc.netlist("rc"), 3))
    xx = torch.zeros((pc.netlist("rc").n_unknowns, 3), dtype=torch.float64, device=pp.device)
    with pytest.raises(CsimError) as e:
        plain.pac(pp, xx, freqs=fr, n_side=1)
    assert e.value.code == CONFIG and "AC" in str(e.value)
    # the host form: the cards fill in, a netlist without them is refused
    bare = Engine(ac.netlist("divider"), 0)
    for kw in (dict(freqs=fr), dict(freqs=fr, f0=1e6)):                  # no .HB card; no .TRAN card
        with pytest.raises(CsimError) as e:
            bare.pac_host(**kw)
        assert e.value.code == CONFIG
    with pytest.raises(CsimError) as e:                                  # no frequencies and no .PAC card
        bare.pac_host(tstep=1e-6 / 16, f0=1e6)
    assert e.value.code == ARG
    ob = np.zeros((1, 2, 3, 5), dtype=complex)
    h16 = 1e-6 / 16
    assert L.csim_pac_batch(bare._h, None, 1, 0.0, 0.0, fr.ctypes.data, 2, 1, None, 0, ob.ctypes.data, None, None, None) == CONFIG
    assert L.csim_pac_batch(bare._h, None, 1, h16, 1e6, None, 0, 1, None, 0, ob.ctypes.data, None, None, None) == ARG
    assert L.csim_pac_batch(bare._h, None, 1, h16, 1e6, fr.ctypes.data, 2, 1, None, 0, None, None, None, None) == ARG
    assert L.csim_pac_batch(bare._h, None, 0, h16, 1e6, fr.ctypes.data, 2, 1, None, 0, ob.ctypes.data, None, None, None) == ARG
    assert L.csim_pac_batch(bare._h, None, 1, h16, 1e6, fr.ctypes.data, 2, 1, None, 0, ob.ctypes.data, None, None, None) == capi.CSIM_OK
    assert abs(ob[0, 0, 1, 1] - 1.0) < 1e-12                             # the divider's input node follows the source
