"""S-parameter analysis through the engine: Engine.sp against tests/sp_reference.py fed with the engine's own
(G, C), the two kernels against each other, Y against Engine.ac with the excitation moved from port to port,
chunking, stream order, the optional S, the card, errors, and a frequency at which the circuit is singular."""
import numpy as np
import pytest

import sp_reference as spref
from conftest import has_gpu, netlist_path

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

PI = 3.14159265358979323846
FREQS = np.array([1e3, 1e6, 3.3e7, 1e9, 1e10])
DBMIXER_PORTS = (("Vrf1+ 112 212 SIN 0.6 0.01 800e6 180", 1), ("Vrf1- 113 213 SIN 0.6  0.01 800e6 0", 2))


def _text(name):
    text = open(netlist_path(name)).read()
    if name == "dbmixer.sp":
        for line, k in DBMIXER_PORTS:
            assert line in text
            text = text.replace(line, line + " PORTNUM %d Z0 25" % k, 1)
    return text


def _nl(name=None, text=None):
    from circuitsimulator_amd import Netlist
    return Netlist.from_text(text if text is not None else _text(name))


def _u64(t):
    a = np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t), dtype=np.complex128)
    return a.view(np.uint64).reshape(a.shape + (2,))


def _systems(eng, nl, params, x):
    """Engine.ac_system -> G, C [B][n][n] row-major, numpy"""
    import torch
    G, C, _ = eng.ac_system(params, x)
    torch.cuda.synchronize()
    return np.ascontiguousarray(G.cpu().numpy()), np.ascontiguousarray(C.cpu().numpy())


NAMES = ("sp_resistor.sp", "sp_pi_pad.sp", "sp_rlc_twoport.sp", "sp_cs_amp.sp", "dbmixer.sp")


@pytest.mark.parametrize("name", NAMES)
def test_engine_equals_reference_and_kernels_agree(name):
    """B = 8 Monte-Carlo instances, 5 frequencies: Y and S equal the reference fed with the engine's (G, C) bit for
    bit, with either kernel"""
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl(name)
    ports = nl.ports
    pe, z0 = [p[1] for p in ports], [p[2] for p in ports]
    B, P = 8, len(ports)
    res = {}
    for kernel in ("wave", "packed"):
        eng = Engine(nl, 0)
        eng.set_option("ac_kernel", kernel)
        params = eng.mc_params(12345, 0.05, 0, B)
        x, _, _ = eng.dc(params)
        r = eng.sp(params, x, freqs=FREQS)
        torch.cuda.synchronize()
        assert tuple(r["y"].shape) == (len(FREQS), P, P, B) and tuple(r["s"].shape) == (len(FREQS), P, P, B)
        assert not r["status"].cpu().numpy().any()
        res[kernel] = (_u64(r["y"]), _u64(r["s"]))
        if kernel == "wave":
            G, C = _systems(eng, nl, params, x)
            omega = 2.0 * PI * FREQS
            for b in range(B):
                ref = spref.sweep_ports(G[b], C[b], omega, pe, z0)
                assert ref["per_f"] == [0] * len(FREQS)
                assert np.array_equal(_u64(ref["y"]), res[kernel][0][:, :, :, b]), (name, b, "y")
                assert np.array_equal(_u64(ref["s"]), res[kernel][1][:, :, :, b]), (name, b, "s")
    assert np.array_equal(res["wave"][0], res["packed"][0]) and np.array_equal(res["wave"][1], res["packed"][1])
    if name == "sp_cs_amp.sp":                                  # non-reciprocal: the stage has gain one way only
        y = res["wave"][0].view(np.float64)
        assert not np.array_equal(y[:, 0, 1], y[:, 1, 0])
    if name == "sp_resistor.sp":                                # the sign: a resistor gives Y11 = +(1/R + gmin)
        y11 = r["y"].cpu().numpy()[:, 0, 0, :]
        Rv = params.cpu().numpy()[list(nl.nominal_params).index(75.0)]
        assert np.array_equal(y11.real, np.broadcast_to(1.0 / Rv + 1e-6, y11.shape)) and np.all(y11.imag == 0)


@pytest.mark.parametrize("name", NAMES)
def test_y_columns_equal_ac_sweeps(name):
    """column j of Y equals, bit for bit with the sign flipped, Engine.ac on the same text with AC 1 on port j only,
    probed at the branch equations"""
    import re
    import torch
    from circuitsimulator_amd import Engine
    text = _text(name)
    nl = _nl(text=text)
    ports = nl.ports
    pe = [p[1] for p in ports]
    B = 8
    eng = Engine(nl, 0)
    params = eng.mc_params(99, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    y = eng.sp(params, x, freqs=FREQS, want_s=False)
    torch.cuda.synchronize()
    assert y["s"] is None
    yv = y["y"].cpu().numpy()
    plain = re.sub(r"(?i) AC\s+\S+(?= )", "", text)             # no AC magnitude anywhere
    for j in range(len(ports)):
        lines = plain.splitlines()
        hit = [i for i, ln in enumerate(lines) if re.search(r"(?i)portnum\s+%d\b" % (j + 1), ln)]
        assert len(hit) == 1
        tok = lines[hit[0]].split()
        at = [t.lower() for t in tok].index("portnum")
        lines[hit[0]] = " ".join(tok[:at] + ["AC", "1"] + tok[at:]) if "sin" not in [t.lower() for t in tok] else \
            " ".join(tok[:3] + ["AC", "1"] + tok[3:])
        nj = _nl(text="\n".join(lines) + "\n")
        assert nj.ports == ports and nj.ac_source(ports[j][0]) == (1.0, 0.0)
        ej = Engine(nj, 0)
        out, st = ej.ac(params, x, freqs=FREQS, probes=pe)
        torch.cuda.synchronize()
        a = out.cpu().numpy()                                   # [F][P][B]
        assert np.array_equal(_u64(-a), _u64(yv[:, :, j, :])), (name, j)


def test_batch_of_64_in_halves_and_across_a_chunk_boundary():
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl("dbmixer.sp")
    eng = Engine(nl, 0)
    chunk = eng.stat("ac_chunk")                                # the engine's own figure, not a restatement of it
    assert 256 <= chunk < 100000
    B = chunk + 33                                              # a second, odd chunk at b0 = chunk > 0
    params = eng.mc_params(4242, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    f = FREQS[1:3]
    full = eng.sp(params, x, freqs=f)
    torch.cuda.synchronize()
    fy, fs, fst = _u64(full["y"]), _u64(full["s"]), full["status"].cpu().numpy()
    pick = list(range(31)) + [chunk - 1, chunk, chunk + 1] + list(range(B - 30, B))
    assert len(pick) == 64
    idx = torch.tensor(pick, device=params.device)
    p64, x64 = params[:, idx].contiguous(), x[:, idx].contiguous()
    r64 = eng.sp(p64, x64, freqs=f)
    assert np.array_equal(_u64(r64["y"]), fy[:, :, :, pick]) and np.array_equal(_u64(r64["s"]), fs[:, :, :, pick])
    assert np.array_equal(r64["status"].cpu().numpy(), fst[pick])
    halves = [eng.sp(p64[:, a:b].contiguous(), x64[:, a:b].contiguous(), freqs=f) for a, b in ((0, 32), (32, 64))]
    for key, want in (("y", fy), ("s", fs)):
        assert np.array_equal(np.concatenate([_u64(h[key]) for h in halves], axis=3), want[:, :, :, pick]), key


def test_two_sweeps_back_to_back_on_a_stream():
    """csim_sp_batch_dev enqueues and never waits: two sweeps with different frequency lists on one stream with no
    synchronisation between them equal their solo runs"""
    import math
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl("dbmixer.sp")
    eng = Engine(nl, 0)
    B = 2048
    params = eng.mc_params(2024, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    f1 = np.array([1e3 * math.pow(10.0, k / 5) for k in range(36)])
    f2 = f1[::-1] * 3.0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a1 = eng.sp(params, x, freqs=f1)
        a2 = eng.sp(params, x, freqs=f2)
        s.synchronize()
        r1 = eng.sp(params, x, freqs=f1)
        s.synchronize()
        r2 = eng.sp(params, x, freqs=f2)
        s.synchronize()
    torch.cuda.synchronize()
    for key in ("y", "s"):
        assert np.array_equal(_u64(a1[key]), _u64(r1[key])) and np.array_equal(_u64(a2[key]), _u64(r2[key])), key
    assert not np.array_equal(_u64(r1["y"]), _u64(r2["y"]))


def test_card_defaults_and_host_layout():
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl("sp_rlc_twoport.sp")
    eng = Engine(nl, 0)
    B = 3
    params = eng.mc_params(5, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    r = eng.sp(params, x)
    torch.cuda.synchronize()
    assert np.array_equal(r["freqs"], nl.sp_freqs()) and len(r["freqs"]) == 9
    h = eng.sp_host(params.cpu().numpy().T.copy())
    assert h["y"].shape == (B, 9, 2, 2) and not h["status"].any()
    assert np.array_equal(_u64(h["y"]), _u64(r["y"].cpu().numpy().transpose(3, 0, 1, 2)))
    assert np.array_equal(_u64(h["s"]), _u64(r["s"].cpu().numpy().transpose(3, 0, 1, 2)))
    assert eng.sp_host(B=2, want_s=False)["s"] is None


def test_errors():
    from circuitsimulator_amd import CsimError, Engine, capi
    # no ports
    eng = Engine(_nl(text=open(netlist_path("ac_rc_lowpass.sp")).read()), 0)
    with pytest.raises(CsimError) as e:
        eng.sp_host(freqs=[1e3])
    assert e.value.code == capi.CSIM_ERR_CONFIG
    # ports but no card and no frequencies
    eng = Engine(_nl(text="* r\nV1 a 0 DC 0 PORTNUM 1\nR1 a 0 50\n"), 0)
    with pytest.raises(CsimError) as e:
        eng.sp_host()
    assert e.value.code == capi.CSIM_ERR_CONFIG
    assert eng.sp_host(freqs=[1e3])["y"].shape == (1, 1, 1, 1)

    def ladder(N):                                              # N unknowns: N - 2 sections, n0 and the branch current
        lines = ["* ladder", "V1 n0 0 DC 0 PORTNUM 1"]
        for k in range(1, N - 1):
            lines += ["R%d n%d n%d 10" % (k, k - 1, k), "C%d n%d 0 1p" % (k, k)]
        return "\n".join(lines) + "\n"
    nl = _nl(text=ladder(64))
    assert nl.n_unknowns == 64
    with pytest.raises(CsimError) as e:
        Engine(nl, 0).sp_host(freqs=[1e3])
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
    nl = _nl(text=ladder(33))
    assert nl.n_unknowns == 33
    eng = Engine(nl, 0)
    assert eng.sp_host(freqs=[1e6])["y"].shape == (1, 1, 1, 1)
    eng.set_option("ac_kernel", "packed")
    with pytest.raises(CsimError) as e:
        eng.sp_host(freqs=[1e6])
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED


def test_singular_at_dc_only():
    """an inductor loop: a V source across an inductor is singular at w = 0 (two branch equations say the same) and
    regular elsewhere -- zeros at that frequency only, the flag set, the other frequencies the reference's"""
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl(text="* loop\nV1 a 0 DC 0 PORTNUM 1\nL1 a 0 1u\nR1 a 0 1k\n")
    eng = Engine(nl, 0)
    params = eng.upload_params(nl.nominal_table(2))
    x, _, _ = eng.dc(params)
    f = np.array([1e6, 0.0, 2e6])
    r = eng.sp(params, x, freqs=f)
    torch.cuda.synchronize()
    y, s = r["y"].cpu().numpy(), r["s"].cpu().numpy()
    assert r["status"].cpu().numpy().tolist() == [4, 4]
    assert np.all(y[1] == 0) and np.all(s[1] == 0) and np.all(y[0] != 0) and np.all(y[2] != 0) and np.all(s[0] != 0)
    G, C = _systems(eng, nl, params, x)
    ref = spref.sweep_ports(G[0], C[0], 2.0 * PI * f, [nl.ports[0][1]], [50.0])
    assert ref["per_f"] == [0, 4, 0]
    assert np.array_equal(_u64(ref["y"]), _u64(y)[:, :, :, 0]) and np.array_equal(_u64(ref["s"]), _u64(s)[:, :, :, 0])
