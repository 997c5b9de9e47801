"""Noise analysis on the GPU through the engine: Engine.noise against tests/noise_reference.py fed with the engine's
own linearised systems and PSDs (bit for bit), the PSDs against their definition, batch independence (halves, the
system-scratch chunk boundary, the two kernels), stream order, the .NOISE card's defaults and the error paths."""
import ctypes as C
import math

import numpy as np
import pytest

import noise_reference as nref
from conftest import has_gpu, netlist_path

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

PI = 3.14159265358979323846
TEMP = 300.15
B = 64

# netlist, output, input source, frequencies (None: the card's)
CIRCUITS = {
    "noise_divider.sp": (None, None, None),
    "noise_rc_lowpass.sp": (None, None, None),
    "noise_cs_amp.sp": (None, None, None),
    "ac_cs_amp.sp": (("d", None), "VIN", [1e3, 1e6, 1e9]),
    "buffer.sp": (("118", None), "Vin", [1e3, 1e7, 1e9]),
    "dbmixer.sp": (("102", "103"), "Vrf1+", [1e5, 1e8, 1e10]),
}


class _IR(C.Structure):
    _fields_ = [("n_unknowns", C.c_int32), ("n_node_eq", C.c_int32), ("n_branch_eq", C.c_int32),
                ("n_elems", C.c_int32), ("n_params", C.c_int32), ("has_nonlinear", C.c_int32),
                ("kind", C.POINTER(C.c_int32)), ("eq", C.POINTER(C.c_int32)), ("branch_eq", C.POINTER(C.c_int32)),
                ("param_slot", C.POINTER(C.c_int32))]


def _records(nl):
    ir = C.cast(nl.ir_ptr, C.POINTER(_IR)).contents
    return [(ir.kind[e], [ir.eq[4 * e + t] for t in range(4)], ir.branch_eq[e], ir.param_slot[e])
            for e in range(ir.n_elems)]


def _elem_index(name, elem_name):
    """element index of a device line by its name, from the netlist text"""
    elem = 0
    for line in open(netlist_path(name)).read().splitlines():
        line = line.split("$")[0].strip()
        if not line or line[0] in "*;.+" or line[0].upper() not in "RCLVIM":
            continue
        if line.split()[0].lower() == elem_name.lower():
            return elem
        elem += 1
    raise KeyError(elem_name)


def _setup(name):
    """-> (netlist, engine, (out_p, out_m), src_elem, freqs) with the card's values where CIRCUITS names none"""
    from circuitsimulator_amd import Engine, Netlist
    nl = Netlist.from_file(netlist_path(name))
    out, src_name, freqs = CIRCUITS[name]
    if out is None:
        card = nl.noise
        out_pm, src, f = (card[0], card[1]), card[2], nl.noise_freqs()[::7]
    else:
        out_pm = (nl.node_eq(out[0]), -1 if out[1] is None else nl.node_eq(out[1]))
        src, f = _elem_index(name, src_name), np.array(freqs)
    assert out_pm[0] >= 0 and src >= 0
    return nl, Engine(nl, 0), out_pm, src, f


def _gain_in(nl, src):
    kind, q, k, _ = _records(nl)[src]
    return ("v", k) if kind == 3 else ("i", q[1], q[0])


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _u64(t):
    a = np.ascontiguousarray(_np(t))
    return a.view(np.uint64)


def _bits_of(res):
    """every output of Engine.noise as bit patterns, instance on the last axis"""
    return {k: _u64(res[k]) if k != "gain" else _u64(res[k]).reshape(_np(res[k]).shape + (2,)).transpose(0, 2, 1)
            for k in ("onoise", "gain", "contrib", "psd") if res[k] is not None}


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_engine_equals_reference_bitwise(name):
    """Engine.noise == noise_reference fed with the engine's ac_system() and its exported PSDs, for every instance of
    a Monte-Carlo table and both kernels"""
    import torch
    nl, eng, out, src, f = _setup(name)
    N = nl.n_unknowns
    params = eng.mc_params(12345, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    G, Cm, _ = eng.ac_system(params, x)
    gens = nl.noise_sources
    a = np.array([g[1] for g in gens], dtype=np.int32)
    b = np.array([g[2] for g in gens], dtype=np.int32)
    omega = 2.0 * PI * f
    gin = _gain_in(nl, src)
    results = {}
    for kernel in (("wave", "packed") if N <= 32 else ("wave",)):
        eng.set_option("ac_kernel", kernel)
        r = eng.noise(params, x, freqs=f, out=out, src=src, temp=TEMP, contrib=True, psd=True)
        torch.cuda.synchronize()
        results[kernel] = r
    eng.set_option("ac_kernel", "auto")
    r = results["wave"]
    Gh, Ch, psd = _np(G), _np(Cm), _np(r["psd"])
    on, con, gain, st = _np(r["onoise"]), _np(r["contrib"]), _np(r["gain"]), _np(r["status"])
    assert on.shape == (len(f), B) and con.shape == (len(f), len(gens), B) and gain.shape == (len(f), B)
    assert np.all(st == 0)
    assert np.all(on > 0) and np.all(np.isfinite(on)) and np.all(np.isfinite(gain))
    for i in range(B):
        ref = nref.solve_sweep(Gh[i], Ch[i], omega, out, a, b, psd[:, i], gin, eps=1e-15)
        assert ref["flags"] == 0
        assert np.array_equal(_u64(on[:, i]), _u64(ref["onoise"])), (name, i)
        assert np.array_equal(_u64(con[:, :, i]), _u64(ref["contrib"])), (name, i)
        assert np.array_equal(_u64(gain[:, i]), _u64(ref["gain"])), (name, i)
    if "packed" in results:
        bw, bp = _bits_of(results["wave"]), _bits_of(results["packed"])
        for k in bw:
            assert np.array_equal(bw[k], bp[k]), (name, k)
    print("%s: N = %d, S = %d, F = %d, B = %d; onoise %.3e .. %.3e V^2/Hz, |gain| %.3e .. %.3e"
          % (name, N, len(gens), len(f), B, on.min(), on.max(), np.abs(gain).min(), np.abs(gain).max()))


def _mos_gg(isP, Vth, K, lam, Vd, Vg, Vs):
    """gate transconductance of the level-1 model, one numpy operation per IEEE operation
    (src/element.cpp:207-270): gg = gm0 (1 + lambda Vds), clipped at 0"""
    p = np.float64(-1.0 if isP else 1.0)
    Vgs = p * (Vg - Vs)
    Vds = p * (Vd - Vs)
    gm0 = np.float64(0.0)
    if Vgs > Vth and Vds >= 0.0:
        Vov = Vgs - Vth
        gm0 = K * Vds if Vds < Vov else K * Vov
    factor = np.float64(1.0) + lam * Vds
    if factor < 0.0:
        factor = np.float64(0.0)
    return gm0 * factor


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_psd_against_definition(name):
    """resistors: kT4 * (1.0 / R) bit for bit; MOSFET channels: kT4 * ((2.0 / 3.0) * |gg|) with gg restated in numpy,
    within 16 ulp (gg is a chain of fewer than ten roundings with no cancellation after the terminal differences;
    whether the device's mos_eval is contracted is not this test's to say)"""
    import torch
    nl, eng, out, src, f = _setup(name)
    params = eng.mc_params(12345, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    r = eng.noise(params, x, freqs=f[:1], out=out, src=-1, temp=TEMP, psd=True)
    torch.cuda.synchronize()
    assert r["gain"] is None and r["contrib"] is None
    psd, P, X = _np(r["psd"]), _np(params), _np(x)
    kT4 = nref.kt4(TEMP)
    assert kT4 == 4.0 * 1.380649e-23 * TEMP
    recs = _records(nl)
    worst, n_mos, n_on = 0.0, 0, 0
    for s, (e, ga, gb) in enumerate(nl.noise_sources):
        kind, q, _, slot = recs[e]
        if kind == 0:
            assert (ga, gb) == (q[0], q[1])
            want = kT4 * (np.float64(1.0) / P[slot])
            assert np.array_equal(_u64(psd[s]), _u64(want)), (name, s)
        else:
            assert kind in (5, 6) and (ga, gb) == (q[0], q[2])
            for i in range(B):
                v = [np.float64(X[t, i]) if t >= 0 else np.float64(0.0) for t in q[:3]]
                gg = _mos_gg(kind == 6, P[slot, i], P[slot + 1, i], P[slot + 2, i], v[0], v[1], v[2])
                want = kT4 * (np.float64(2.0 / 3.0) * np.abs(gg))
                n_mos += 1
                n_on += want > 0
                ulp = np.spacing(want) if want > 0 else np.float64(5e-324)
                dev = abs(float(psd[s, i]) - float(want)) / float(ulp)
                worst = max(worst, dev)
                assert dev <= 16, (name, s, i, psd[s, i], want)
    print("%s: %d MOSFET PSDs (%d conducting), largest deviation from the numpy restatement %.1f ulp" % (name, n_mos, n_on, worst))
    assert n_mos == 0 or n_on > 0


def test_zero_resistance_has_no_noise():
    import torch
    from circuitsimulator_amd import Engine, Netlist
    nl = Netlist.from_file(netlist_path("noise_divider.sp"))
    eng = Engine(nl, 0)
    table = nl.nominal_table(4)
    slot = _records(nl)[1][3]
    table[slot, 2] = 0.0                                      # R1 of instance 2
    params = eng.upload_params(table)
    x, _, _ = eng.dc(params)
    r = eng.noise(params, x, contrib=True, psd=True)
    torch.cuda.synchronize()
    psd, con = _np(r["psd"]), _np(r["contrib"])
    assert psd[0, 2] == 0 and not np.signbit(psd[0, 2]) and np.all(con[:, 0, 2] == 0)
    assert np.all(psd[0, [0, 1, 3]] == nref.kt4(TEMP) * (1.0 / 10e3))
    # closed form of the nominal instances: kT4 (G1 + G2) / (G1 + G2 + gmin)^2, gain G1 / (G1 + G2 + gmin)
    g1, g2 = 1.0 / 10e3, 1.0 / 30e3
    assert np.allclose(_np(r["onoise"])[:, 0], nref.kt4(TEMP) * (g1 + g2) / (g1 + g2 + 1e-6) ** 2, rtol=1e-12)
    assert np.allclose(_np(r["gain"])[:, 0], g1 / (g1 + g2 + 1e-6), rtol=1e-12)


def _ac_chunk(N):
    """instances per chunk of the sweeps: 256 MiB of system scratch (engine_freq.cpp acChunk)"""
    return max(256, (256 << 20) // (8 * (2 * N * N + 2 * N)))


def test_batch_independence():
    """instance b's results are the same bits in a batch of 64, in two halves, and in a batch that crosses the system
    scratch's chunk boundary with an odd second chunk"""
    import torch
    nl, eng, out, src, f = _setup("dbmixer.sp")
    chunk = _ac_chunk(nl.n_unknowns)
    big = chunk + 89
    params = eng.mc_params(12345, 0.05, 0, big)
    x, _, _ = eng.dc(params)

    def run(sel):
        r = eng.noise(params[:, sel].contiguous(), x[:, sel].contiguous(), freqs=f, out=out, src=src, contrib=True, psd=True)
        torch.cuda.synchronize()
        return _bits_of(r), _np(r["status"])
    full, fst = run(slice(0, big))
    assert not np.array_equal(full["onoise"][:, 0], full["onoise"][:, chunk])
    b64, s64 = run(slice(0, B))
    h1, _ = run(slice(0, B // 2))
    h2, _ = run(slice(B // 2, B))
    idx = torch.tensor([0, chunk - 1, chunk, chunk + 1, big - 1], device=params.device)
    tail, tst = run(idx)
    pick = idx.cpu().numpy()
    for k in full:
        assert np.array_equal(b64[k], full[k][..., :B]), k
        assert np.array_equal(np.concatenate([h1[k], h2[k]], axis=-1), b64[k]), k
        assert np.array_equal(tail[k], full[k][..., pick]), k
    assert np.array_equal(s64, fst[:B]) and np.array_equal(tst, fst[pick])


def test_two_sweeps_back_to_back_on_a_stream():
    """csim_noise_batch_dev enqueues and never waits: two sweeps with different frequency lists of equal length on a
    non-blocking stream with nothing between them, then one synchronise; both equal the synchronised runs"""
    import torch
    nl, eng, out, src, _ = _setup("dbmixer.sp")
    nB = 4096
    params = eng.mc_params(2024, 0.05, 0, nB)
    x, _, _ = eng.dc(params)
    f1 = np.array([1e3 * math.pow(10.0, k / 10) for k in range(71)])
    f2 = f1[::-1] * 3.0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a1 = eng.noise(params, x, freqs=f1, out=out, src=src)
        a2 = eng.noise(params, x, freqs=f2, out=out, src=src)
        s.synchronize()
        r1 = eng.noise(params, x, freqs=f1, out=out, src=src)
        s.synchronize()
        r2 = eng.noise(params, x, freqs=f2, out=out, src=src)
        s.synchronize()
    torch.cuda.synchronize()
    for got, want in ((a1, r1), (a2, r2)):
        bg, bw = _bits_of(got), _bits_of(want)
        bad = {k: int(np.count_nonzero(bg[k] != bw[k])) for k in bw}
        print("back-to-back noise sweeps: values that differ from the synchronised run:", bad)
        assert not any(bad.values())
    assert not np.array_equal(_bits_of(a1)["onoise"], _bits_of(a2)["onoise"])


def test_card_defaults():
    """noise_host() with no arguments takes everything from the card; equal to the explicit call"""
    from circuitsimulator_amd import Engine, Netlist
    nl = Netlist.from_file(netlist_path("noise_cs_amp.sp"))
    eng = Engine(nl, 0)
    card = nl.noise
    assert card[3:] == ("dec", 10, 1e3, 1e9)
    d = eng.noise_host()
    e = eng.noise_host(B=1, freqs=nl.noise_freqs(), out=(nl.node_eq("d"), -1), src=_elem_index("noise_cs_amp.sp", "VIN"),
                       temp=300.15)
    assert d["onoise"].shape == (1, 61) and d["gain"].shape == (1, 61)
    assert np.array_equal(_u64(d["onoise"]), _u64(e["onoise"])) and np.array_equal(_u64(d["gain"]), _u64(e["gain"]))
    assert np.all(d["status"] == 0) and np.all(d["onoise"] > 0)
    # the amplifier inverts and amplifies at low frequency; the noise rolls off with the load capacitor
    assert d["gain"][0, 0].real < -1.0 and d["onoise"][0, -1] < d["onoise"][0, 0]
    # layout of the host form: [B][F], [B][F][S], [B][S]
    table = np.repeat(nl.nominal_params[None, :], 3, axis=0)
    h = eng.noise_host(params=table, contrib=True, psd=True)
    assert h["onoise"].shape == (3, 61) and h["contrib"].shape == (3, 61, 2) and h["psd"].shape == (3, 2)
    for i in range(3):
        assert np.array_equal(_u64(h["onoise"][i]), _u64(d["onoise"][0]))
    tot = np.zeros(61)
    for s in range(2):
        tot = tot + h["contrib"][0, :, s]
    assert np.array_equal(_u64(tot), _u64(h["onoise"][0]))


def test_error_paths():
    import torch
    from circuitsimulator_amd import Engine, Netlist, capi
    nl = Netlist.from_file(netlist_path("ac_cs_amp.sp"))              # no .NOISE card
    eng = Engine(nl, 0)
    params = eng.upload_params(nl.nominal_table(2))
    x, _, _ = eng.dc(params)
    d = nl.node_eq("d")

    def code(fn):
        with pytest.raises(capi.CsimError) as e:
            fn()
        return e.value.code
    assert code(lambda: eng.noise(params, x)) == capi.CSIM_ERR_CONFIG
    assert code(lambda: eng.noise_host()) == capi.CSIM_ERR_CONFIG
    L = capi.lib()
    on = np.zeros((1, 1))
    f1 = np.array([1e3])
    assert L.csim_noise_batch(eng._h, None, 1, None, 0, d, -1, -1, 300.15, on.ctypes.data, None, None, None, None) == capi.CSIM_ERR_CONFIG
    assert L.csim_noise_batch(eng._h, None, 1, f1.ctypes.data, 1, -2, -1, -1, 300.15, on.ctypes.data, None, None, None, None) == capi.CSIM_ERR_CONFIG
    assert code(lambda: eng.noise(params, x, freqs=[1e3], out=(d, d))) == capi.CSIM_ERR_ARG
    assert code(lambda: eng.noise(params, x, freqs=[1e3], out=(-1, d))) == capi.CSIM_ERR_ARG
    assert code(lambda: eng.noise(params, x, freqs=[1e3], out=nl.n_unknowns)) == capi.CSIM_ERR_ARG
    rd = _elem_index("ac_cs_amp.sp", "RD")
    assert code(lambda: eng.noise(params, x, freqs=[1e3], out=d, src=rd)) == capi.CSIM_ERR_ARG
    assert code(lambda: eng.noise(params, x, freqs=[1e3], out=d, src=nl.n_elems)) == capi.CSIM_ERR_ARG
    for temp in (0.0, -1.0, float("nan"), float("inf")):
        assert code(lambda: eng.noise(params, x, freqs=[1e3], out=d, temp=temp)) == capi.CSIM_ERR_CONFIG
    # B == 0 and F == 0 do nothing; a good call still works afterwards
    r = eng.noise(params, x, freqs=[], out=d)
    assert tuple(r["onoise"].shape) == (0, 2)
    r = eng.noise(params, x, freqs=[1e3], out=d)
    torch.cuda.synchronize()
    assert np.all(_np(r["onoise"]) > 0) and r["gain"] is None
    # 64 unknowns: beyond the kernels
    S = 62
    lines = ["* RC ladder of %d sections" % S, "V1 n0 0 AC 1 0"]
    for k in range(1, S + 1):
        lines += ["R%d n%d n%d 10" % (k, k - 1, k), "C%d n%d 0 1p" % (k, k)]
    big = Netlist.from_text("\n".join(lines) + "\n")
    assert big.n_unknowns == 64
    beng = Engine(big, 0)
    bp = beng.upload_params(big.nominal_table(1))
    bx, _, _ = beng.dc(bp)
    assert code(lambda: beng.noise(bp, bx, freqs=[1e3], out=big.node_eq("n5"))) == capi.CSIM_ERR_UNSUPPORTED
    assert code(lambda: beng.noise_host(freqs=[1e3], out=big.node_eq("n5"))) == capi.CSIM_ERR_UNSUPPORTED
