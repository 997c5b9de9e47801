"""AC small-signal analysis on the GPU: closed forms, a numpy model of (G + jwC) built from the IR and the engine's
own operating points, the oracle's transient stamp, the two sweep kernels against each other, the 2N real-equivalent
through lu_solve_batch, the transient's small-signal response, and a singular instance."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import has_gpu, netlist_path

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

GMIN = 1e-6          # csim_consts.tran_gmin
PI = 3.14159265358979323846


def _nl(name=None, text=None):
    from circuitsimulator_amd import Netlist
    return Netlist.from_text(text) if text is not None else Netlist.from_file(netlist_path(name))


def _with_ac(name, src):
    text = open(netlist_path(name)).read()
    assert src in text
    return _nl(text=text.replace(src, src.replace(" SIN", " AC 1 SIN"), 1))


def _rel(a, ref, floor):
    return np.max(np.abs(a - ref) / np.maximum(np.abs(ref), floor))


class _IR(C.Structure):
    _fields_ = [("n_unknowns", C.c_int32), ("n_node_eq", C.c_int32), ("n_branch_eq", C.c_int32),
                ("n_elems", C.c_int32), ("n_params", C.c_int32), ("has_nonlinear", C.c_int32),
                ("kind", C.POINTER(C.c_int32)), ("eq", C.POINTER(C.c_int32)), ("branch_eq", C.POINTER(C.c_int32)),
                ("param_slot", C.POINTER(C.c_int32))]


def _records(nl):
    ir = C.cast(nl.ir_ptr, C.POINTER(_IR)).contents
    return [(ir.kind[e], [ir.eq[4 * e + t] for t in range(4)], ir.branch_eq[e], ir.param_slot[e])
            for e in range(ir.n_elems)]


def _numpy_C(nl, p):
    """the C part from the IR records (include/csim.h AC semantics), parameters p [P]"""
    N = nl.n_unknowns
    Cm = np.zeros((N, N))

    def cap(a, b, v):
        if v <= 0.0:
            return
        for i, j, s in ((a, a, 1), (b, b, 1), (a, b, -1), (b, a, -1)):
            if i >= 0 and j >= 0:
                Cm[i, j] += s * v
    for kind, q, k, s in _records(nl):
        if kind == 1:
            cap(q[0], q[1], p[s])
        elif kind == 2 and p[s] > 0.0 and 0 <= k < N:
            Cm[k, k] -= p[s]
        elif kind in (5, 6):
            cj = p[s + 3]
            D, G, S, Bk = q
            cap(G, S, 0.5 * cj)
            cap(G, D, 0.5 * cj)
            cap(S, Bk, cj)
            cap(D, Bk, cj)
    return Cm


def _numpy_J(nl):
    N = nl.n_unknowns
    J = np.zeros(N, dtype=complex)
    for e, (kind, q, k, s) in enumerate(_records(nl)):
        mag, deg = nl.ac_source(e)
        v = mag * complex(math.cos(deg * PI / 180.0), math.sin(deg * PI / 180.0))
        if kind == 3 and 0 <= k < N:
            J[k] += v
        elif kind == 4:
            if q[0] >= 0:
                J[q[0]] -= v
            if q[1] >= 0:
                J[q[1]] += v
    return J


def test_rc_lowpass_closed_form():
    from circuitsimulator_amd import Engine
    nl = _nl("ac_rc_lowpass.sp")
    eng = Engine(nl, 0)
    f = nl.ac_freqs()
    out, st = eng.ac_host(B=1)
    assert out.shape == (1, len(f), nl.n_unknowns) and int(st[0]) == 0
    G = 1.0 / 1e3
    H = G / (G + GMIN + 1j * (2.0 * PI * f) * 1e-9)
    assert _rel(out[0, :, nl.node_eq("out")], H, 1e-300) <= 1e-12
    assert np.all(out[0, :, nl.node_eq("in")] == 1.0)


def test_series_rlc_closed_form():
    from circuitsimulator_amd import Engine
    nl = _nl("ac_rlc_series.sp")
    eng = Engine(nl, 0)
    f = nl.ac_freqs()
    out, st = eng.ac_host(B=2, probes=[nl.node_eq("b"), nl.node_eq("a")])
    assert int(st.max()) == 0
    w = 2.0 * PI * f
    G, Yb = 1.0 / 50.0, GMIN + 1j * w * 1e-9
    Vb = G / ((1.0 + 1j * w * 1e-6 * Yb) * (G + GMIN) + Yb)
    Va = Vb * (1.0 + 1j * w * 1e-6 * Yb)
    assert _rel(out[1, :, 0], Vb, 1e-300) <= 1e-12
    assert _rel(out[0, :, 1], Va, 1e-300) <= 1e-12


def test_rc_ladder_wave_kernel():
    """42 unknowns: beyond the register-resident kernel; auto picks the wave kernel, packed is refused."""
    from circuitsimulator_amd import CsimError, Engine
    nl = _nl("ac_rc_ladder.sp")
    assert nl.n_unknowns == 42
    eng = Engine(nl, 0)
    f = nl.ac_freqs()
    out, st = eng.ac_host(B=1, probes=[nl.node_eq("n40"), nl.node_eq("n20")])
    assert int(st[0]) == 0
    w = 2.0 * PI * f
    R, Cv = 10.0, 1e-12
    ysub = GMIN + 1j * w * Cv                  # admittance seen into node k, from the far end
    ratios = [1.0 / (1.0 + R * ysub)]
    for _ in range(39):
        ysub = GMIN + 1j * w * Cv + 1.0 / (R + 1.0 / ysub)
        ratios.append(1.0 / (1.0 + R * ysub))
    ratios = ratios[::-1]                      # V_k / V_{k-1}, k = 1 .. 40
    v40, v20 = np.prod(ratios, axis=0), np.prod(ratios[:20], axis=0)
    assert _rel(out[0, :, 0], v40, 1e-300) <= 1e-12
    assert _rel(out[0, :, 1], v20, 1e-300) <= 1e-12
    eng.set_option("ac_kernel", "packed")
    with pytest.raises(CsimError):
        eng.ac_host(B=1)


@pytest.fixture(scope="module")
def dbmixer_ac():
    import torch
    from circuitsimulator_amd import Engine
    nl = _with_ac("dbmixer.sp", "Vrf1+ 112 212 SIN")
    eng = Engine(nl, 0)
    B = 256
    params = eng.mc_params(12345, 0.05, 0, B)
    x, _, st = eng.dc(params)
    f = np.array([1e3 * math.pow(10.0, k / 10) for k in range(71)])
    out, st = eng.ac(params, x, freqs=f, status=st)
    G, Cm, J = eng.ac_system(params, x)
    torch.cuda.synchronize()
    return dict(nl=nl, eng=eng, B=B, params=params, x=x, f=f, out=out.cpu().numpy(), st=st.cpu().numpy(),
                G=G.cpu().numpy(), C=Cm.cpu().numpy(), J=J.cpu().numpy())


def test_dbmixer_against_numpy_model(dbmixer_ac):
    from oracle import binding as orc
    d = dbmixer_ac
    nl, B, f = d["nl"], d["B"], d["f"]
    assert int((d["st"] & 0x4).max()) == 0
    ph = d["params"].cpu().numpy()
    xh = d["x"].cpu().numpy()
    J = _numpy_J(nl)
    w = 2.0 * PI * f
    worst = 0.0
    for b in list(range(0, B, 17)) + [B - 1]:
        Go, _ = orc.stamp_tran(nl.ir_ptr, ph, b, xh[:, b].copy(), xh[:, b].copy(), 0.0, 1e300)
        assert np.max(np.abs(d["G"][b] - Go)) <= 1e-300, b
        Cm = _numpy_C(nl, ph[:, b])
        assert np.allclose(d["C"][b], Cm, rtol=1e-14, atol=0), b
        assert np.array_equal(d["J"][b], J)
        for fi in range(len(f)):
            ref = np.linalg.solve(Go + 1j * w[fi] * Cm, J)
            worst = max(worst, _rel(d["out"][fi, :, b], ref, 1e-15))
    assert worst <= 1e-10, worst


def test_dbmixer_real_equivalent_lu_solve_batch(dbmixer_ac):
    from circuitsimulator_amd import lu_solve_batch
    d = dbmixer_ac
    N, B = d["nl"].n_unknowns, d["B"]
    for fi in (0, 40, 70):
        wC = (2.0 * PI * d["f"][fi]) * d["C"]
        A = np.block([[d["G"], -wC], [wC, d["G"]]])
        rhs = np.concatenate([d["J"].real, d["J"].imag], axis=1)
        x, fl = lu_solve_batch(A, rhs)
        assert int(np.max(fl)) == 0
        z = x[:, :N] + 1j * x[:, N:]
        assert _rel(d["out"][fi].T, z, 1e-15) <= 1e-10, fi


@pytest.mark.parametrize("name,src", [("dbmixer.sp", "Vrf1+ 112 212 SIN"), ("buffer.sp", "Vin 101 0 SIN")])
def test_wave_and_packed_bit_identical(name, src):
    from circuitsimulator_amd import Engine
    nl = _with_ac(name, src)
    eng = Engine(nl, 0)
    B = 64
    params = eng.mc_params(12345, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    f = np.array([1e3 * math.pow(10.0, k / 10) for k in range(71)])
    res = {}
    for k in ("wave", "packed"):
        eng.set_option("ac_kernel", k)
        out, st = eng.ac(params, x, freqs=f)
        res[k] = (out.cpu().numpy(), st.cpu().numpy())
    assert np.array_equal(res["wave"][1], res["packed"][1])
    assert np.array_equal(res["wave"][0].view(np.float64), res["packed"][0].view(np.float64))


def test_transient_small_signal_matches_ac():
    """A 10 mV SIN on the AC source, tstep with w dt = 6e-4, phasor fitted over the last two periods.  (With 1 mV the
    per-step change of the output is close to the transient's Newton tolerance, 1e-6: the accepted iterates lag the
    waveform, and the oracle's transient -- which the engine's reproduces -- sits 1.6 % off the small-signal limit.)"""
    from circuitsimulator_amd import Engine
    nl = _nl("ac_cs_amp.sp")
    eng = Engine(nl, 0)
    d = nl.node_eq("d")
    f0 = 1e6
    ac, st = eng.ac_host(B=1, freqs=[f0], probes=[d])
    assert int(st[0]) == 0
    h = ac[0, 0, 0]
    assert abs(h) > 1.0                                  # an amplifier
    tstep, tstop = nl.tstep, nl.tstop
    assert 2.0 * PI * f0 * tstep <= 1e-3
    wave, _, _, tst = eng.tran_host(B=1, probes=[d])
    assert int(tst[0]) & 0x7 == 0
    v = wave[0, :, 0]
    t = np.arange(len(v)) * tstep
    keep = t >= tstop - 2.0 / f0                         # the last two periods
    M = np.stack([np.ones(keep.sum()), np.sin(2 * PI * f0 * t[keep]), np.cos(2 * PI * f0 * t[keep])], axis=1)
    c = np.linalg.lstsq(M, v[keep], rcond=None)[0]
    # v = a sin + b cos = Re((b - j a) e^{jwt}); the input 1e-2 sin(wt) = Re(-1e-2 j e^{jwt})
    phasor = complex(c[2], -c[1]) / (-1e-2j)
    assert abs(phasor - h) / abs(h) <= 0.01, (phasor, h)


def test_singular_instance_flagged_others_unchanged():
    from circuitsimulator_amd import Engine
    nl = _nl("ac_rlc_series.sp")
    eng = Engine(nl, 0)
    slotL = [s for kind, q, k, s in _records(nl) if kind == 2][0]
    good = np.repeat(nl.nominal_params[None, :], 3, axis=0)
    good[1, slotL - 1] = 75.0                            # a different R, so that the instances differ
    bad = np.insert(good, 1, good[0], axis=0)
    bad[1, slotL] = 0.0                                  # L = 0: the transient drops the inductor, its row is empty
    ref, st_ref = eng.ac_host(params=good)
    out, st = eng.ac_host(params=bad)
    assert int(st[1]) & 0x4
    assert np.all(out[1] == 0)
    keep = [0, 2, 3]
    assert np.array_equal(out[keep], ref) and np.array_equal(st[keep], st_ref)
    assert int(st_ref.max()) & 0x4 == 0


# ---- instance chunking, the frequency / probe caches, stream order, excitation, sizes, layout
def _ac_chunk(N):
    """instances per chunk of csim_ac_batch_dev: 256 MiB of system scratch (engine_freq.cpp acChunk)"""
    return max(256, (256 << 20) // (8 * (2 * N * N + 2 * N)))


def _u64(t):
    """device complex tensor or numpy complex array -> its bit pattern, shape + (2,)"""
    a = np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t), dtype=np.complex128)
    return a.view(np.uint64).reshape(a.shape + (2,))


def _spread_params(nl, B, seed):
    """[P][B]: the nominal parameters, every one scaled by its own factor in 1 +- 5 % per instance"""
    rng = np.random.default_rng(seed)
    return nl.nominal_params[:, None] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (nl.n_params, B)))


def _ladder_text(N):
    """RC ladder with N unknowns: N - 2 sections, nodes n0 .. n<N-2>, and the source's branch current"""
    S = N - 2
    lines = ["* RC ladder of %d sections" % S, "V1 n0 0 AC 1 0"]
    for k in range(1, S + 1):
        lines += ["R%d n%d n%d 10" % (k, k - 1, k), "C%d n%d 0 1p" % (k, k)]
    return "\n".join(lines) + "\n"


def _ladder_closed_form(S, f, upto):
    """V(n<upto>) / V(n0) of the S-section ladder, the continued fraction of test_rc_ladder_wave_kernel"""
    w = 2.0 * PI * f
    R, Cv = 10.0, 1e-12
    ysub = GMIN + 1j * w * Cv
    ratios = [1.0 / (1.0 + R * ysub)]
    for _ in range(S - 1):
        ysub = GMIN + 1j * w * Cv + 1.0 / (R + 1.0 / ysub)
        ratios.append(1.0 / (1.0 + R * ysub))
    ratios = ratios[::-1]
    return np.prod(ratios[:upto], axis=0)


def _chunking(nl, eng, params, B, freqs, probes):
    import torch
    N = nl.n_unknowns
    chunk = _ac_chunk(N)
    assert chunk < B - 1 and B - chunk < chunk          # two chunks, the second one short
    assert (B - chunk) % 2 == 1                         # and odd: the last packed wavefront is half empty
    x, _, _ = eng.dc(params)
    out, st = eng.ac(params, x, freqs=freqs, probes=probes)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (len(freqs), len(probes), B)
    full, fst = _u64(out), st.cpu().numpy()
    assert not np.array_equal(full[:, :, 0], full[:, :, chunk]) and not np.array_equal(full[:, :, chunk], full[:, :, B - 1])
    pick = [0, chunk - 1, chunk, chunk + 1, B - 1]
    idx = torch.tensor(pick, device=params.device)
    o5, s5 = eng.ac(params[:, idx].contiguous(), x[:, idx].contiguous(), freqs=freqs, probes=probes)
    assert np.array_equal(_u64(o5), full[:, :, pick])
    assert np.array_equal(s5.cpu().numpy(), fst[pick])
    h = B // 2
    halves = [eng.ac(params[:, a:b].contiguous(), x[:, a:b].contiguous(), freqs=freqs, probes=probes)
              for a, b in ((0, h), (h, B))]
    assert h < chunk and B - h < chunk                  # neither half is chunked
    assert np.array_equal(np.concatenate([_u64(o) for o, _ in halves], axis=2), full)
    assert np.array_equal(np.concatenate([s.cpu().numpy() for _, s in halves]), fst)


def test_chunked_batch_packed_kernel():
    """dbmixer (N = 31): 16 912 instances fill the system scratch; 89 more make a second, odd chunk at b0 > 0"""
    from circuitsimulator_amd import Engine
    nl = _with_ac("dbmixer.sp", "Vrf1+ 112 212 SIN")
    assert nl.n_unknowns == 31 and _ac_chunk(31) == 16912
    eng = Engine(nl, 0)
    B = 16912 + 89
    params = eng.mc_params(12345, 0.05, 0, B)
    _chunking(nl, eng, params, B, [1e5, 1e9], [nl.n_unknowns - 1, 3])


def test_chunked_batch_wave_kernel():
    """the RC ladder (N = 42): 9 289 instances per chunk, 7 in the second"""
    from circuitsimulator_amd import Engine
    nl = _nl("ac_rc_ladder.sp")
    assert nl.n_unknowns == 42 and _ac_chunk(42) == 9289
    eng = Engine(nl, 0)
    B = 9289 + 7
    params = eng.upload_params(_spread_params(nl, B, 42))
    _chunking(nl, eng, params, B, [1e6, 1e9], [nl.node_eq("n40"), nl.node_eq("n20")])


def test_frequency_and_probe_caches():
    """one engine, changing frequency lists (shorter, the first again, longer than ever) and probe lists: every
    result equals a fresh engine's"""
    from circuitsimulator_amd import Engine
    nl = _with_ac("buffer.sp", "Vin 101 0 SIN")
    B = 8
    fa = np.array([1e3, 1e5, 1e7, 1e8, 1e9])
    fb = np.array([2e4, 3e6, 4e8])
    fl = np.array([1e3 * 7.0 ** k for k in range(9)])

    def run(eng, f, probes):
        params = eng.mc_params(777, 0.05, 0, B)
        x, _, _ = eng.dc(params)
        out, st = eng.ac(params, x, freqs=f, probes=probes)
        return _u64(out), st.cpu().numpy()
    eng = Engine(nl, 0)
    for f, probes in ((fa, [3, 1]), (fb, [3, 1]), (fb, None), (fa, None), (fa, [1]), (fl, [1]), (fb, [3, 1]), (fl, None)):
        got = run(eng, f, probes)
        want = run(Engine(nl, 0), f, probes)
        assert got[0].shape == (len(f), nl.n_unknowns if probes is None else len(probes), B, 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (len(f), probes)


def test_two_sweeps_back_to_back_on_a_stream():
    """csim_ac_batch_dev enqueues and never waits: two sweeps on a non-blocking stream with nothing between them --
    frequency lists of equal length and different values, different probe lists -- then one synchronise.  Both
    results equal those of the same calls each followed by a synchronise.  (With the second list copied over the
    buffer the first sweep was still reading, 1 155 072 of the first sweep's 1 163 264 values came out wrong.)"""
    import torch
    from circuitsimulator_amd import Engine
    nl = _with_ac("dbmixer.sp", "Vrf1+ 112 212 SIN")
    eng = Engine(nl, 0)
    B = 4096
    params = eng.mc_params(2024, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    f1 = np.array([1e3 * math.pow(10.0, k / 10) for k in range(71)])
    f2 = f1[::-1] * 3.0
    p1, p2 = [30, 5], [7, 12, 0]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a1, st1 = eng.ac(params, x, freqs=f1, probes=p1)
        a2, st2 = eng.ac(params, x, freqs=f2, probes=p2)
        s.synchronize()
        r1, rs1 = eng.ac(params, x, freqs=f1, probes=p1)
        s.synchronize()
        r2, rs2 = eng.ac(params, x, freqs=f2, probes=p2)
        s.synchronize()
    torch.cuda.synchronize()
    bad1 = int(np.count_nonzero(_u64(a1) != _u64(r1)))
    bad2 = int(np.count_nonzero(_u64(a2) != _u64(r2)))
    print("back-to-back sweeps: %d of %d values of the first, %d of %d of the second differ from the synchronised runs"
          % (bad1, _u64(r1).size, bad2, _u64(r2).size))
    assert bad1 == 0 and bad2 == 0
    assert np.array_equal(st1.cpu().numpy(), rs1.cpu().numpy()) and np.array_equal(st2.cpu().numpy(), rs2.cpu().numpy())


def test_current_source_phase_and_two_sources():
    """I1 a 0 AC 2 30 into R || C, V2 b 0 AC 0.5 -90 through R2 to the same node: superposition, with the sign
    convention of include/csim.h (a current source takes its value out of its first node)"""
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl("ac_isrc_phase.sp")
    eng = Engine(nl, 0)
    f = nl.ac_freqs()
    assert len(f) == 21
    a, b = nl.node_eq("a"), nl.node_eq("b")
    k = [i for i in range(nl.n_unknowns) if i not in (a, b)]
    assert len(k) == 1
    out, st = eng.ac_host(B=1)
    assert int(st[0]) == 0
    w = 2.0 * PI * f
    I1 = 2.0 * complex(math.cos(30.0 * PI / 180.0), math.sin(30.0 * PI / 180.0))
    V2 = 0.5 * complex(math.cos(-90.0 * PI / 180.0), math.sin(-90.0 * PI / 180.0))
    G1, G2 = 1.0 / 1e3, 1.0 / 2e3
    Va = (G2 * V2 - I1) / (G1 + G2 + GMIN + 1j * w * 1e-9)
    Ib = -(G2 * (V2 - Va) + GMIN * V2)
    assert _rel(out[0, :, a], Va, 1e-300) <= 1e-12
    assert _rel(out[0, :, b], np.full(len(f), V2), 1e-300) <= 1e-12
    assert _rel(out[0, :, k[0]], Ib, 1e-300) <= 1e-12
    params = eng.upload_params(nl.nominal_table(1))
    x, _, _ = eng.dc(params)
    _, _, J = eng.ac_system(params, x)
    torch.cuda.synchronize()
    Jn = _numpy_J(nl)
    assert Jn[a] == -I1 and Jn[k[0]] == V2 and Jn[b] == 0
    assert np.array_equal(J.cpu().numpy()[0], Jn)


@pytest.mark.parametrize("N", [17, 24, 25, 32, 33, 63])
def test_ladder_sizes_through_a_netlist(N):
    from circuitsimulator_amd import CsimError, Engine, capi
    nl = _nl(text=_ladder_text(N))
    assert nl.n_unknowns == N
    S = N - 2
    mid = S // 2
    f = np.array([1e3 * math.pow(10.0, k / 5) for k in range(26)])           # the grid of ac_rc_ladder.sp's card
    probes = [nl.node_eq("n%d" % S), nl.node_eq("n%d" % mid)]
    res = {}
    for kern in ("auto", "wave", "packed"):
        eng = Engine(nl, 0)
        eng.set_option("ac_kernel", kern)
        if kern == "packed" and N > 32:
            with pytest.raises(CsimError) as e:
                eng.ac_host(B=1, freqs=f, probes=probes)
            assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
            continue
        out, st = eng.ac_host(B=1, freqs=f, probes=probes)
        assert int(st[0]) == 0
        assert _rel(out[0, :, 0], _ladder_closed_form(S, f, S), 1e-300) <= 1e-12, kern
        assert _rel(out[0, :, 1], _ladder_closed_form(S, f, mid), 1e-300) <= 1e-12, kern
        res[kern] = out
    assert np.array_equal(_u64(res["auto"]), _u64(res["packed" if N <= 32 else "wave"]))
    if N <= 32:
        assert np.array_equal(_u64(res["wave"]), _u64(res["packed"]))


def test_sixty_four_unknowns_and_no_ac_source_are_refused():
    from circuitsimulator_amd import CsimError, Engine, capi
    nl = _nl(text=_ladder_text(64))
    assert nl.n_unknowns == 64
    with pytest.raises(CsimError) as e:
        Engine(nl, 0).ac_host(B=1, freqs=[1e6])
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
    quiet = _nl(text=_ladder_text(10).replace("V1 n0 0 AC 1 0", "V1 n0 0 DC 1"))
    with pytest.raises(CsimError) as e:
        Engine(quiet, 0).ac_host(B=1, freqs=[1e6])
    assert e.value.code == capi.CSIM_ERR_CONFIG


def test_host_layout_and_status_is_ored():
    """csim_ac_batch returns [B][F][n_probe]; the device form [F][n_probe][B] -- with B = 3, F = 4 and two probes a
    swapped index shows.  d_status is OR-ed: bits set before the call stay."""
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl("ac_rlc_series.sp")
    eng = Engine(nl, 0)
    slotL = [s for kind, q, k, s in _records(nl) if kind == 2][0]
    table = np.repeat(nl.nominal_params[None, :], 3, axis=0)
    table[1, slotL - 1], table[2, slotL - 1] = 75.0, 120.0
    f = [1e6, 3e6, 5e6, 9e6]
    probes = [nl.node_eq("b"), nl.node_eq("a")]
    host, hst = eng.ac_host(params=table, freqs=f, probes=probes)
    assert host.shape == (3, 4, 2)
    params = eng.upload_params(table.T)
    x, _, _ = eng.dc(params)
    dev, dst = eng.ac(params, x, freqs=f, probes=probes)
    torch.cuda.synchronize()
    dev = dev.cpu().numpy()
    assert dev.shape == (4, 2, 3)
    assert len({dev[i, j, b] for i in range(4) for j in range(2) for b in range(3)}) == 24
    assert np.array_equal(_u64(host), _u64(np.transpose(dev, (2, 0, 1))))
    assert np.array_equal(hst, dst.cpu().numpy().astype(np.uint32))
    # one singular instance (L = 0), bit 0x20 preset on it and on a regular one
    bad = np.insert(table, 1, table[0], axis=0)
    bad[1, slotL] = 0.0
    params = eng.upload_params(bad.T)
    x, _, _ = eng.dc(params)
    st = torch.tensor([0, 0x20, 0, 0x20], dtype=torch.int32, device=params.device)
    out, st2 = eng.ac(params, x, freqs=f, probes=probes, status=st)
    torch.cuda.synchronize()
    assert st2 is st and st.tolist() == [0, 0x24, 0, 0x20]
    out = out.cpu().numpy()
    assert np.all(out[:, :, 1] == 0)
    assert np.array_equal(_u64(out[:, :, [0, 2, 3]]), _u64(dev))
