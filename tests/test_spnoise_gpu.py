"""Two-port noise analysis through the engine: Engine.sp_noise against tests/spnoise_reference.py fed with the engine's
own (G, C) and generator PSDs, the two kernels against each other, the diagonal of Cy against Engine.noise, chunking,
stream order, the host entry point, the card's grid, port counts other than two, and the refusals."""
import numpy as np
import pytest

import spnoise_reference as spnref
from conftest import has_gpu, netlist_path

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

PI = 3.14159265358979323846
FREQS = np.array([1e6, 3.3e7, 1e9])
DBMIXER_PORTS = (("Vrf1+ 112 212 SIN 0.6 0.01 800e6 180", 1), ("Vrf1- 113 213 SIN 0.6  0.01 800e6 0", 2))
KEYS = ("y", "cy", "nf", "fmin", "rn", "yopt")
TEMP = 300.15


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
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        return a.view(np.uint64).reshape(a.shape + (2,))
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _equal(a, b, keys=KEYS):
    return all(np.array_equal(_u64(a[k]), _u64(b[k])) for k in keys)


NAMES = ("spn_cs_amp.sp", "sp_pi_pad.sp", "dbmixer.sp")


@pytest.mark.parametrize("name", NAMES)
def test_engine_equals_reference_and_kernels_agree(name):
    """64 Monte-Carlo instances, 3 frequencies: Y, Cy, NF, Fmin, Rn and Yopt equal the reference fed with the engine's
    (G, C) and PSDs bit for bit, with either kernel; the diagonal of Cy is Engine.noise at the port's branch equation"""
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl(name)
    ports = nl.ports
    pe, z0 = [p[1] for p in ports], [p[2] for p in ports]
    src = nl.noise_sources
    sa, sb = [g[1] for g in src], [g[2] for g in src]
    B = 64
    res = {}
    for kernel in ("wave", "packed"):
        eng = Engine(nl, 0)
        eng.set_option("ac_kernel", kernel)
        params = eng.mc_params(12345, 0.05, 0, B)
        x, _, _ = eng.dc(params)
        r = eng.sp_noise(params, x, freqs=FREQS, temp=TEMP)
        torch.cuda.synchronize()
        assert tuple(r["cy"].shape) == (len(FREQS), 2, 2, B) and tuple(r["nf"].shape) == (len(FREQS), B)
        assert not r["status"].cpu().numpy().any()
        res[kernel] = r
        if kernel == "wave":
            G, C, _ = eng.ac_system(params, x)
            on = [eng.noise(params, x, freqs=FREQS, out=k, src=-1, temp=TEMP, psd=True) for k in pe]
            torch.cuda.synchronize()
            G, C = np.ascontiguousarray(G.cpu().numpy()), np.ascontiguousarray(C.cpu().numpy())
            psd = on[0]["psd"].cpu().numpy()                    # [S][B]
            for i in range(2):
                assert np.array_equal(_u64(on[i]["onoise"]), _u64(r["cy"][:, i, i, :].real)), (name, i)
                assert not r["cy"][:, i, i, :].imag.cpu().numpy().any()
            got = {k: r[k].cpu().numpy() for k in KEYS}
            omega = 2.0 * PI * FREQS
            for b in range(B):
                ref = spnref.sweep(G[b], C[b], omega, pe, z0, sa, sb, psd[:, b])
                assert ref["per_f"] == [0] * len(FREQS)
                for k in KEYS:
                    assert np.array_equal(_u64(ref[k]), _u64(got[k][..., b])), (name, b, k)
    assert _equal(res["wave"], res["packed"])
    if name == "sp_pi_pad.sp":                                  # passive: Cy = kT4 Re(Y) (Twiss), here with the engine's gmin
        cy, y = res["wave"]["cy"].cpu().numpy(), res["wave"]["y"].cpu().numpy()
        assert np.allclose(cy, 4.0 * 1.380649e-23 * TEMP * y.real, rtol=1e-3, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_batch_of_64_in_halves_and_across_a_chunk_boundary(name):
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl(name)
    eng = Engine(nl, 0)
    chunk = eng.stat("ac_chunk")                                # the engine's own figure (it grows as N shrinks)
    assert 256 <= chunk < 1000000
    B = chunk + 33                                              # a second, odd chunk at b0 = chunk > 0
    params = eng.mc_params(4242, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    f = FREQS[:2]
    full = eng.sp_noise(params, x, freqs=f)
    torch.cuda.synchronize()
    want = {k: _u64(full[k]) for k in KEYS}
    fst = full["status"].cpu().numpy()
    pick = list(range(31)) + [chunk - 1, chunk, chunk + 1] + list(range(B - 30, B))
    assert len(pick) == 64
    idx = torch.tensor(pick, device=params.device)
    p64, x64 = params[:, idx].contiguous(), x[:, idx].contiguous()
    r64 = eng.sp_noise(p64, x64, freqs=f)
    halves = [eng.sp_noise(p64[:, a:b].contiguous(), x64[:, a:b].contiguous(), freqs=f) for a, b in ((0, 32), (32, 64))]
    torch.cuda.synchronize()
    assert np.array_equal(r64["status"].cpu().numpy(), fst[pick])
    for k in KEYS:
        ax = 3 if k in ("y", "cy") else 1                       # the instance axis
        sel = np.take(want[k], pick, axis=ax)
        assert np.array_equal(_u64(r64[k]), sel), k
        assert np.array_equal(np.concatenate([_u64(h[k]) for h in halves], axis=ax), sel), k


@pytest.mark.parametrize("name", NAMES)
def test_two_sweeps_back_to_back_on_a_stream(name):
    """csim_spnoise_batch_dev enqueues and never waits: two sweeps with different frequency lists on one stream with no
    synchronisation between them equal their solo runs"""
    import math
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl(name)
    eng = Engine(nl, 0)
    B = 2048
    params = eng.mc_params(2024, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    f1 = np.array([1e3 * math.pow(10.0, k / 5) for k in range(36)])
    f2 = f1[::-1] * 3.0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a1 = eng.sp_noise(params, x, freqs=f1)
        a2 = eng.sp_noise(params, x, freqs=f2)
        s.synchronize()
        r1 = eng.sp_noise(params, x, freqs=f1)
        s.synchronize()
        r2 = eng.sp_noise(params, x, freqs=f2)
        s.synchronize()
    torch.cuda.synchronize()
    assert _equal(a1, r1) and _equal(a2, r2)
    if name != "sp_pi_pad.sp":                                  # the resistive pad does not see the frequency
        assert not np.array_equal(_u64(r1["cy"]), _u64(r2["cy"]))


@pytest.mark.parametrize("name", NAMES)
def test_host_entry_is_the_transposed_device_result(name):
    """csim_spnoise_batch (DC, then the sweep, from host tables) on 64 Monte-Carlo instances: every output is the
    device entry's, instance-major, bit for bit"""
    import torch
    from circuitsimulator_amd import Engine
    eng = Engine(_nl(name), 0)
    B = 64
    params = eng.mc_params(777, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    r = eng.sp_noise(params, x, freqs=FREQS, temp=TEMP)
    torch.cuda.synchronize()
    h = eng.sp_noise_host(params.cpu().numpy().T.copy(), freqs=FREQS, temp=TEMP)
    assert h["cy"].shape == (B, len(FREQS), 2, 2) and h["nf"].shape == (B, len(FREQS)) and not h["status"].any()
    for k in ("y", "cy"):
        assert np.array_equal(_u64(h[k]), _u64(r[k].cpu().numpy().transpose(3, 0, 1, 2))), k
    for k in ("nf", "fmin", "rn", "yopt"):
        assert np.array_equal(_u64(h[k]), _u64(r[k].cpu().numpy().T)), k


def test_card_defaults_and_host_layout():
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl("spn_cs_amp.sp")
    assert nl.sp_noise
    eng = Engine(nl, 0)
    B = 3
    params = eng.mc_params(5, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    r = eng.sp_noise(params, x)
    torch.cuda.synchronize()
    assert np.array_equal(r["freqs"], nl.sp_freqs()) and len(r["freqs"]) == 16
    h = eng.sp_noise_host(params.cpu().numpy().T.copy())
    assert h["cy"].shape == (B, 16, 2, 2) and h["nf"].shape == (B, 16) and not h["status"].any()
    for k in ("y", "cy"):
        assert np.array_equal(_u64(h[k]), _u64(r[k].cpu().numpy().transpose(3, 0, 1, 2))), k
    for k in ("nf", "fmin", "rn", "yopt"):
        assert np.array_equal(_u64(h[k]), _u64(r[k].cpu().numpy().T)), k
    # the temperature moves the generators, not the 290 K the noise factor is referred to
    hot = eng.sp_noise(params, x, temp=2.0 * 300.15)
    torch.cuda.synchronize()
    assert torch.allclose(hot["cy"], 2.0 * r["cy"], rtol=1e-12, atol=0)
    assert torch.allclose(hot["nf"] - 1.0, 2.0 * (r["nf"] - 1.0), rtol=1e-9, atol=0)
    assert torch.equal(torch.view_as_real(hot["y"]), torch.view_as_real(r["y"]))
    # Y is the S-parameter analysis' Y, from the factorisation of the transposed matrix
    sp = eng.sp(params, x)
    torch.cuda.synchronize()
    assert torch.allclose(sp["y"], r["y"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("name,P", [("sp_resistor.sp", 1), ("three", 3)])
def test_other_port_counts_return_y_and_cy_only(name, P):
    from circuitsimulator_amd import CsimError, Engine, capi
    text = _text(name) if name != "three" else (
        "* three ports\nV1 a 0 DC 0 PORTNUM 1\nV2 b 0 DC 0 PORTNUM 2\nV3 c 0 DC 0 PORTNUM 3 Z0 75\n"
        "R1 a b 100\nR2 b c 50\nR3 c 0 20\nC1 b 0 1p\n")
    nl = _nl(text=text)
    eng = Engine(nl, 0)
    r = eng.sp_noise_host(B=2, freqs=[1e6, 1e9], temp=290.0)
    assert sorted(r) == ["cy", "freqs", "status", "y"] and r["cy"].shape == (2, 2, P, P)
    assert np.allclose(r["cy"], spnref.KT4_0 * r["y"].real, rtol=1e-3, atol=1e-30)          # passive: Twiss, but for gmin
    with pytest.raises(ValueError):
        eng.sp_noise_host(B=2, freqs=[1e6], noise_params=True)
    # the library's own answer (the Python wrapper refuses earlier)
    f, cy, nf, st = np.array([1e6]), np.zeros((1, 1, P, P, 2)), np.zeros((1, 1)), np.zeros(1, dtype=np.uint32)
    rc = capi.lib().csim_spnoise_batch(eng._h, None, 1, f.ctypes.data, 1, 290.0, None, cy.ctypes.data, nf.ctypes.data, None,
                                       None, None, st.ctypes.data)
    assert rc == capi.CSIM_ERR_CONFIG
    with pytest.raises(CsimError) as e:
        eng.sp_noise_host(B=1, freqs=[1e6], temp=0.0)
    assert e.value.code == capi.CSIM_ERR_CONFIG


def test_errors():
    from circuitsimulator_amd import CsimError, Engine, capi
    eng = Engine(_nl(text=open(netlist_path("ac_rc_lowpass.sp")).read()), 0)        # no ports
    with pytest.raises(CsimError) as e:
        eng.sp_noise_host(freqs=[1e3])
    assert e.value.code == capi.CSIM_ERR_CONFIG
    eng = Engine(_nl(text="* r\nV1 a 0 DC 0 PORTNUM 1\nR1 a 0 50\n"), 0)            # ports, no card, no frequencies
    with pytest.raises(CsimError) as e:
        eng.sp_noise_host()
    assert e.value.code == capi.CSIM_ERR_CONFIG
    for temp in (-1.0, float("nan"), float("inf")):
        with pytest.raises(CsimError) as e:
            eng.sp_noise_host(freqs=[1e3], temp=temp)
        assert e.value.code == capi.CSIM_ERR_CONFIG

    def ladder(N):                                              # N unknowns: N - 2 sections, n0 and the branch current
        lines = ["* ladder", "V1 n0 0 DC 0 PORTNUM 1"]
        for k in range(1, N - 1):
            lines += ["R%d n%d n%d 10" % (k, k - 1, k), "C%d n%d 0 1p" % (k, k)]
        return "\n".join(lines) + "\n"
    nl = _nl(text=ladder(64))
    assert nl.n_unknowns == 64
    with pytest.raises(CsimError) as e:
        Engine(nl, 0).sp_noise_host(freqs=[1e3])
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
    nl = _nl(text=ladder(33))
    eng = Engine(nl, 0)
    assert eng.sp_noise_host(freqs=[1e6])["cy"].shape == (1, 1, 1, 1)
    eng.set_option("ac_kernel", "packed")
    with pytest.raises(CsimError) as e:
        eng.sp_noise_host(freqs=[1e6])
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED


def test_singular_at_dc_only():
    """a V source across an inductor is singular at w = 0 and regular elsewhere: +0.0 everywhere at that frequency only,
    the flag set, the other frequencies the reference's"""
    import torch
    from circuitsimulator_amd import Engine
    nl = _nl(text="* loop\nV1 a 0 DC 0 PORTNUM 1\nV2 b 0 DC 0 PORTNUM 2\nR2 a b 30\nL1 a 0 1u\nR1 a 0 1k\n")
    eng = Engine(nl, 0)
    params = eng.upload_params(nl.nominal_table(2))
    x, _, _ = eng.dc(params)
    f = np.array([1e6, 0.0, 2e6])
    r = eng.sp_noise(params, x, freqs=f)
    torch.cuda.synchronize()
    assert r["status"].cpu().numpy().tolist() == [4, 4]
    for k in KEYS:
        v = _u64(r[k])[1]
        assert not v.any(), k                                   # +0.0: no bit set
    assert np.all(r["cy"].cpu().numpy()[[0, 2]].real != 0) and np.all(r["nf"].cpu().numpy()[[0, 2]] > 1.0)
