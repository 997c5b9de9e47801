"""Loop-gain analysis on the GPU through the engine: Engine.stb against tests/stb_reference.py fed with the engine's own
linearised systems (T and the solutions bit for bit, the margins within stb_cases.MARGIN_BOUND), the sign and the
meaning of the two injections pinned to Engine.ac on netlists derived from the golden one, chunking, the host-pointer
form and the card's defaults, and the refusals."""
import numpy as np
import pytest

import stb_cases as sc
import stb_reference as sref
from conftest import has_gpu, netlist_path

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

PI = 3.14159265358979323846
B = 5
NAMES = ["stb_cs_loop.sp", "stb_cs_loop_p.sp"]

# Engine.stb against T formed in numpy (complex128, the textbook formula with its divisions) from two Engine.ac runs,
# relative to |T|.  The solutions are the same bits (one column never sees another); what differs is the rounding of
# a dozen complex operations, amplified where Tv + Ti + 2 cancels.  Measured on the GPU over the 71 frequencies of both
# golden loops: largest 1.02e-12 (test_sign_and_semantics_against_engine_ac prints it); the bound is ten times that.
AC_BOUND = 1.02e-11


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(t):
    return np.ascontiguousarray(_np(t)).view(np.uint64)


def _margins(r):
    return np.stack([_np(r[k]) for k in ("pm", "fc", "gm", "f180")], axis=1)


@pytest.mark.parametrize("name", NAMES)
def test_engine_equals_reference(name):
    import torch
    from circuitsimulator_amd import Engine, Netlist
    nl = Netlist.from_file(netlist_path(name))
    eng = Engine(nl, 0)
    params = eng.mc_params(12345, 0.05, 0, B)
    x, _, _ = eng.dc(params)
    G, Cm, _ = (_np(t) for t in eng.ac_system(params, x))
    f = nl.stb_freqs()
    omega = 2.0 * PI * f
    probe = nl.stb[1:4]
    refs = [sref.solve_sweep(G[b], Cm[b], omega, probe) for b in range(B)]
    want_m, want_found = zip(*[sref.margins(f, r["t"]) for r in refs])
    assert all(r["flags"] == 0 for r in refs) and list(want_found) == [3] * B
    got, worst = {}, 0.0
    for kernel in ("wave", "packed"):
        eng.set_option("ac_kernel", kernel)
        r = got[kernel] = eng.stb(params, x, want_x=True)     # the card's probe and grid
        torch.cuda.synchronize()
        t, xs = _np(r["t"]), _np(r["x"])
        assert t.shape == (len(f), B) and xs.shape == (len(f), 2, nl.n_unknowns, B)
        assert np.all(_np(r["status"]) == 0), kernel
        for b in range(B):
            assert np.array_equal(_bits(t[:, b]), _bits(refs[b]["t"])), (kernel, b)
            assert np.array_equal(_bits(xs[..., b]), _bits(refs[b]["x"])), (kernel, b)
        assert _np(r["found"]).tolist() == list(want_found), kernel
        worst = max(worst, sc.margins_close(_margins(r), np.stack(want_m)))
    eng.set_option("ac_kernel", "auto")
    for k in ("t", "x", "pm", "fc", "gm", "f180", "found"):
        assert np.array_equal(_np(got["wave"][k]).view(np.uint8), _np(got["packed"][k]).view(np.uint8)), k
    pm = _np(got["wave"]["pm"])
    print("%s: PM %.2f .. %.2f degrees, GM %.2f .. %.2f dB; margins against numpy: largest deviation %.3e"
          % (name, pm.min(), pm.max(), _np(got["wave"]["gm"]).min(), _np(got["wave"]["gm"]).max(), worst))
    assert np.all(pm > 0) and np.ptp(pm) > 0.1                 # the mismatch does spread the margin
    assert np.all(t[0].real > 1.0)                             # negative feedback: positive real at low frequency
    # the probe by its element index, a grid of its own, no margins: T of those frequencies
    r = eng.stb(params, x, freqs=f[10:13], probe=nl.stb[0], margins=False)
    assert r["pm"] is None and r["found"] is None and r["x"] is None
    assert np.array_equal(_bits(r["t"]), _bits(got["wave"]["t"][10:13]))
    # the host-pointer form: its own DC operating point, the card's probe and grid
    rh = eng.stb_host(params=_np(params).T.copy(), want_x=True)
    assert rh["t"].shape == (B, len(f)) and np.all(rh["status"] == 0)
    assert np.array_equal(_bits(rh["t"]), _bits(_np(got["wave"]["t"]).T))
    assert np.array_equal(_bits(rh["x"]), _bits(np.transpose(_np(got["wave"]["x"]), (3, 0, 1, 2))))
    assert np.array_equal(_bits(np.stack([rh[k] for k in ("pm", "fc", "gm", "f180")])), _bits(_margins(got["packed"]).T))
    assert rh["found"].tolist() == [3] * B
    assert eng.stb_host(B=2, margins=False)["pm"] is None


@pytest.mark.parametrize("name", NAMES)
def test_sign_and_semantics_against_engine_ac(name):
    """The two injections as two AC analyses of the code that was there before: `AC 1` on the probe gives vx and vy,
    `Iinj 0 <+node> AC 1` beside a probe with `AC 0` gives ib; T from them by the textbook formula in numpy."""
    from circuitsimulator_amd import Engine, Netlist
    text = open(netlist_path(name)).read()
    assert "Vprobe d fb DC 0\n" in text
    nl = Netlist.from_file(netlist_path(name))
    f = nl.stb_freqs()
    el, ex, ey, ek = nl.stb[:4]

    def ac(derived):
        nd = Netlist.from_text(derived)
        assert nd.eq_names == nl.eq_names
        e = Engine(nd, 0)
        p = e.upload_params(nd.nominal_table(1))
        x, _, _ = e.dc(p)
        out, st = e.ac(p, x, freqs=f)
        assert int(_np(st)[0]) == 0
        return _np(out)[:, :, 0]

    v = ac(text.replace("Vprobe d fb DC 0\n", "Vprobe d fb DC 0 AC 1\n"))
    i = ac(text.replace("Vprobe d fb DC 0\n", "Vprobe d fb DC 0 AC 0\n").replace(".stb ", "Iinj 0 d DC 0 AC 1\n.stb "))
    vx, vy, ib = v[:, ex], v[:, ey], i[:, ek]
    assert np.allclose(vx - vy, 1.0, rtol=1e-12)
    tv, ti = -vx / vy, (1.0 - ib) / ib
    want = (tv * ti - 1.0) / (tv + ti + 2.0)
    eng = Engine(nl, 0)
    p = eng.upload_params(nl.nominal_table(1))
    x, _, _ = eng.dc(p)
    r = eng.stb(p, x, want_x=True)
    t, xs = _np(r["t"])[:, 0], _np(r["x"])[..., 0]
    # the solutions are the AC analysis' own bits: a column is the single right-hand-side solve
    assert np.array_equal(_bits(xs[:, 0]), _bits(v)) and np.array_equal(_bits(xs[:, 1]), _bits(i))
    dev = np.max(np.abs(t - want) / np.abs(want))
    print("%s: Engine.stb against two Engine.ac runs: largest relative deviation %.3e" % (name, dev))
    assert dev <= AC_BOUND
    assert want[0].real > 1.0 and abs(want[0].imag) < 0.01    # a wrong sign of either injection does not survive this


def test_batch_in_halves_and_across_a_chunk_boundary():
    import torch
    from circuitsimulator_amd import Engine, Netlist
    nl = Netlist.from_file(netlist_path(NAMES[0]))
    eng = Engine(nl, 0)
    chunk = eng.stat("ac_chunk")
    assert 256 <= chunk < 1000000
    nb = chunk + 33                                            # a second, odd chunk at b0 = chunk > 0
    params = eng.mc_params(4242, 0.05, 0, nb)
    x, _, _ = eng.dc(params)
    f = nl.stb_freqs()[36:48:2]                                # six points around both crossings
    full = eng.stb(params, x, freqs=f)
    torch.cuda.synchronize()
    keys = ("t", "pm", "fc", "gm", "f180", "found", "status")
    want = {k: _np(full[k]) for k in keys}
    assert np.mean(want["found"] == 3) > 0.99 and np.all(want["status"] == 0)
    pick = list(range(31)) + [chunk - 1, chunk, chunk + 1] + list(range(nb - 30, nb))
    idx = torch.tensor(pick, device=params.device)
    p64, x64 = params[:, idx].contiguous(), x[:, idx].contiguous()
    r64 = eng.stb(p64, x64, freqs=f)
    halves = [eng.stb(p64[:, a:b].contiguous(), x64[:, a:b].contiguous(), freqs=f) for a, b in ((0, 32), (32, 64))]
    torch.cuda.synchronize()
    for k in keys:
        sel = np.take(want[k], pick, axis=-1)
        assert np.array_equal(_np(r64[k]).view(np.uint8), sel.view(np.uint8)), k
        assert np.array_equal(np.concatenate([_np(h[k]) for h in halves], axis=-1).view(np.uint8), sel.view(np.uint8)), k
    assert not np.array_equal(want["t"][:, 0], want["t"][:, chunk])


def _ladder(N):
    """RC ladder with N unknowns, a 0 V probe in its first section: n0, the probe's node, n1 .. and two branch currents"""
    t = ["* ladder", "V1 n0 0 DC 1.2", "Vp n0 m0 DC 0", "R0 m0 n1 10", "C0 n1 0 1p"]
    for k in range(2, N - 3):
        t += ["R%d n%d n%d 10" % (k, k - 1, k), "C%d n%d 0 1p" % (k, k)]
    return "\n".join(t) + "\n"


def _refused(fn, code):
    from circuitsimulator_amd import CsimError
    with pytest.raises(CsimError) as e:
        fn()
    assert e.value.code == code, e.value


def test_entry_refusals():
    from circuitsimulator_amd import Engine, Netlist, capi
    f = np.array([1e6, 2e6])

    def setup(text):
        nl = Netlist.from_text(text)
        eng = Engine(nl, 0)
        params = eng.upload_params(nl.nominal_table(2))
        x, _, _ = eng.dc(params)
        return nl, eng, params, x

    nl, eng, params, x = setup(_ladder(64))
    assert nl.n_unknowns == 64
    _refused(lambda: eng.stb(params, x, freqs=f, probe=1), capi.CSIM_ERR_UNSUPPORTED)
    _refused(lambda: eng.stb_host(B=2, freqs=f, probe=1), capi.CSIM_ERR_UNSUPPORTED)

    nl, eng, params, x = setup(_ladder(33))
    assert nl.n_unknowns == 33
    r = eng.stb(params, x, freqs=f, probe=1)                   # no AC source anywhere: none is needed
    # V1 holds the + node: vx = 0 and ib = 0, so num = 0 while den = vy is not: T is a true zero, no flag
    assert np.all(_np(r["status"]) == 0) and np.all(_np(r["t"]) == 0) and np.all(_np(r["found"]) == 0)
    eng.set_option("ac_kernel", "packed")
    _refused(lambda: eng.stb(params, x, freqs=f, probe=1), capi.CSIM_ERR_UNSUPPORTED)
    eng.set_option("ac_kernel", "block")
    _refused(lambda: eng.stb(params, x, freqs=f, probe=1), capi.CSIM_ERR_UNSUPPORTED)
    assert "block" in capi.lib().csim_last_error().decode()
    _refused(lambda: eng.stb_host(B=2, freqs=f, probe=1), capi.CSIM_ERR_UNSUPPORTED)
    eng.set_option("ac_kernel", "auto")
    _refused(lambda: eng.stb(params, x, freqs=f), capi.CSIM_ERR_CONFIG)                 # no card, no probe
    _refused(lambda: eng.stb(params, x, probe=1), capi.CSIM_ERR_CONFIG)                 # no card, no frequencies
    _refused(lambda: eng.stb_host(B=2, probe=1), capi.CSIM_ERR_CONFIG)
    _refused(lambda: eng.stb(params, x, freqs=f, probe=0), capi.CSIM_ERR_CONFIG)        # V1: its - node is ground
    _refused(lambda: eng.stb(params, x, freqs=f, probe=2), capi.CSIM_ERR_CONFIG)        # R0: not a V source
    _refused(lambda: eng.stb(params, x, freqs=f, probe=nl.n_elems), capi.CSIM_ERR_CONFIG)
    _refused(lambda: eng.stb(params, x, freqs=f, probe=-2), capi.CSIM_ERR_CONFIG)
    for bad in ([0.0, 1e6], [1e6, 1e6], [2e6, 1e6]):                                    # margins need an increasing grid
        _refused(lambda: eng.stb(params, x, freqs=np.array(bad), probe=1), capi.CSIM_ERR_ARG)
        _refused(lambda: eng.stb_host(B=2, freqs=np.array(bad), probe=1), capi.CSIM_ERR_ARG)
        assert np.all(_np(eng.stb(params, x, freqs=np.array(bad), probe=1, margins=False)["status"]) == 0)

    # a card that names a probe the netlist does not have, and one on ground: kept, refused when used
    for card in (".STB Vnowhere DEC 2 1k 1meg", ".STB V1 DEC 2 1k 1meg"):
        nl, eng, params, x = setup(_ladder(8) + card + "\n")
        assert nl.stb is not None
        _refused(lambda: eng.stb(params, x), capi.CSIM_ERR_CONFIG)
        _refused(lambda: eng.stb_host(B=2), capi.CSIM_ERR_CONFIG)
        assert np.all(_np(eng.stb(params, x, probe=1)["status"]) == 0)                   # the probe given: the card's grid
