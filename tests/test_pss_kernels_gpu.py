"""The kernels of the periodic-steady-state analysis (kernels_pss.hip) bit for bit: the forward trajectory of the period
kernel is the general transient's, its harmonics are the numpy DFT of that waveform over the library's table; chunks and
probe lists change no bit; an instance whose start is not finite stops alone."""
import numpy as np
import pytest

import pss_cases as pc
import pss_reference as pr
from circuitsimulator_amd import capi, pss_twiddles
from conftest import has_gpu
from test_pss_gpu import _bits, run, tran_from

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


@pytest.mark.parametrize("name,B", [(n, 65) for n in pc.CASES] + [(n, 3) for n in pc.SHIPPED])
def test_forward_bits(name, B):
    """max_rounds = 1: the period starts at the caller's state, so the harmonics are those of the general transient's K
    steps from it.  Every harmonic's sum ends with the term of x_K and the row m = 0 is the plain sum of all K states, so
    a bit of x_K (or of any x_k) that differed would show here; x_K itself is not an output of the entry."""
    import torch
    g = run(name, B)
    K, H = g["K"], g["H"]
    r = g["eng"].pss(g["params"], g["x_dc"], tstep=g["h"], f0=1.0 / (K * g["h"]), n_harm=H, max_rounds=1)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(r["x0"]), _bits(g["x_dc"])) and np.all(r["rounds"].cpu().numpy() == 1)
    xe, st, wave = tran_from(g, g["x_dc"], K, wave=True)
    assert np.array_equal(_bits(wave[K]), _bits(xe)) and np.array_equal(_bits(wave[0]), _bits(g["x_dc"]))
    c, s = pss_twiddles(K)
    harm = r["harm"].cpu().numpy()
    closed = np.max(np.abs(xe - g["x_dc"].cpu().numpy()), axis=0) < pr.TOL
    status = r["status"].cpu().numpy().astype(np.uint32)
    for b in range(B):
        want = pr.dft(np.ascontiguousarray(wave[1:, :, b]), c, s, H)
        assert np.array_equal(_bits(harm[:, :, b].real), _bits(want.real)), (name, b)
        assert np.array_equal(_bits(harm[:, :, b].imag), _bits(want.imag)), (name, b)
        assert bool(status[b] & capi.ST_PSS_NONCONV) == (not closed[b])     # the closure test saw the transient's x_K
        assert (status[b] & 0x3) == (st[b] & 0x3)                             # the transient's own bits, as the transient sets them


def test_x_K_itself_through_the_divider():
    """x_K bit for bit, directly.  The divider has W_K = 0, so I - W_K is the identity and the update's solve returns
    r = x_K - x0 untouched (no elimination step, divisions by 1.0).  With a tol no closure can meet, round 1 updates:
    the returned state is x0 + (x_K - x0) in the kernel's arithmetic, which numpy repeats from Engine.tran's final state.
    Round 2 then starts where round 1 ended: its closure is what the transient gives from there."""
    import torch
    g = run("divider", 65)
    r = g["eng"].pss(g["params"], g["x_dc"], tstep=g["h"], f0=1.0 / (g["K"] * g["h"]), n_harm=g["H"], tol=1e-300, max_rounds=2)
    torch.cuda.synchronize()
    assert np.all(r["rounds"].cpu().numpy() == 2)
    x0 = g["x_dc"].cpu().numpy()
    xe, _, _ = tran_from(g, g["x_dc"], g["K"])
    assert np.any(xe != x0)
    want = x0 + (xe - x0)
    assert np.array_equal(_bits(r["x0"]), _bits(want))
    # where x0 is zero (the divider's DC point: the SIN source starts at 0 V), or within a factor of two of x_K, the
    # difference and the sum are exact: there the returned state is x_K itself
    exact = ((x0 == 0.0) | ((np.abs(xe) <= 2 * np.abs(x0)) & (np.abs(x0) <= 2 * np.abs(xe)))) & (xe != 0.0)
    assert exact.any() and np.array_equal(_bits(r["x0"].cpu().numpy()[exact]), _bits(xe[exact]))


def test_probe_list_and_chunks_change_no_bits():
    import torch
    g = run("cs", 65)
    eng, nl = g["eng"], g["nl"]
    kw = dict(tstep=g["h"], f0=1.0 / (g["K"] * g["h"]), n_harm=g["H"])
    probes = [nl.node_eq("d"), nl.node_eq("g"), nl.node_eq("d")]
    some = eng.pss(g["params"], g["x_dc"], probes=probes, **kw)
    eng.set_option("pss_chunk", 32)                                      # 32 + 32 + 1 instances
    try:
        chunked = eng.pss(g["params"], g["x_dc"], **kw)
        odd = eng.pss(g["params"][:, :33].contiguous(), g["x_dc"][:, :33].contiguous(), **kw)
    finally:
        eng.set_option("pss_chunk", 0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(some["harm"]), _bits(g["harm"][:, probes, :]))
    for k in ("x0", "rounds", "status"):
        assert np.array_equal(_bits(some[k]), _bits(g[k]))
    for k in ("x0", "harm", "rounds", "status"):
        assert np.array_equal(_bits(chunked[k]), _bits(g[k])), k
        assert np.array_equal(_bits(odd[k]), _bits(g[k][..., :33])), k


def test_a_start_that_is_not_finite_stops_its_instance_only():
    """an input check: the kernel looks at the start vector before it integrates"""
    import torch
    g = run("cs", 3)
    x = g["x_dc"].clone()
    x[1, 1] = float("nan")
    r = g["eng"].pss(g["params"], x, tstep=g["h"], f0=1.0 / (g["K"] * g["h"]), n_harm=g["H"])
    torch.cuda.synchronize()
    st = r["status"].cpu().numpy().astype(np.uint32)
    assert st[1] & capi.ST_TRAN_NONFINITE and not (st[1] & capi.ST_PSS_NONCONV) and r["rounds"].cpu().numpy()[1] == 1
    assert np.all(_bits(r["harm"][:, :, 1]) == 0)                        # a stopped instance reports zeros, not leftovers
    h = g["eng"].pss_host(params=np.ascontiguousarray(pc.params(g["nl"], 3).T), tstep=g["h"], f0=1.0 / (g["K"] * g["h"]),
                          n_harm=g["H"])
    assert np.array_equal(_bits(np.ascontiguousarray(np.moveaxis(h["harm"], 0, 2))), _bits(g["harm"]))
    for b in (0, 2):
        assert st[b] == g["status"][b]
        assert np.array_equal(_bits(r["x0"][:, b]), _bits(g["x0"][:, b]))
        assert np.array_equal(_bits(r["harm"][:, :, b]), _bits(g["harm"][:, :, b]))
        assert r["rounds"].cpu().numpy()[b] == g["rounds"][b]
