"""AC, noise, S-parameter and two-port noise analysis share one chunk driver, one frequency-list cache, one system
scratch and one PSD scratch per engine (engine_freq.cpp): whatever ran before on an engine, every call gives the bits
the same call gives on an engine that has done nothing else."""
import numpy as np
import pytest

from conftest import has_gpu, netlist_path

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

# Of the two-port netlists with noise generators that tests/test_spnoise_gpu.py uses, the smallest whose answers depend
# on the frequency (5 unknowns; the 4 of sp_pi_pad.sp are resistive, so a stale frequency list would not show there).
# Its VIN carries the AC magnitude already.
NETLIST = "spn_cs_amp.sp"
B = 3
LISTS = (np.array([1e6, 2e8]), np.array([3.3e7, 1e9]), np.array([5e6, 7e8]))
CALLS = ("ac", "noise_psd", "noise", "sp", "sp_noise")


def _bits(v):
    a = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        return a.view(np.uint64).reshape(a.shape + (2,))
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _run(eng, nl, call, params, x, freqs):
    """one analysis -> {name: result}, device tensors (nothing waits here)"""
    if call == "ac":
        out, st = eng.ac(params, x, freqs=freqs)
        return dict(out=out, status=st)
    if call in ("noise", "noise_psd"):
        r = eng.noise(params, x, freqs=freqs, out=nl.node_eq("d"), src=nl.ports[0][0], contrib=True, psd=call == "noise_psd")
    elif call == "sp":
        r = eng.sp(params, x, freqs=freqs)
    else:
        r = eng.sp_noise(params, x, freqs=freqs)
    return {k: v for k, v in r.items() if k != "freqs" and v is not None}


@pytest.mark.parametrize("kernel", ["auto", "wave"])
def test_any_order_of_analyses_on_one_engine_gives_a_fresh_engines_bits(kernel):
    import torch
    from circuitsimulator_amd import Engine, Netlist
    text = open(netlist_path(NETLIST)).read()
    assert "VIN g 0 DC 0.9 AC 1 " in text
    nl = Netlist.from_text(text)

    def engine():
        e = Engine(nl, 0)
        e.set_option("ac_kernel", kernel)
        return e

    eng = engine()
    params = eng.mc_params(777, 0.05, 0, B)
    x, _, _ = eng.dc(params)

    fresh = {}

    def reference(call, li):
        if (call, li) not in fresh:
            r = _run(engine(), nl, call, params, x, LISTS[li])
            torch.cuda.synchronize()
            fresh[(call, li)] = {k: _bits(v) for k, v in r.items()}
        return fresh[(call, li)]

    first = [(c, i % 3) for i, c in enumerate(CALLS)]
    rotated = [(c, (i + 1) % 3) for i, c in reversed(list(enumerate(CALLS)))]
    for sequence in (first, rotated, first):
        got = [_run(eng, nl, c, params, x, LISTS[li]) for c, li in sequence]       # enqueued back to back
        torch.cuda.synchronize()
        for (c, li), r in zip(sequence, got):
            want = reference(c, li)
            assert sorted(r) == sorted(want)
            assert "status" in r and (c != "noise_psd" or "psd" in r) and (c != "noise" or "psd" not in r)
            for k in want:
                assert np.array_equal(_bits(r[k]), want[k]), (kernel, c, li, k)
    assert len(fresh) == 10                                     # five analyses, two lists each
    assert not np.array_equal(fresh[("sp", 0)]["y"], fresh[("sp", 1)]["y"])        # the lists do matter
