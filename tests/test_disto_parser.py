"""The .DISTO card and the device list of the distortion analysis: the card's forms and its errors, the shipped
netlists' IR unchanged by an added card, the MOSFET lists of buffer.sp and dbmixer.sp.  No GPU."""
import numpy as np
import pytest

from conftest import netlist_path

STAGE = """* degenerated common-source stage
VDD vdd 0 DC 3
VIN g 0 DC 1.2 AC 1m
RD vdd d 2k
RS s 0 200
M1 d g s n 10e-6 1e-6 2
.MODEL 2 VT 0.5 MU 3e-2 COX 6e-3 LAMBDA 0.05 CJ0 4.0e-14
"""


def _nl(text):
    from circuitsimulator_amd import Netlist
    return Netlist.from_text(text)


@pytest.mark.parametrize("card,out_m,grid", [
    (".DISTO V(d) DEC 10 1k 1g", None, ("dec", 10, 1e3, 1e9)),
    (".disto v(d) oct 3 10 1meg", None, ("oct", 3, 10.0, 1e6)),
    (".DISTO V(d,s) LIN 5 1 100", "s", ("lin", 5, 1.0, 100.0)),
    (".DISTO V(d, s) LIN 5 1 100", "s", ("lin", 5, 1.0, 100.0)),
    (".DISTO V(d,0) DEC 2 1 10", None, ("dec", 2, 1.0, 10.0)),
])
def test_disto_card_forms(card, out_m, grid):
    from circuitsimulator_amd.engine import ac_freqs
    nl = _nl(STAGE + card + "\n")
    assert nl.n_elems == 5
    want_m = -1 if out_m is None else nl.node_eq(out_m)
    assert nl.disto == (nl.node_eq("d"), want_m) + grid
    assert nl.node_eq("d") >= 0 and (out_m is None or want_m >= 0)
    assert np.array_equal(nl.disto_freqs(), ac_freqs(*grid))
    assert nl.ac is None and nl.noise is None and nl.sp is None


def test_disto_card_absent_invalid_and_beside_the_others():
    from circuitsimulator_amd import capi
    nl = _nl(STAGE)
    assert nl.disto is None
    with pytest.raises(capi.CsimError) as e:
        nl.disto_freqs()
    assert e.value.code == capi.CSIM_ERR_CONFIG
    for bad in (".DISTO", ".DISTO V(d) DEC 10 1k", ".DISTO I(VIN) DEC 10 1 1k", ".DISTO V(d) VIN DEC 10 1 1k",
                ".DISTO V(d) DEC ten 1 1k", ".DISTO V(d) DEC 10 1 1k 0.9",          # f2overf1: two tones are out of scope
                ".DISTO DEC 10 1 1k", ".DISTO V(d) SWEEP 10 1 1k"):
        assert _nl(STAGE + bad + "\n").disto is None, bad
    both = _nl(STAGE + ".AC OCT 4 10 1k\n.NOISE V(d) VIN DEC 10 1 1k\n.DISTO V(s) LIN 3 5 50\n")
    assert both.ac == ("oct", 4, 10.0, 1000.0) and both.noise[3:] == ("dec", 10, 1.0, 1000.0)
    assert both.disto == (both.node_eq("s"), -1, "lin", 3, 5.0, 50.0)
    # an output node the netlist does not have: the card is kept, the equation is -2 (refused when used)
    assert _nl(STAGE + ".DISTO V(nowhere) DEC 10 1 1k\n").disto[0] == -2


def _expected_devices(text, nl):
    """MOSFETs with their drain, gate and source equations, in element order, from the netlist text"""
    out, elem = [], 0
    for line in text.splitlines():
        line = line.split("$")[0].strip()
        if not line or line[0] in "*;.+":
            continue
        tok = line.split()
        head = tok[0][0].upper()
        if head not in "RCLVIM":
            continue
        if head == "M":
            out.append((elem, nl.node_eq(tok[1]), nl.node_eq(tok[2]), nl.node_eq(tok[3])))
        elem += 1
    return out, elem


@pytest.mark.parametrize("name,n_m", [("buffer.sp", 4), ("dbmixer.sp", 6), ("disto_cs_amp.sp", 1), ("disto_cs_amp_p.sp", 1),
                                      ("noise_divider.sp", 0)])
def test_device_list(name, n_m):
    from circuitsimulator_amd import Netlist
    text = open(netlist_path(name)).read()
    nl = Netlist.from_file(netlist_path(name))
    want, n_elems = _expected_devices(text, nl)
    assert n_elems == nl.n_elems
    assert nl.disto_devices == want and len(want) == n_m
    # the channel generators of the noise analysis are the same devices, drain - source
    assert [(e, d, s) for e, d, _, s in want] == [g for g in nl.noise_sources if g[0] in {w[0] for w in want}]
    if name == "buffer.sp":
        assert -1 in [s for _, _, _, s in want]                # M2 and M4 have their sources on ground


@pytest.mark.parametrize("name,card", [("buffer.sp", ".DISTO V(118) DEC 10 1k 1g"),
                                       ("dbmixer.sp", ".disto v(102,103) dec 5 1e5 1e10")])
def test_shipped_netlists_unchanged_by_disto_card(name, card):
    """A .DISTO card changes neither P, nor the nominal parameters, the equation names, the CSV header, the probes, the
    other cards, the generator list or the device list."""
    from circuitsimulator_amd import Netlist
    text = open(netlist_path(name)).read()
    ref = Netlist.from_text(text)
    assert ref.disto is None
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.strip().lower().startswith(".tran"))
    nz = Netlist.from_text("\n".join(lines[:at] + [card] + lines[at:]) + "\n")
    assert nz.disto is not None and nz.disto[0] >= 0
    assert nz.n_params == ref.n_params and nz.n_unknowns == ref.n_unknowns and nz.n_elems == ref.n_elems
    assert np.array_equal(nz.nominal_params, ref.nominal_params)
    assert nz.eq_names == ref.eq_names
    assert nz.csv_header == ref.csv_header
    assert nz.probes == ref.probes
    assert np.array_equal(nz.mc_kinds, ref.mc_kinds)
    assert (nz.tran_enabled, nz.tstep, nz.tstop, nz.tstart) == (ref.tran_enabled, ref.tstep, ref.tstop, ref.tstart)
    assert (nz.ac, nz.noise, nz.sp) == (ref.ac, ref.noise, ref.sp)
    assert nz.noise_sources == ref.noise_sources and nz.disto_devices == ref.disto_devices
    if name == "buffer.sp":
        assert nz.n_params == 36


def test_golden_netlists_carry_a_card():
    from circuitsimulator_amd import Netlist
    for name in ("disto_cs_amp.sp", "disto_cs_amp_p.sp"):
        nl = Netlist.from_file(netlist_path(name))
        assert nl.disto == (nl.node_eq("d"), -1, "dec", 5, 1e3, 1e9), name
        assert len(nl.disto_freqs()) == 31 and len(nl.disto_devices) == 1
