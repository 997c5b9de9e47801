"""The defaults the host-pointer C entries take from the netlist's cards, reached through capi.lib() directly (the Python
wrappers fill every default in themselves and never get here): a null frequency list with F = 0, out_p_eq = -2,
probe_elem = -1, tstep = f0 = 0.  Each entry is called once with everything left to the card and once with the same
values passed explicitly, taken from the Netlist card tuples; every output array and the status words must be equal
byte for byte.  B = 3, nominal parameters with one column off by 1 % in one instance.  On buffer.sp, which carries
none of the sweep cards, every entry returns the code and the message recorded below."""
import numpy as np
import pytest

from conftest import netlist_path

pytestmark = pytest.mark.gpu

B = 3
TEMP = 300.15
FILL = -7.0                      # what every output holds before a call: both calls must write the same entries


def _setup(name):
    from circuitsimulator_amd import Engine, Netlist
    nl = Netlist.from_file(netlist_path(name))
    params = np.repeat(nl.nominal_params[None, :], B, axis=0).copy()         # [B][P]
    params[1, int(np.flatnonzero(nl.nominal_params)[0])] *= 1.01
    return nl, Engine(nl, 0), params


def _outs(*specs):
    """fresh output arrays: a shape means float64, (shape, dtype) the integer words"""
    arrs = []
    for s in specs:
        shape, dt = s if isinstance(s[-1], type) else (s, np.float64)
        arrs.append(np.full(shape, FILL if dt is np.float64 else 77, dtype=dt))
    return arrs


def _call(name, eng, args):
    from circuitsimulator_amd import capi
    raw = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]
    rc = getattr(capi.lib(), name)(eng._h, *raw)
    return rc, capi.lib().csim_last_error().decode()


def _same(name, eng, shapes, by_card, explicit):
    """by_card, explicit: (outputs) -> the argument list after the engine handle"""
    a, b = _outs(*shapes), _outs(*shapes)
    rc_a, msg_a = _call(name, eng, by_card(a))
    rc_b, msg_b = _call(name, eng, explicit(b))
    assert (rc_a, rc_b) == (0, 0), (msg_a, msg_b)
    assert not np.all(a[0] == FILL), "the call wrote nothing"
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), (name, "output", i)


U32, I32 = np.uint32, np.int32


def test_ac_batch():
    nl, eng, p = _setup("ac_rc_lowpass.sp")
    f = nl.ac_freqs()
    assert nl.ac is not None and len(f) > 1
    _same("csim_ac_batch", eng, [(B, len(f), nl.n_unknowns, 2), ((B,), U32)],
          lambda o: [p, B, None, 0, None, 0, o[0], o[1]],
          lambda o: [p, B, f, len(f), None, 0, o[0], o[1]])


def test_noise_batch():
    nl, eng, p = _setup("noise_rc_lowpass.sp")
    out_p, out_m, src = nl.noise[:3]
    f, S = nl.noise_freqs(), len(nl.noise_sources)
    assert out_p >= 0 and src >= 0 and S > 0
    _same("csim_noise_batch", eng, [(B, len(f)), (B, len(f), 2), (B, len(f), S), (B, S), ((B,), U32)],
          lambda o: [p, B, None, 0, -2, -1, -1, TEMP] + o,
          lambda o: [p, B, f, len(f), out_p, out_m, src, TEMP] + o)


def test_sp_batch():
    nl, eng, p = _setup("sp_resistor.sp")
    f, PP = nl.sp_freqs(), len(nl.ports) ** 2
    _same("csim_sp_batch", eng, [(B, len(f), PP, 2), (B, len(f), PP, 2), ((B,), U32)],
          lambda o: [p, B, None, 0] + o,
          lambda o: [p, B, f, len(f)] + o)


def test_spnoise_batch():
    nl, eng, p = _setup("spn_cs_amp.sp")
    f, PP = nl.sp_freqs(), len(nl.ports) ** 2
    assert PP == 4 and nl.sp_noise
    shapes = [(B, len(f), PP, 2), (B, len(f), PP, 2), (B, len(f)), (B, len(f)), (B, len(f)), (B, len(f), 2), ((B,), U32)]
    _same("csim_spnoise_batch", eng, shapes,
          lambda o: [p, B, None, 0, TEMP] + o,
          lambda o: [p, B, f, len(f), TEMP] + o)


def test_disto_batch():
    nl, eng, p = _setup("disto_cs_amp.sp")
    out_p, out_m = nl.disto[:2]
    f, N, M = nl.disto_freqs(), nl.n_unknowns, len(nl.disto_devices)
    assert out_p >= 0 and M > 0
    _same("csim_disto_batch", eng, [(B, len(f), 3 * N, 2), (B, len(f), 2), (B, M, 7), ((B,), U32)],
          lambda o: [p, B, None, 0, -2, -1] + o,
          lambda o: [p, B, f, len(f), out_p, out_m] + o)


def test_stb_batch():
    nl, eng, p = _setup("stb_cs_loop.sp")
    f, N = nl.stb_freqs(), nl.n_unknowns
    assert nl.stb[0] >= 0
    _same("csim_stb_batch", eng, [(B, len(f), 2), (B, len(f), 2 * N, 2), (B, 4), ((B,), I32), ((B,), U32)],
          lambda o: [p, B, None, 0, -1] + o,
          lambda o: [p, B, f, len(f), nl.stb[0]] + o)


def test_pss_batch():
    nl, eng, p = _setup("pss_rc.sp")
    f0, n_harm = nl.hb
    N = nl.n_unknowns
    assert nl.tran_enabled and n_harm > 0
    _same("csim_pss_batch", eng, [(B, N), (B, n_harm + 1, N, 2), ((B,), I32), ((B,), U32)],
          lambda o: [p, B, 0.0, 0.0, 0, None, 0, 0.0, 0] + o,
          lambda o: [p, B, nl.tstep, f0, n_harm, None, 0, 0.0, 0] + o)


def test_pac_batch():
    nl, eng, p = _setup("pac_switch_mixer.sp")
    f, n_side, N = nl.pac_freqs(), nl.pac[4], nl.n_unknowns
    assert n_side == 2
    _same("csim_pac_batch", eng, [(B, len(f), 2 * n_side + 1, N, 2), (B, N), ((B,), I32), ((B,), U32)],
          lambda o: [p, B, 0.0, 0.0, None, 0, n_side, None, 0] + o,
          lambda o: [p, B, nl.tstep, nl.hb[0], f, len(f), n_side, None, 0] + o)


def test_pnoise_batch():
    nl, eng, p = _setup("pnoise_switch_mixer.sp")
    out_p, out_m, src = nl.pnoise[:3]
    f, n_side, N, S = nl.pnoise_freqs(), nl.pnoise[7], nl.n_unknowns, len(nl.noise_sources)
    nsb = 2 * n_side + 1
    assert out_p >= 0 and out_m >= 0 and src >= 0 and n_side == 2
    shapes = [(B, len(f)), (B, len(f), nsb, 2), (B, len(f), S), (B, len(f), nsb), (B, N), ((B,), I32), ((B,), U32)]
    _same("csim_pnoise_batch", eng, shapes,
          lambda o: [p, B, 0.0, 0.0, None, 0, n_side, -2, -1, -1, TEMP] + o,
          lambda o: [p, B, nl.tstep, nl.hb[0], f, len(f), n_side, out_p, out_m, src, TEMP] + o)


CONFIG, ARG = -7, -1
ONE = np.array([1e6])
# (entry, arguments after the engine handle with `o` one large output buffer, code, message): recorded from the library
# before the cards moved into csim::Cards.  buffer.sp has .TRAN 1e-9 300e-9 and .hb 1e-2 3 (K beyond 2^22), no AC
# source, no port and none of the sweep cards.
NO_CARD = [
    ("csim_ac_batch", lambda p, o: [p, B, None, 0, None, 0, o, o], CONFIG,
     "AC analysis: no source carries an AC magnitude (V/I ... AC mag [phase])"),
    ("csim_noise_batch", lambda p, o: [p, B, None, 0, -2, -1, -1, TEMP, o, None, None, None, o], CONFIG,
     "noise analysis: no frequencies given and the netlist has no .NOISE card"),
    ("csim_noise_batch", lambda p, o: [p, B, ONE, 1, -2, -1, -1, TEMP, o, None, None, None, o], CONFIG,
     "csim_noise_batch: no output given and the netlist has no .NOISE card"),
    ("csim_sp_batch", lambda p, o: [p, B, None, 0, o, o, o], CONFIG,
     "S-parameter analysis: the netlist declares no port (V ... PORTNUM k [Z0 r])"),
    ("csim_spnoise_batch", lambda p, o: [p, B, None, 0, TEMP, o, o, None, None, None, None, o], CONFIG,
     "S-parameter analysis: the netlist declares no port (V ... PORTNUM k [Z0 r])"),
    ("csim_disto_batch", lambda p, o: [p, B, None, 0, -2, -1, None, o, None, o], CONFIG,
     "distortion analysis: no frequencies given and the netlist has no .DISTO card"),
    ("csim_disto_batch", lambda p, o: [p, B, ONE, 1, -2, -1, None, o, None, o], CONFIG,
     "csim_disto_batch: no output given and the netlist has no .DISTO card"),
    ("csim_stb_batch", lambda p, o: [p, B, None, 0, -1, o, None, None, None, o], CONFIG,
     "loop-gain analysis: no frequencies given and the netlist has no .STB card"),
    ("csim_stb_batch", lambda p, o: [p, B, ONE, 1, -1, o, None, None, None, o], CONFIG,
     "loop-gain analysis: no probe given and the netlist has no .STB card"),
    ("csim_pss_batch", lambda p, o: [p, B, 0.0, 0.0, 0, None, 0, 0.0, 0, o, o, None, o], CONFIG,
     "csim_pss_batch: the period 1/f0 must be a whole number of steps, at most 2^22 (|K tstep f0 - 1| <= 1e-9)"),
    ("csim_pac_batch", lambda p, o: [p, B, 0.0, 0.0, None, 0, 1, None, 0, o, o, None, o], ARG,
     "csim_pac_batch: no frequencies given and no .PAC card to take them from"),
    ("csim_pnoise_batch", lambda p, o: [p, B, 0.0, 0.0, None, 0, 1, -2, -1, -1, TEMP, o, None, None, None, o, None, o], ARG,
     "csim_pnoise_batch: no frequencies given and no .PNOISE card to take them from"),
    ("csim_pnoise_batch", lambda p, o: [p, B, 0.0, 0.0, ONE, 1, 1, -2, -1, -1, TEMP, o, None, None, None, o, None, o], CONFIG,
     "csim_pnoise_batch: no output given and the netlist has no .PNOISE card"),
]


def test_without_a_card_on_buffer_sp():
    nl, eng, p = _setup("buffer.sp")
    assert (nl.ac, nl.noise, nl.sp, nl.disto, nl.stb, nl.pac, nl.pnoise) == (None,) * 7 and nl.hb == (1e-2, 3)
    scratch = np.zeros(1 << 16)
    got = [(name,) + _call(name, eng, args(p, scratch)) for name, args, _, _ in NO_CARD]
    for g in got:
        print(g)
    assert got == [(name, code, msg) for name, _, code, msg in NO_CARD]
    assert not scratch.any()
