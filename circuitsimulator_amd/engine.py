"""Host-side mirror of the reference's analysis interface over the C-ABI.

Netlist  ~ parseNetlist() + Circuit::assignEquationIndices()   (src/main.cpp:29,34)
Engine.dc    ~ computeDcOperatingPoint()                       (include/tanalisis.hpp:9)
Engine.tran  ~ runTransientAnalysisBackwardEuler()             (include/tanalisis.hpp:15-17)
lu_solve_batch ~ Solver::solveLinearSystemLU()                 (include/solver.hpp:83-131)

for a BATCH of instances.  torch is used for device memory and streams only;
all arithmetic happens in the HIP kernels behind include/csim.h.
"""
import ctypes as C

import numpy as np

from . import capi


AC_SWEEPS = ("dec", "oct", "lin")


def ac_freqs(sweep, n_points, fstart, fstop):
    """SPICE frequency grid (csim_ac_freqs): sweep "dec" | "oct" | "lin" (or 0, 1, 2) -> numpy [F], Hz."""
    sw = AC_SWEEPS.index(sweep.lower()) if isinstance(sweep, str) else int(sweep)
    L = capi.lib()
    n = L.csim_ac_num_freqs(sw, int(n_points), float(fstart), float(fstop))
    if n < 0:
        capi.check(int(n))
    f = np.zeros(n, dtype=np.float64)
    capi.check(L.csim_ac_freqs(sw, int(n_points), float(fstart), float(fstop), f.ctypes.data))
    return f


def pss_num_steps(tstep, f0):
    """K = round(1 / (f0 tstep)), the steps of one period (csim_pss_num_steps); raises CsimError when the step does not
    divide the period or K exceeds 2^22."""
    K = capi.lib().csim_pss_num_steps(float(tstep), float(f0))
    if K < 0:
        capi.check(int(K))
    return int(K)


def pss_twiddles(K):
    """The library's own table of the periodic steady state's harmonics (csim_pss_twiddles):
    -> (cos(2 pi j / K), sin(2 pi j / K)), numpy [K] each."""
    c, s = np.zeros(int(K)), np.zeros(int(K))
    capi.check(capi.lib().csim_pss_twiddles(int(K), c.ctypes.data, s.ctypes.data))
    return c, s


class Netlist:
    """A parsed, indexed and flattened netlist (host only)."""

    def __init__(self, handle, source=None):
        self._h = handle
        self.source = source
        L = capi.lib()
        c = [C.c_int32() for _ in range(5)]
        capi.check(L.csim_netlist_counts(self._h, *[C.byref(v) for v in c]))
        self.n_nodes, self.n_elems, self.n_unknowns, self.n_node_eq, self.n_branch_eq = [v.value for v in c]
        self.eq_names = [L.csim_netlist_eq_name(self._h, i).decode() for i in range(self.n_unknowns)]
        en, ts, tp, t0 = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
        capi.check(L.csim_netlist_tran(self._h, C.byref(en), C.byref(ts), C.byref(tp), C.byref(t0)))
        self.tran_enabled, self.tstep, self.tstop, self.tstart = bool(en.value), ts.value, tp.value, t0.value
        self.probes = [L.csim_netlist_probe_eq(self._h, i) for i in range(L.csim_netlist_num_probes(self._h))]
        need = L.csim_netlist_csv_header(self._h, None, 0)
        buf = C.create_string_buffer(need + 1)
        L.csim_netlist_csv_header(self._h, buf, need + 1)
        self.csv_header = buf.value.decode()
        self.n_params = self._n_params()
        self.nominal_params = np.zeros(self.n_params, dtype=np.float64)
        capi.check(L.csim_netlist_nominal_params(self._h, self.nominal_params.ctypes.data))
        self.mc_kinds = np.zeros(self.n_params, dtype=np.int32)
        capi.check(L.csim_netlist_mc_kinds(self._h, self.mc_kinds.ctypes.data))
        # the .AC card: None, or (sweep "dec" | "oct" | "lin", n_points, fstart, fstop)
        self.ac = self._card("ac")

    # -- the sweep cards: one reader, one grid; a card is None when the netlist has none ---------------------------
    def _card(self, name, lead=0, tail=0, dtail=0):
        """What csim_netlist_<name> reports: None, or (`lead` resolved indices, sweep "dec" | "oct" | "lin", n_points,
        fstart, fstop, `tail` further ints or `dtail` further doubles) -- the order of the getter's arguments after
        `enabled`."""
        ints = [C.c_int32() for _ in range(1 + lead + 2)]
        grid = [C.c_double(), C.c_double()]
        more = [C.c_int32() for _ in range(tail)] + [C.c_double() for _ in range(dtail)]
        capi.check(getattr(capi.lib(), "csim_netlist_" + name)(self._h, *[C.byref(x) for x in ints + grid + more]))
        if not ints[0].value:
            return None
        return (tuple(x.value for x in ints[1:1 + lead]) + (AC_SWEEPS[ints[-2].value], ints[-1].value)
                + tuple(x.value for x in grid + more))

    @staticmethod
    def _card_freqs(name, card, grid):
        """Frequency grid of a card (numpy, Hz); `grid` is the slice of its tuple that holds sweep .. fstop."""
        if card is None:
            raise capi.CsimError(capi.CSIM_ERR_CONFIG, "the netlist has no .%s card" % name)
        return ac_freqs(*card[grid])

    @property
    def noise(self):
        """The .NOISE card: None, or (out_p_eq, out_m_eq, src_elem, sweep, n_points, fstart, fstop); out_m_eq -1 =
        ground, src_elem -1 = no input source."""
        return self._card("noise", lead=3)

    @property
    def disto(self):
        """The .DISTO card: None, or (out_p_eq, out_m_eq, sweep, n_points, fstart, fstop); out_m_eq -1 = ground."""
        return self._card("disto", lead=2)

    @property
    def imd(self):
        """The .IMD card: None, or (out_p_eq, out_m_eq, sweep, n_points, fstart, fstop, f2overf1); out_m_eq -1 = ground."""
        return self._card("imd", lead=2, dtail=1)

    @property
    def stb(self):
        """The .STB card: None, or (probe element, eq_p, eq_m, eq_br, sweep, n_points, fstart, fstop).  The element is -2
        for a name the netlist does not have; the equations are -2 when the probe is not a V source, -1 = ground."""
        return self._card("stb", lead=4)

    @property
    def pac(self):
        """The .PAC card: None, or (sweep "dec" | "oct" | "lin", n_points, fstart, fstop, n_side)."""
        return self._card("pac", tail=1)

    @property
    def pnoise(self):
        """The .PNOISE card: None, or (out_p_eq, out_m_eq, src_elem, sweep, n_points, fstart, fstop, n_side); out_m_eq
        -1 = ground, src_elem -1 = no input source."""
        return self._card("pnoise", lead=3, tail=1)

    @property
    def sp(self):
        """The .SP card: None, or (sweep "dec" | "oct" | "lin", n_points, fstart, fstop)."""
        return self._card("sp")

    def ac_freqs(self):
        """Frequency grid of the .AC card (numpy, Hz)."""
        return self._card_freqs("AC", self.ac, slice(0, 4))

    def noise_freqs(self):
        """Frequency grid of the .NOISE card (numpy, Hz)."""
        return self._card_freqs("NOISE", self.noise, slice(3, 7))

    def sp_freqs(self):
        """Frequency grid of the .SP card (numpy, Hz)."""
        return self._card_freqs("SP", self.sp, slice(0, 4))

    def disto_freqs(self):
        """Frequency grid of the .DISTO card (numpy, Hz)."""
        return self._card_freqs("DISTO", self.disto, slice(2, 6))

    def imd_freqs(self):
        """The tones of the .IMD card (Hz): (f1 numpy [F], the card's grid; f2 = f2overf1 * fstart)."""
        f1 = self._card_freqs("IMD", self.imd, slice(2, 6))
        return f1, self.imd[6] * self.imd[4]

    def stb_freqs(self):
        """Frequency grid of the .STB card (numpy, Hz)."""
        return self._card_freqs("STB", self.stb, slice(4, 8))

    def pac_freqs(self):
        """Frequency grid of the .PAC card (numpy, Hz)."""
        return self._card_freqs("PAC", self.pac, slice(0, 4))

    def pnoise_freqs(self):
        """Frequency grid of the .PNOISE card (numpy, Hz)."""
        return self._card_freqs("PNOISE", self.pnoise, slice(3, 7))

    @property
    def hb(self):
        """The .HB card: None, or (f0 in Hz, n_harm)."""
        en, f0, nh = C.c_int32(), C.c_double(), C.c_int32()
        capi.check(capi.lib().csim_netlist_hb(self._h, C.byref(en), C.byref(f0), C.byref(nh)))
        return (f0.value, nh.value) if en.value else None

    @property
    def pz(self):
        """The .PZ card: None, or (fmax in Hz, sigma0 in rad/s)."""
        en, fm, s0 = C.c_int32(), C.c_double(), C.c_double()
        capi.check(capi.lib().csim_netlist_pz(self._h, C.byref(en), C.byref(fm), C.byref(s0)))
        return (fm.value, s0.value) if en.value else None

    @property
    def noise_sources(self):
        """The noise generators in element order: [(element index, eq_a, eq_b)], -1 = ground."""
        L = capi.lib()
        out = []
        for i in range(L.csim_netlist_num_noise_sources(self._h)):
            e, a, b = C.c_int32(), C.c_int32(), C.c_int32()
            capi.check(L.csim_netlist_noise_source(self._h, i, C.byref(e), C.byref(a), C.byref(b)))
            out.append((e.value, a.value, b.value))
        return out

    @property
    def disto_devices(self):
        """The non-linear devices (MOSFETs) in element order: [(element index, eq_d, eq_g, eq_s)], -1 = ground."""
        L = capi.lib()
        out = []
        for i in range(L.csim_netlist_num_disto_devices(self._h)):
            e, d, g, s = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
            capi.check(L.csim_netlist_disto_device(self._h, i, C.byref(e), C.byref(d), C.byref(g), C.byref(s)))
            out.append((e.value, d.value, g.value, s.value))
        return out

    @property
    def ports(self):
        """The ports (V sources with PORTNUM k [Z0 r]) in port order: [(element index, branch equation, Z0)].
        Raises CsimError(CSIM_ERR_CONFIG) when the numbering has a gap or a duplicate or there are more than 4."""
        L = capi.lib()
        n = L.csim_netlist_num_ports(self._h)
        if n < 0:
            capi.check(n)
        out = []
        for i in range(n):
            e, k, z = C.c_int32(), C.c_int32(), C.c_double()
            capi.check(L.csim_netlist_port(self._h, i, C.byref(e), C.byref(k), C.byref(z)))
            out.append((e.value, k.value, z.value))
        return out

    @property
    def sp_noise(self):
        """True when the .SP card carries the trailing 1 (ngspice's donoise): two-port noise wanted with the sweep."""
        v = C.c_int32()
        capi.check(capi.lib().csim_netlist_sp_noise(self._h, C.byref(v)))
        return bool(v.value)

    def ac_source(self, elem):
        """(mag, phase_deg) of element elem's `AC mag [phase]` (0, 0 without one)."""
        m, p = C.c_double(), C.c_double()
        capi.check(capi.lib().csim_netlist_ac_source(self._h, int(elem), C.byref(m), C.byref(p)))
        return m.value, p.value

    @property
    def has_nonlinear(self):
        """any MOSFET -> Newton DC (csim_ir.has_nonlinear)"""
        ir = capi.lib().csim_netlist_ir(self._h)
        return bool(C.cast(ir, C.POINTER(C.c_int32))[5])

    def _n_params(self):
        # csim_ir: int32 n_unknowns, n_node_eq, n_branch_eq, n_elems, n_params, ...
        ir = capi.lib().csim_netlist_ir(self._h)
        return int(C.cast(ir, C.POINTER(C.c_int32))[4])

    @classmethod
    def from_file(cls, path):
        h = C.c_void_p()
        capi.check(capi.lib().csim_netlist_parse_file(str(path).encode(), C.byref(h)))
        return cls(h, source=str(path))

    @classmethod
    def from_text(cls, text):
        data = text.encode() if isinstance(text, str) else bytes(text)
        h = C.c_void_p()
        capi.check(capi.lib().csim_netlist_parse_text(data, len(data), C.byref(h)))
        return cls(h, source="<memory>")

    @property
    def handle(self):
        return self._h

    @property
    def ir_ptr(self):
        return C.c_void_p(capi.lib().csim_netlist_ir(self._h))

    def node_eq(self, name):
        return capi.lib().csim_netlist_node_eq(self._h, str(name).encode())

    def num_steps(self, tstep=None, tstop=None):
        return capi.lib().csim_tran_num_steps(self.tstep if tstep is None else tstep,
                                              self.tstop if tstop is None else tstop)

    def dc_sweeps(self):
        L = capi.lib()
        out = []
        for i in range(L.csim_netlist_num_dc_sweeps(self._h)):
            e, a, b, s = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
            capi.check(L.csim_netlist_dc_sweep(self._h, i, C.byref(e), C.byref(a), C.byref(b), C.byref(s)))
            out.append((e.value, a.value, b.value, s.value))
        return out

    def dc_sweep_table(self, i=0):
        """(.DC card i) -> (swept values [n], params [P][n]); every point is one DC instance."""
        L = capi.lib()
        n = L.csim_netlist_dc_sweep_points(self._h, i)
        params = np.zeros((self.n_params, n), dtype=np.float64)
        values = np.zeros(n, dtype=np.float64)
        if n > 0:
            capi.check(L.csim_netlist_dc_sweep_params(self._h, i, n, params.ctypes.data, values.ctypes.data))
        return values, params

    def mc_params_host(self, seed, sigma, b_first, B):
        """Host mirror of the device generator: numpy [P][B] (slot-major)."""
        out = np.zeros((self.n_params, B), dtype=np.float64)
        capi.check(capi.lib().csim_mc_params_host(self._h, seed, sigma, b_first, B, out.ctypes.data))
        return out

    def nominal_table(self, B):
        return np.repeat(self.nominal_params[:, None], B, axis=1).copy()

    def __del__(self):
        try:
            if self._h:
                capi.lib().csim_netlist_free(self._h)
                self._h = None
        except Exception:
            pass


def _torch():
    import torch
    return torch


class Engine:
    """One engine per (circuit, GPU).  Raises CsimError if no HIP device."""

    def __init__(self, netlist, device=0):
        self.netlist = netlist
        self.device = int(device)
        h = C.c_void_p()
        capi.check(capi.lib().csim_engine_create(netlist.handle, self.device, C.byref(h)))
        self._h = h
        self.N = netlist.n_unknowns
        self.P = netlist.n_params

    @property
    def tran_kernel(self):
        return capi.lib().csim_engine_tran_kernel(self._h).decode()

    @property
    def sched_info(self):
        """csim_engine_sched_info parsed: dict(text=..., ops=dict(fma, mul, addsub, recip, cmp)) or None"""
        text = capi.lib().csim_engine_sched_info(self._h).decode()
        if not text:
            return None
        ops = {}
        if "ops_per_solve:" in text:
            for item in text.split("ops_per_solve:")[1].split():
                k, _, v = item.partition("=")
                if v.isdigit():
                    ops[k] = int(v)
        return dict(text=text, ops=ops)

    def lanes_for_batch(self, B):
        """lanes per instance of the transient kernel for B instances: 1 / 16 (scheduled), 64 (general)"""
        n = capi.lib().csim_engine_lanes_for_batch(self._h, int(B))
        return n if n else 64

    def set_kernel(self, which):
        capi.check(capi.lib().csim_engine_set_kernel(self._h, {"auto": 0, "general": 1, "scheduled": 2, "faithful": 3}[which]))

    def set_option(self, key, value):
        """csim_engine_set_option: hybrid_rounds, hybrid_steps, lanes_per_instance, jit_dir, ... (include/csim.h)"""
        capi.check(capi.lib().csim_engine_set_option(self._h, str(key).encode(), str(value).encode()))

    def stat(self, key):
        """csim_engine_stat: "near_verified", "near_rolled_back", "ac_chunk" (include/csim.h)"""
        return int(capi.lib().csim_engine_stat(self._h, str(key).encode()))

    # -- device-pointer forms (torch tensors on cuda:<device>, slot-major) ----
    def _dev(self):
        return "cuda:%d" % self.device

    def _stream(self):
        torch = _torch()
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def upload_params(self, table):
        """numpy [P][B] -> device tensor"""
        torch = _torch()
        t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).to(self._dev())
        assert t.shape[0] == self.P
        return t

    def mc_params(self, seed, sigma, b_first, B):
        torch = _torch()
        out = torch.empty((self.P, B), dtype=torch.float64, device=self._dev())
        capi.check(capi.lib().csim_mc_params_dev(self._h, seed, sigma, b_first, B, out.data_ptr(), self._stream()))
        return out

    def dc(self, params):
        """params: device [P][B] -> (x [N][B], iters [B] int32, status [B] int32-bits)"""
        torch = _torch()
        B = params.shape[1]
        x = torch.empty((self.N, B), dtype=torch.float64, device=self._dev())
        it = torch.zeros(B, dtype=torch.int32, device=self._dev())
        st = torch.zeros(B, dtype=torch.int32, device=self._dev())
        capi.check(capi.lib().csim_dc_batch_dev(self._h, params.data_ptr(), B, x.data_ptr(), it.data_ptr(),
                                                st.data_ptr(), self._stream()))
        return x, it, st

    def dc_gs(self, params):
        """dcSolveGaussSeidel for a batch: params device [P][B] -> (x [N][B], iters, status)"""
        torch = _torch()
        B = params.shape[1]
        x = torch.empty((self.N, B), dtype=torch.float64, device=self._dev())
        it = torch.zeros(B, dtype=torch.int32, device=self._dev())
        st = torch.zeros(B, dtype=torch.int32, device=self._dev())
        capi.check(capi.lib().csim_dc_gs_batch_dev(self._h, params.data_ptr(), B, x.data_ptr(), it.data_ptr(),
                                                   st.data_ptr(), self._stream()))
        return x, it, st

    def dc_sweep(self, i=0):
        """Execute .DC card i of the netlist as one batch: -> (values, x [N][n], iters, status)."""
        values, table = self.netlist.dc_sweep_table(i)
        x, it, st = self.dc(self.upload_params(table))
        return values, x, it, st

    def tran(self, params, x, tstep, step_first, n_steps, iters, status, probes=None, out_stride=1,
             wave=None, step_iters=None):
        """Advance the batch by n_steps time steps in place (x, iters, status are updated)."""
        B = params.shape[1]
        n_probe = 0
        pe = None
        if wave is not None:
            pe = (C.c_int32 * len(probes))(*probes)
            n_probe = len(probes)
        capi.check(capi.lib().csim_tran_batch_dev(
            self._h, params.data_ptr(), B, float(tstep), int(step_first), int(n_steps), pe, n_probe,
            int(out_stride), wave.data_ptr() if wave is not None else None, x.data_ptr(), iters.data_ptr(),
            status.data_ptr(), step_iters.data_ptr() if step_iters is not None else None, self._stream()))

    def _ac_args(self, freqs, probes):
        f = self.netlist.ac_freqs() if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        pe = None if probes is None else (C.c_int32 * len(probes))(*probes)
        return f, pe, (self.N if probes is None else len(probes))

    def ac(self, params, x_op, freqs=None, probes=None, status=None):
        """AC sweep of the batch around the operating points x_op (device [N][B], from dc()).
        freqs: Hz (None = the .AC card); probes: equation indices (None = every unknown).
        -> (device complex128 [F][n_probe][B], status [B] int32, OR-ed into `status` when given)."""
        torch = _torch()
        B = params.shape[1]
        f, pe, n_probe = self._ac_args(freqs, probes)
        out = torch.zeros((len(f), n_probe, B, 2), dtype=torch.float64, device=self._dev())
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=self._dev())
        capi.check(capi.lib().csim_ac_batch_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), f.ctypes.data, len(f),
                                                pe, n_probe, out.data_ptr(), st.data_ptr(), self._stream()))
        return torch.view_as_complex(out), st

    def ac_system(self, params, x_op):
        """The linearised system per instance (csim_ac_system_dev): -> (G [B][N][N], C [B][N][N], J [B][N] complex),
        device tensors."""
        torch = _torch()
        B, N = params.shape[1], self.N
        sys = torch.empty((B, 2 * N * N + 2 * N), dtype=torch.float64, device=self._dev())
        capi.check(capi.lib().csim_ac_system_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), sys.data_ptr(),
                                                 self._stream()))
        G = sys[:, :N * N].reshape(B, N, N).transpose(1, 2)
        Cm = sys[:, N * N:2 * N * N].reshape(B, N, N).transpose(1, 2)
        J = torch.complex(sys[:, 2 * N * N:2 * N * N + N], sys[:, 2 * N * N + N:])
        return G, Cm, J

    # -- host-pointer forms (numpy, instance-major as in SURVEY.md 8b) --------
    def ac_host(self, params=None, B=1, freqs=None, probes=None):
        """DC operating point + AC sweep: -> (numpy complex128 [B][F][n_probe], status [B])."""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f, pe, n_probe = self._ac_args(freqs, probes)
        out = np.zeros((B, len(f), n_probe, 2))
        st = np.zeros(B, dtype=np.uint32)
        capi.check(capi.lib().csim_ac_batch(self._h, params.ctypes.data if params is not None else None, B,
                                            f.ctypes.data, len(f), pe, n_probe, out.ctypes.data, st.ctypes.data))
        return out[..., 0] + 1j * out[..., 1], st

    @staticmethod
    def _out_pair(out, card, card_name):
        """out: an equation, (out_p, out_m) or None = the card's (its first two entries) -> (out_p, out_m)"""
        if out is None:
            if card is None:
                raise capi.CsimError(capi.CSIM_ERR_CONFIG, "no output given and the netlist has no %s card" % card_name)
            return card[0], card[1]
        if isinstance(out, (tuple, list)):
            return int(out[0]), int(out[1])
        return int(out), -1

    def _noise_args(self, freqs, out, src):
        """-> (freqs, out_p, out_m, src_elem); None takes the .NOISE card's value (src: -1 without a card)"""
        card = self.netlist.noise
        if freqs is None:
            f = self.netlist.noise_freqs()
        else:
            f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        out_p, out_m = self._out_pair(out, card, ".NOISE")
        if src is None:
            src = card[2] if card is not None else -1
        return f, out_p, out_m, int(src)

    def noise(self, params, x_op, freqs=None, out=None, src=None, temp=300.15, contrib=False, psd=False, status=None):
        """Noise sweep of the batch around the operating points x_op (device [N][B], from dc()); csim_noise_batch_dev.
        freqs: Hz; out: equation or (out_p, out_m), -1 = ground; src: V/I element index for the gain, -1 = none --
        None takes each from the .NOISE card.  temp in kelvin.
        -> dict(freqs, onoise [F][B] V^2/Hz, gain complex [F][B] or None, contrib [F][S][B] or None,
                psd [S][B] or None, status [B]); device tensors; status is OR-ed into `status` when given."""
        torch = _torch()
        B = params.shape[1]
        f, out_p, out_m, src = self._noise_args(freqs, out, src)
        S = len(self.netlist.noise_sources)
        dev = self._dev()
        on = torch.zeros((len(f), B), dtype=torch.float64, device=dev)
        g = torch.zeros((len(f), B, 2), dtype=torch.float64, device=dev) if src >= 0 else None
        con = torch.zeros((len(f), S, B), dtype=torch.float64, device=dev) if contrib else None
        ps = torch.zeros((S, B), dtype=torch.float64, device=dev) if psd else None
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
        capi.check(capi.lib().csim_noise_batch_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), f.ctypes.data, len(f),
                                                   out_p, out_m, src, float(temp), on.data_ptr(), ptr(g), ptr(con),
                                                   ptr(ps), st.data_ptr(), self._stream()))
        return dict(freqs=f, onoise=on, gain=torch.view_as_complex(g) if g is not None else None, contrib=con, psd=ps,
                    status=st)

    def noise_host(self, params=None, B=1, freqs=None, out=None, src=None, temp=300.15, contrib=False, psd=False):
        """DC operating point + noise sweep (csim_noise_batch): numpy, instance-major.
        -> dict(freqs, onoise [B][F], gain complex [B][F] or None, contrib [B][F][S] or None, psd [B][S] or None,
                status [B])"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f, out_p, out_m, src = self._noise_args(freqs, out, src)
        S = len(self.netlist.noise_sources)
        on = np.zeros((B, len(f)))
        g = np.zeros((B, len(f), 2)) if src >= 0 else None
        con = np.zeros((B, len(f), S)) if contrib else None
        ps = np.zeros((B, S)) if psd else None
        st = np.zeros(B, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None else None    # noqa: E731
        capi.check(capi.lib().csim_noise_batch(self._h, ptr(params), B, f.ctypes.data, len(f), out_p, out_m, src,
                                               float(temp), on.ctypes.data, ptr(g), ptr(con), ptr(ps), st.ctypes.data))
        return dict(freqs=f, onoise=on, gain=g[..., 0] + 1j * g[..., 1] if g is not None else None, contrib=con, psd=ps,
                    status=st)

    def _disto_args(self, freqs, out):
        """-> (freqs, out_p, out_m); None takes the .DISTO card's value"""
        card = self.netlist.disto
        if freqs is None:
            f = self.netlist.disto_freqs()
        else:
            f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        return (f,) + self._out_pair(out, card, ".DISTO")

    def disto(self, params, x_op, freqs=None, out=None, want_h=True, coef=False, status=None):
        """Single-tone distortion sweep of the batch around the operating points x_op (device [N][B], from dc());
        csim_disto_batch_dev.  freqs: Hz; out: equation or (out_p, out_m), -1 = ground -- None takes each from the
        .DISTO card.
        -> dict(freqs, h complex [F][3][N][B] (x1, x2, x3) or None, hd [F][2][B] (HD2, HD3), coef [M][7][B] or None,
                status [B]); device tensors; status is OR-ed into `status` when given."""
        torch = _torch()
        B = params.shape[1]
        f, out_p, out_m = self._disto_args(freqs, out)
        M = len(self.netlist.disto_devices)
        dev = self._dev()
        h = torch.zeros((len(f), 3, self.N, B, 2), dtype=torch.float64, device=dev) if want_h else None
        hd = torch.zeros((len(f), 2, B), dtype=torch.float64, device=dev)
        cf = torch.zeros((M, 7, B), dtype=torch.float64, device=dev) if coef else None
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
        capi.check(capi.lib().csim_disto_batch_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), f.ctypes.data, len(f),
                                                   out_p, out_m, ptr(h), hd.data_ptr(), ptr(cf), st.data_ptr(),
                                                   self._stream()))
        return dict(freqs=f, h=torch.view_as_complex(h) if h is not None else None, hd=hd, coef=cf, status=st)

    def disto_host(self, params=None, B=1, freqs=None, out=None, want_h=True, coef=False):
        """DC operating point + distortion sweep (csim_disto_batch): numpy, instance-major.
        -> dict(freqs, h complex [B][F][3][N] or None, hd [B][F][2], coef [B][M][7] or None, status [B])"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f, out_p, out_m = self._disto_args(freqs, out)
        M = len(self.netlist.disto_devices)
        h = np.zeros((B, len(f), 3, self.N), dtype=np.complex128) if want_h else None
        hd = np.zeros((B, len(f), 2))
        cf = np.zeros((B, M, 7)) if coef else None
        st = np.zeros(B, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None else None    # noqa: E731
        capi.check(capi.lib().csim_disto_batch(self._h, ptr(params), B, f.ctypes.data, len(f), out_p, out_m, ptr(h),
                                               hd.ctypes.data, ptr(cf), st.ctypes.data))
        return dict(freqs=f, h=h, hd=hd, coef=cf, status=st)

    def _imd_args(self, freqs, f2, out):
        """-> (f1, f2, out_p, out_m); freqs None takes both tones from the .IMD card, out None its output"""
        card = self.netlist.imd
        if freqs is None:
            f, card_f2 = self.netlist.imd_freqs()
            f2 = card_f2 if f2 is None else f2
        else:
            f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
            if f2 is None:
                raise capi.CsimError(capi.CSIM_ERR_CONFIG, "imd: freqs given without f2")
        return (f, float(f2)) + self._out_pair(out, card, ".IMD")

    def imd(self, params, x_op, freqs=None, f2=None, out=None, want_h=True, coef=False, status=None):
        """Two-tone intermodulation sweep of the batch around the operating points x_op (device [N][B], from dc());
        csim_imd_batch_dev.  freqs: the first tone, Hz; f2: the second tone, Hz; out: equation or (out_p, out_m), -1 =
        ground -- None takes each from the .IMD card.
        -> dict(freqs, f2, h complex [F][6][N][B] (the solutions at f1, f2, f1 + f2, f1 - f2, 2 f1, 2 f1 - f2) or None,
                im [F][3][B] (IM2+, IM2-, IM3), coef [M][7][B] or None, status [B]); device tensors; status is OR-ed
                into `status` when given."""
        torch = _torch()
        B = params.shape[1]
        f, f2, out_p, out_m = self._imd_args(freqs, f2, out)
        M = len(self.netlist.disto_devices)
        dev = self._dev()
        h = torch.zeros((len(f), 6, self.N, B, 2), dtype=torch.float64, device=dev) if want_h else None
        im = torch.zeros((len(f), 3, B), dtype=torch.float64, device=dev)
        cf = torch.zeros((M, 7, B), dtype=torch.float64, device=dev) if coef else None
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
        capi.check(capi.lib().csim_imd_batch_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), f.ctypes.data, len(f), f2,
                                                 out_p, out_m, ptr(h), im.data_ptr(), ptr(cf), st.data_ptr(),
                                                 self._stream()))
        return dict(freqs=f, f2=f2, h=torch.view_as_complex(h) if h is not None else None, im=im, coef=cf, status=st)

    def imd_host(self, params=None, B=1, freqs=None, f2=None, out=None, want_h=True, coef=False):
        """DC operating point + intermodulation sweep (csim_imd_batch): numpy, instance-major.
        -> dict(freqs, f2, h complex [B][F][6][N] or None, im [B][F][3], coef [B][M][7] or None, status [B])"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f, f2, out_p, out_m = self._imd_args(freqs, f2, out)
        M = len(self.netlist.disto_devices)
        h = np.zeros((B, len(f), 6, self.N), dtype=np.complex128) if want_h else None
        im = np.zeros((B, len(f), 3))
        cf = np.zeros((B, M, 7)) if coef else None
        st = np.zeros(B, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None else None    # noqa: E731
        capi.check(capi.lib().csim_imd_batch(self._h, ptr(params), B, f.ctypes.data, len(f), f2, out_p, out_m, ptr(h),
                                             im.ctypes.data, ptr(cf), st.ctypes.data))
        return dict(freqs=f, f2=f2, h=h, im=im, coef=cf, status=st)

    def _stb_args(self, freqs, probe):
        """-> (freqs, probe element); None takes the .STB card's value (-1 tells the library to)"""
        f = self.netlist.stb_freqs() if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        return f, -1 if probe is None else int(probe)

    @staticmethod
    def _stb_dict(f, t, x, mg, fd, st, axis):
        """margins [4][B] (axis 0) or [B][4] (axis 1) -> the four named entries"""
        if mg is None:
            pm = fc = gm = f180 = None
        else:
            pm, fc, gm, f180 = (mg[i] if axis == 0 else np.ascontiguousarray(mg[:, i]) for i in range(4))
        return dict(freqs=f, t=t, x=x, pm=pm, fc=fc, gm=gm, f180=f180, found=fd, status=st)

    def stb(self, params, x_op, freqs=None, probe=None, margins=True, want_x=False, status=None):
        """Loop-gain sweep of the batch around the operating points x_op (device [N][B], from dc()); csim_stb_batch_dev.
        freqs: Hz; probe: element index of a V source in series in the loop, + on the driving side -- None takes each
        from the .STB card.  margins need strictly increasing positive frequencies.
        -> dict(freqs, t complex [F][B], x complex [F][2][N][B] or None, pm (degrees), fc (Hz), gm (dB), f180 (Hz) [B]
                (NaN where not found) and found [B] (bit 0 unity, bit 1 phase crossing) or None, status [B]); device
                tensors; status is OR-ed into `status` when given."""
        torch = _torch()
        B = params.shape[1]
        f, probe = self._stb_args(freqs, probe)
        dev = self._dev()
        t = torch.zeros((len(f), B, 2), dtype=torch.float64, device=dev)
        x = torch.zeros((len(f), 2, self.N, B, 2), dtype=torch.float64, device=dev) if want_x else None
        mg = torch.zeros((4, B), dtype=torch.float64, device=dev) if margins else None
        fd = torch.zeros(B, dtype=torch.int32, device=dev) if margins else None
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        ptr = lambda v: v.data_ptr() if v is not None else None     # noqa: E731
        capi.check(capi.lib().csim_stb_batch_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), f.ctypes.data, len(f), probe,
                                                 t.data_ptr(), ptr(x), ptr(mg), ptr(fd), st.data_ptr(), self._stream()))
        return self._stb_dict(f, torch.view_as_complex(t), torch.view_as_complex(x) if x is not None else None, mg, fd, st, 0)

    def stb_host(self, params=None, B=1, freqs=None, probe=None, margins=True, want_x=False):
        """DC operating point + loop-gain sweep (csim_stb_batch): numpy, instance-major.
        -> dict(freqs, t complex [B][F], x complex [B][F][2][N] or None, pm, fc, gm, f180, found [B] or None, status [B])"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f, probe = self._stb_args(freqs, probe)
        t = np.zeros((B, len(f)), dtype=np.complex128)
        x = np.zeros((B, len(f), 2, self.N), dtype=np.complex128) if want_x else None
        mg = np.zeros((B, 4)) if margins else None
        fd = np.zeros(B, dtype=np.int32) if margins else None
        st = np.zeros(B, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None else None    # noqa: E731
        capi.check(capi.lib().csim_stb_batch(self._h, ptr(params), B, f.ctypes.data, len(f), probe, t.ctypes.data, ptr(x),
                                             ptr(mg), ptr(fd), st.ctypes.data))
        return self._stb_dict(f, t, x, mg, fd, st, 1)

    @staticmethod
    def _pz_args(fmax, sigma0):
        """None for fmax takes both from the .PZ card (NaN tells the library to)"""
        if fmax is None:
            return float("nan"), 0.0
        return float(fmax), 0.0 if sigma0 is None else float(sigma0)

    def pz(self, params, x_op, fmax=None, sigma0=None, status=None):
        """Poles of the batch's linearisations around the operating points x_op (device [N][B], from dc());
        csim_pz_batch_dev.  fmax: Hz, eigenvalues slower than 1 / (2 pi fmax) are poles at infinity; sigma0: rad/s,
        the shift of G + sigma0 C (default 0) -- fmax None takes both from the .PZ card.
        -> dict(poles complex [N][B] (slot k of instance b: dominant first, NaN beyond n_poles), n_poles, n_rhp int32
                [B], max_re [B], status [B]); device tensors; status is OR-ed into `status` when given."""
        torch = _torch()
        B = params.shape[1]
        fmax, sigma0 = self._pz_args(fmax, sigma0)
        dev = self._dev()
        poles = torch.zeros((self.N, B, 2), dtype=torch.float64, device=dev)
        n_poles = torch.zeros(B, dtype=torch.int32, device=dev)
        n_rhp = torch.zeros(B, dtype=torch.int32, device=dev)
        max_re = torch.zeros(B, dtype=torch.float64, device=dev)
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        capi.check(capi.lib().csim_pz_batch_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), fmax, sigma0, poles.data_ptr(),
                                                n_poles.data_ptr(), n_rhp.data_ptr(), max_re.data_ptr(), st.data_ptr(),
                                                self._stream()))
        return dict(poles=torch.view_as_complex(poles), n_poles=n_poles, n_rhp=n_rhp, max_re=max_re, status=st)

    def pz_host(self, params=None, B=1, fmax=None, sigma0=None):
        """DC operating point + poles (csim_pz_batch): numpy, instance-major.
        -> dict(poles complex [B][N], n_poles, n_rhp [B], max_re [B], status [B])"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        fmax, sigma0 = self._pz_args(fmax, sigma0)
        poles = np.zeros((B, self.N), dtype=np.complex128)
        n_poles = np.zeros(B, dtype=np.int32)
        n_rhp = np.zeros(B, dtype=np.int32)
        max_re = np.zeros(B)
        st = np.zeros(B, dtype=np.uint32)
        capi.check(capi.lib().csim_pz_batch(self._h, params.ctypes.data if params is not None else None, B, fmax, sigma0,
                                            poles.ctypes.data, n_poles.ctypes.data, n_rhp.ctypes.data, max_re.ctypes.data,
                                            st.ctypes.data))
        return dict(poles=poles, n_poles=n_poles, n_rhp=n_rhp, max_re=max_re, status=st)

    def _pss_args(self, tstep, f0, n_harm, probes, tol, max_rounds):
        """-> (tstep, f0, n_harm, probe array or None, n_probe, tol, max_rounds) with the cards' values filled in, so the
        output shapes are known (a non-positive tstep or f0 means the card, as in the C entry: the library would
        otherwise take the card's harmonic count after the outputs are sized); 0 asks the library for an engine option"""
        if f0 is not None and not float(f0) > 0.0 and np.isfinite(float(f0)):
            f0, n_harm = None, None
        if tstep is not None and not float(tstep) > 0.0 and np.isfinite(float(tstep)):
            tstep = None
        if f0 is None:
            card = self.netlist.hb
            if card is None:
                raise capi.CsimError(capi.CSIM_ERR_CONFIG, "no f0 given and the netlist has no .HB card")
            f0 = card[0]
            n_harm = card[1] if n_harm is None else n_harm
        if n_harm is None:
            n_harm = 0
        if tstep is None:
            if not self.netlist.tran_enabled:
                raise capi.CsimError(capi.CSIM_ERR_CONFIG, "no tstep given and the netlist has no .TRAN card")
            tstep = self.netlist.tstep
        pe = None if probes is None else (C.c_int32 * len(probes))(*probes)
        return (float(tstep), float(f0), int(n_harm), pe, self.N if probes is None else len(probes),
                0.0 if tol is None else float(tol), 0 if max_rounds is None else int(max_rounds))

    def pss(self, params, x0, tstep=None, f0=None, n_harm=None, probes=None, tol=None, max_rounds=None, status=None):
        """Periodic steady state of the batch by shooting Newton (csim_pss_batch_dev), started at x0 (device [N][B],
        normally dc()'s; not modified).  tstep None = the .TRAN card's step; f0 None = the .HB card (n_harm too);
        probes: equation indices (None = every unknown); tol, max_rounds None = the engine options.
        -> dict(x0 [N][B], harm complex [n_harm+1][n_probe][B] (peak phasors, cosine reference), rounds [B],
                status [B], K); device tensors; status is OR-ed into `status` when given.  The call waits on the stream."""
        torch = _torch()
        B = params.shape[1]
        tstep, f0, n_harm, pe, n_probe, tol, max_rounds = self._pss_args(tstep, f0, n_harm, probes, tol, max_rounds)
        dev = self._dev()
        x = x0.clone().contiguous()
        harm = torch.zeros((max(n_harm, 0) + 1, n_probe, B, 2), dtype=torch.float64, device=dev)
        rounds = torch.zeros(B, dtype=torch.int32, device=dev)
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        capi.check(capi.lib().csim_pss_batch_dev(self._h, params.data_ptr(), B, tstep, f0, n_harm, pe, n_probe, tol,
                                                 max_rounds, x.data_ptr(), harm.data_ptr(), rounds.data_ptr(),
                                                 st.data_ptr(), self._stream()))
        K = int(capi.lib().csim_pss_num_steps(tstep, f0))
        return dict(x0=x, harm=torch.view_as_complex(harm), rounds=rounds, status=st, K=K)

    def pss_host(self, params=None, B=1, tstep=None, f0=None, n_harm=None, probes=None, tol=None, max_rounds=None):
        """DC operating point + periodic steady state (csim_pss_batch): numpy, instance-major.
        -> dict(x0 [B][N], harm complex [B][n_harm+1][n_probe], rounds [B], status [B], K)"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        tstep, f0, n_harm, pe, n_probe, tol, max_rounds = self._pss_args(tstep, f0, n_harm, probes, tol, max_rounds)
        x = np.zeros((B, self.N))
        harm = np.zeros((B, max(n_harm, 0) + 1, n_probe), dtype=np.complex128)
        rounds = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.uint32)
        capi.check(capi.lib().csim_pss_batch(self._h, params.ctypes.data if params is not None else None, B, tstep, f0,
                                             n_harm, pe, n_probe, tol, max_rounds, x.ctypes.data, harm.ctypes.data,
                                             rounds.ctypes.data, st.ctypes.data))
        return dict(x0=x, harm=harm, rounds=rounds, status=st, K=int(capi.lib().csim_pss_num_steps(tstep, f0)))

    def _pac_args(self, freqs, n_side, tstep, f0, probes):
        """-> (freqs, n_side, tstep, f0, probe array or None, n_probe) with the cards' values filled in, so the output
        shapes are known; a non-positive tstep or f0 means the card, as in the C entry"""
        tstep, f0, _, pe, n_probe, _, _ = self._pss_args(tstep, f0, 0, probes, None, None)
        card = self.netlist.pac
        if freqs is None:
            if card is None:
                raise capi.CsimError(capi.CSIM_ERR_ARG, "no frequencies given and the netlist has no .PAC card")
            freqs = self.netlist.pac_freqs()
        f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        if n_side is None:
            n_side = card[4] if card is not None else 1
        return f, int(n_side), tstep, f0, pe, n_probe

    def pac(self, params, x0, freqs=None, n_side=None, tstep=None, f0=None, probes=None, status=None):
        """Periodic AC analysis of the batch around the orbit that starts at x0 (device [N][B], normally pss()["x0"]; not
        modified): csim_pac_batch_dev.  freqs: input frequencies in Hz, None = the .PAC card; n_side None = the card's
        (1 without one); tstep None = the .TRAN card's step; f0 None = the .HB card's; probes: equation indices
        (None = every unknown).
        -> dict(freqs, p complex [F][2 n_side + 1][n_probe][B] (the transfer from the AC sources to the sideband
                f + m f0 at index m + n_side), status [B], K, n_side); device tensors; status is OR-ed into `status` when
        given.  The call waits on the stream."""
        torch = _torch()
        B = params.shape[1]
        f, n_side, tstep, f0, pe, n_probe = self._pac_args(freqs, n_side, tstep, f0, probes)
        dev = self._dev()
        x = x0.contiguous()
        out = torch.zeros((len(f), 2 * max(n_side, 0) + 1, n_probe, B, 2), dtype=torch.float64, device=dev)
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        capi.check(capi.lib().csim_pac_batch_dev(self._h, params.data_ptr(), B, tstep, f0, x.data_ptr(), f.ctypes.data, len(f),
                                                 n_side, pe, n_probe, out.data_ptr(), st.data_ptr(), self._stream()))
        return dict(freqs=f, p=torch.view_as_complex(out), status=st, K=int(capi.lib().csim_pss_num_steps(tstep, f0)),
                    n_side=n_side)

    def pac_host(self, params=None, B=1, freqs=None, n_side=None, tstep=None, f0=None, probes=None):
        """DC operating point + periodic steady state + periodic AC analysis (csim_pac_batch): numpy, instance-major.
        -> dict(freqs, p complex [B][F][2 n_side + 1][n_probe], x0 [B][N], rounds [B], status [B], K, n_side)"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f, n_side, tstep, f0, pe, n_probe = self._pac_args(freqs, n_side, tstep, f0, probes)
        out = np.zeros((B, len(f), 2 * max(n_side, 0) + 1, n_probe), dtype=np.complex128)
        x = np.zeros((B, self.N))
        rounds = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.uint32)
        capi.check(capi.lib().csim_pac_batch(self._h, params.ctypes.data if params is not None else None, B, tstep, f0,
                                             f.ctypes.data, len(f), n_side, pe, n_probe, out.ctypes.data, x.ctypes.data,
                                             rounds.ctypes.data, st.ctypes.data))
        return dict(freqs=f, p=out, x0=x, rounds=rounds, status=st, K=int(capi.lib().csim_pss_num_steps(tstep, f0)),
                    n_side=n_side)

    def _pnoise_args(self, freqs, n_side, tstep, f0, out, src):
        """-> (freqs, n_side, tstep, f0, out_p, out_m, src_elem): None takes the cards' values (.PNOISE for the grid,
        n_side, output and source; .TRAN and .HB for tstep and f0), so the output shapes are known"""
        tstep, f0, _, _, _, _, _ = self._pss_args(tstep, f0, 0, None, None, None)
        card = self.netlist.pnoise
        if freqs is None:
            if card is None:
                raise capi.CsimError(capi.CSIM_ERR_ARG, "no frequencies given and the netlist has no .PNOISE card")
            freqs = self.netlist.pnoise_freqs()
        f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        if n_side is None:
            n_side = card[7] if card is not None else 1
        out_p, out_m = self._out_pair(out, card, ".PNOISE")
        if src is None:
            src = card[2] if card is not None else -1
        return f, int(n_side), tstep, f0, out_p, out_m, int(src)

    def pnoise(self, params, x0, freqs=None, n_side=None, tstep=None, f0=None, out=None, src=None, temp=300.15,
               contrib=False, side=False, status=None):
        """Periodic noise analysis of the batch around the orbit that starts at x0 (device [N][B], normally pss()["x0"];
        not modified): csim_pnoise_batch_dev.  freqs: output frequencies in Hz; out: equation or (out_p, out_m), -1 =
        ground; src: V/I element index for the conversion gains, -1 = none; n_side -- None takes each from the .PNOISE
        card (n_side 1 and src -1 without one); tstep None = the .TRAN card's step; f0 None = the .HB card's; temp in kelvin.
        -> dict(freqs, onoise [F][B] V^2/Hz, gain complex [F][2 n_side + 1][B] or None (from f + m f0 at the source to
                the output at f, index m + n_side), contrib [F][S][B] or None, side [F][2 n_side + 1][B] or None,
                status [B], K, n_side); device tensors; status is OR-ed into `status` when given.  The call waits on the
        stream."""
        torch = _torch()
        B = params.shape[1]
        f, n_side, tstep, f0, out_p, out_m, src = self._pnoise_args(freqs, n_side, tstep, f0, out, src)
        S = len(self.netlist.noise_sources)
        nsb = 2 * max(n_side, 0) + 1
        dev = self._dev()
        x = x0.contiguous()
        on = torch.zeros((len(f), B), dtype=torch.float64, device=dev)
        g = torch.zeros((len(f), nsb, B, 2), dtype=torch.float64, device=dev) if src >= 0 else None
        con = torch.zeros((len(f), S, B), dtype=torch.float64, device=dev) if contrib else None
        sd = torch.zeros((len(f), nsb, B), dtype=torch.float64, device=dev) if side else None
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
        capi.check(capi.lib().csim_pnoise_batch_dev(self._h, params.data_ptr(), B, tstep, f0, x.data_ptr(), f.ctypes.data,
                                                    len(f), n_side, out_p, out_m, src, float(temp), on.data_ptr(), ptr(g),
                                                    ptr(con), ptr(sd), st.data_ptr(), self._stream()))
        return dict(freqs=f, onoise=on, gain=torch.view_as_complex(g) if g is not None else None, contrib=con, side=sd,
                    status=st, K=int(capi.lib().csim_pss_num_steps(tstep, f0)), n_side=n_side)

    def pnoise_host(self, params=None, B=1, freqs=None, n_side=None, tstep=None, f0=None, out=None, src=None, temp=300.15,
                    contrib=False, side=False):
        """DC operating point + periodic steady state + periodic noise analysis (csim_pnoise_batch): numpy,
        instance-major.
        -> dict(freqs, onoise [B][F], gain complex [B][F][2 n_side + 1] or None, contrib [B][F][S] or None,
                side [B][F][2 n_side + 1] or None, x0 [B][N], rounds [B], status [B], K, n_side)"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f, n_side, tstep, f0, out_p, out_m, src = self._pnoise_args(freqs, n_side, tstep, f0, out, src)
        S = len(self.netlist.noise_sources)
        nsb = 2 * max(n_side, 0) + 1
        on = np.zeros((B, len(f)))
        g = np.zeros((B, len(f), nsb, 2)) if src >= 0 else None
        con = np.zeros((B, len(f), S)) if contrib else None
        sd = np.zeros((B, len(f), nsb)) if side else None
        x = np.zeros((B, self.N))
        rounds = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None else None    # noqa: E731
        capi.check(capi.lib().csim_pnoise_batch(self._h, ptr(params), B, tstep, f0, f.ctypes.data, len(f), n_side, out_p,
                                                out_m, src, float(temp), on.ctypes.data, ptr(g), ptr(con), ptr(sd),
                                                x.ctypes.data, rounds.ctypes.data, st.ctypes.data))
        return dict(freqs=f, onoise=on, gain=g[..., 0] + 1j * g[..., 1] if g is not None else None, contrib=con, side=sd,
                    x0=x, rounds=rounds, status=st, K=int(capi.lib().csim_pss_num_steps(tstep, f0)), n_side=n_side)

    def sp(self, params, x_op, freqs=None, want_s=True, status=None):
        """S-parameter sweep of the batch around the operating points x_op (device [N][B], from dc());
        csim_sp_batch_dev.  freqs: Hz, None = the .SP card.
        -> dict(freqs, y complex [F][P][P][B], s the same or None, status [B]); device tensors; status is OR-ed into
        `status` when given."""
        torch = _torch()
        B = params.shape[1]
        f = self.netlist.sp_freqs() if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        P = len(self.netlist.ports)
        dev = self._dev()
        y = torch.zeros((len(f), P, P, B, 2), dtype=torch.float64, device=dev)
        s = torch.zeros((len(f), P, P, B, 2), dtype=torch.float64, device=dev) if want_s else None
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        capi.check(capi.lib().csim_sp_batch_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), f.ctypes.data, len(f),
                                                y.data_ptr(), s.data_ptr() if s is not None else None, st.data_ptr(),
                                                self._stream()))
        return dict(freqs=f, y=torch.view_as_complex(y), s=torch.view_as_complex(s) if s is not None else None, status=st)

    def sp_host(self, params=None, B=1, freqs=None, want_s=True):
        """DC operating point + S-parameter sweep (csim_sp_batch): numpy, instance-major.
        -> dict(freqs, y complex [B][F][P][P], s the same or None, status [B])"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f = self.netlist.sp_freqs() if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        P = len(self.netlist.ports)
        y = np.zeros((B, len(f), P, P), dtype=np.complex128)
        s = np.zeros((B, len(f), P, P), dtype=np.complex128) if want_s else None
        st = np.zeros(B, dtype=np.uint32)
        capi.check(capi.lib().csim_sp_batch(self._h, params.ctypes.data if params is not None else None, B, f.ctypes.data,
                                            len(f), y.ctypes.data, s.ctypes.data if s is not None else None,
                                            st.ctypes.data))
        return dict(freqs=f, y=y, s=s, status=st)

    def sp_noise(self, params, x_op, freqs=None, temp=300.15, status=None, noise_params=None):
        """Two-port noise sweep of the batch around the operating points x_op (device [N][B], from dc());
        csim_spnoise_batch_dev.  freqs: Hz, None = the .SP card; temp in kelvin (the generators' temperature; NF is
        referred to 290 K).  noise_params: None = for two ports; True with any other port count is a ValueError.
        -> dict(freqs, y, cy complex [F][P][P][B], status [B]) and, for two ports, nf, fmin, rn [F][B] (linear) and
        yopt complex [F][B]; device tensors; status is OR-ed into `status` when given."""
        torch = _torch()
        B = params.shape[1]
        f = self.netlist.sp_freqs() if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        P = len(self.netlist.ports)
        if noise_params and P != 2:
            raise ValueError("NF, Fmin, Rn and Yopt exist for two ports only (the netlist has %d)" % P)
        two = P == 2 if noise_params is None else bool(noise_params)
        dev = self._dev()
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)     # noqa: E731
        y, cy = z(len(f), P, P, B, 2), z(len(f), P, P, B, 2)
        nf, fmin, rn, yopt = (z(len(f), B), z(len(f), B), z(len(f), B), z(len(f), B, 2)) if two else (None,) * 4
        st = status if status is not None else torch.zeros(B, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
        capi.check(capi.lib().csim_spnoise_batch_dev(self._h, params.data_ptr(), B, x_op.data_ptr(), f.ctypes.data, len(f),
                                                     float(temp), y.data_ptr(), cy.data_ptr(), ptr(nf), ptr(fmin), ptr(rn),
                                                     ptr(yopt), st.data_ptr(), self._stream()))
        r = dict(freqs=f, y=torch.view_as_complex(y), cy=torch.view_as_complex(cy), status=st)
        if two:
            r.update(nf=nf, fmin=fmin, rn=rn, yopt=torch.view_as_complex(yopt))
        return r

    def sp_noise_host(self, params=None, B=1, freqs=None, temp=300.15, noise_params=None):
        """DC operating point + two-port noise sweep (csim_spnoise_batch): numpy, instance-major.
        -> dict(freqs, y, cy complex [B][F][P][P], status [B]) and, for two ports, nf, fmin, rn [B][F], yopt complex
        [B][F]"""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        f = self.netlist.sp_freqs() if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        P = len(self.netlist.ports)
        if noise_params and P != 2:
            raise ValueError("NF, Fmin, Rn and Yopt exist for two ports only (the netlist has %d)" % P)
        two = P == 2 if noise_params is None else bool(noise_params)
        y = np.zeros((B, len(f), P, P), dtype=np.complex128)
        cy = np.zeros((B, len(f), P, P), dtype=np.complex128)
        nf, fmin, rn = (np.zeros((B, len(f))) for _ in range(3)) if two else (None,) * 3
        yopt = np.zeros((B, len(f)), dtype=np.complex128) if two else None
        st = np.zeros(B, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None else None    # noqa: E731
        capi.check(capi.lib().csim_spnoise_batch(self._h, ptr(params), B, f.ctypes.data, len(f), float(temp), y.ctypes.data,
                                                 cy.ctypes.data, ptr(nf), ptr(fmin), ptr(rn), ptr(yopt), st.ctypes.data))
        r = dict(freqs=f, y=y, cy=cy, status=st)
        if two:
            r.update(nf=nf, fmin=fmin, rn=rn, yopt=yopt)
        return r

    def dc_host(self, params=None, B=1):
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        x = np.zeros((B, self.N))
        it = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.uint32)
        capi.check(capi.lib().csim_dc_batch(self._h, params.ctypes.data if params is not None else None, B,
                                            x.ctypes.data, it.ctypes.data, st.ctypes.data))
        return x, it, st

    def tran_host(self, params=None, B=1, tstep=None, tstop=None, tstart=None, probes=None, out_stride=1):
        nl = self.netlist
        tstep = nl.tstep if tstep is None else tstep
        tstop = nl.tstop if tstop is None else tstop
        tstart = nl.tstart if tstart is None else tstart
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        wave = None
        pe = None
        n_probe = 0
        if probes is not None:
            n_probe = len(probes)
            pe = (C.c_int32 * n_probe)(*probes)
            rows = capi.lib().csim_tran_num_rows(tstep, tstop, tstart, out_stride)
            wave = np.zeros((B, rows, n_probe))
        xf = np.zeros((B, self.N))
        it = np.zeros(B, dtype=np.int64)
        st = np.zeros(B, dtype=np.uint32)
        capi.check(capi.lib().csim_tran_batch(
            self._h, params.ctypes.data if params is not None else None, B, tstep, tstop, tstart, pe, n_probe,
            out_stride, wave.ctypes.data if wave is not None else None, xf.ctypes.data, it.ctypes.data,
            st.ctypes.data))
        return wave, xf, it, st

    def write_csv(self, path, params=None, instance=0, tstep=None, tstop=None, tstart=None, probes=None):
        """csim_tran_write_csv: the transient of one instance of params ([B][P] numpy, instance-major; None = nominal)
        as the reference's CSV.  probes None: the netlist's .PLOTNV/.PRINT probes if any, else every unknown."""
        nl = self.netlist
        tstep = nl.tstep if tstep is None else tstep
        tstop = nl.tstop if tstop is None else tstop
        tstart = nl.tstart if tstart is None else tstart
        B = 1
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            B = params.shape[0]
        pe, n_probe = None, 0
        if probes:
            n_probe = len(probes)
            pe = (C.c_int32 * n_probe)(*probes)
        capi.check(capi.lib().csim_tran_write_csv(
            self._h, params.ctypes.data if params is not None else None, B, int(instance), tstep, tstop, tstart,
            pe, n_probe, str(path).encode()))

    def jit_scheduled(self, params, tstep=None, plan_steps=200):
        """Plan + generate + hipcc + load the lane-per-instance kernel for this netlist (needs hipcc)."""
        tstep = self.netlist.tstep if tstep is None else tstep
        capi.check(capi.lib().csim_engine_jit_scheduled(self._h, params.data_ptr(), params.shape[1], float(tstep),
                                                        int(plan_steps)))

    @staticmethod
    def _positions(schedules, N):
        """["0:21,8:22", "-", ...] -> int32 [n][N] pivot row positions"""
        pos = np.tile(np.arange(N, dtype=np.int32), (len(schedules), 1))
        for a, text in enumerate(schedules):
            for item in text.replace("-", "").split(","):
                if item.strip():
                    k, p = item.split(":")
                    pos[a, int(k)] = int(p)
        return np.ascontiguousarray(pos)

    def jit_with_schedules(self, schedules, dc_schedules=()):
        """Generate + hipcc + load the kernels for explicit pivot schedules ("k:p,k:p" strings as
        returned by record_pivot_schedules / record_dc_pivot_schedules)."""
        pos = self._positions(list(schedules), self.N)
        dpos = self._positions(list(dc_schedules), self.N) if len(dc_schedules) else None
        capi.check(capi.lib().csim_engine_jit_with_schedules(
            self._h, pos.ctypes.data, pos.shape[0], dpos.ctypes.data if dpos is not None else None,
            dpos.shape[0] if dpos is not None else 0))

    @staticmethod
    def _schedules_in(info_text):
        """(transient, dc) schedule strings out of a csim_sched_info text"""
        if not info_text or "schedule=" not in info_text:
            return [], []
        body = info_text.split("schedule=", 1)[1].split(" lds_doubles", 1)[0]
        tran, dc = [], []
        for item in body.split(";"):
            item = item.strip()
            if not item:
                continue
            if item.startswith("dc "):
                dc.append(item[3:].strip())
            else:
                tran.append(item)
        return tran, dc

    def loaded_schedules(self):
        """(transient, dc) schedule strings of the generated library in use, in its order ([] / [] without one)."""
        info = self.sched_info
        return self._schedules_in(info["text"] if info else "")

    def refine_schedules(self, params, status, tstep=None, n_steps=300, max_instances=8, max_new=8):
        """Instances a run flagged CSIM_ST_SCHED_FALLBACK used pivot sequences the generated kernels do not carry:
        they then finish on the general kernel, a handful of waves alone on the chip (buffer.sp, 4 096 Monte-Carlo
        instances at sigma 5 %: 31 instances, 0.8 % of the work, most of the wall time).  This replays up to
        `max_instances` of them through the planner, appends the sequences it has not seen to the loaded ones and
        re-specialises (generate + hipcc + load; needs hipcc).  `status` = the status words of that run (tensor or
        array).  Returns the number of sequences added (0: nothing done).  Results never depend on the list --
        every factorisation verifies the sequence it uses -- only how many instances stay on the fast kernels."""
        st = status.cpu().numpy() if hasattr(status, "cpu") else np.asarray(status)
        flagged = np.nonzero((st & 0x20) != 0)[0]
        known, known_dc = self.loaded_schedules()
        if not len(flagged) or not known:
            return 0
        have = set(known)
        new = {}
        for b in flagged[:max_instances]:
            alts, _ = self.record_pivot_schedules(params, int(b), tstep, n_steps)
            for sched, n in alts:
                if sched not in have:
                    new[sched] = new.get(sched, 0) + n
        if not new:
            return 0
        room = min(max_new, 16 - len(known))          # csim_engine_jit_with_schedules takes up to 16 transient sequences
        added = [s for s, _ in sorted(new.items(), key=lambda kv: -kv[1])][:max(0, room)]
        if not added:
            return 0
        self.jit_with_schedules(known + added, known_dc)
        return len(added)

    def record_pivot_schedule(self, params, instance=0, tstep=None, n_steps=200):
        """Planner: pivot row position per column of the first transient factorisation of one
        instance (general kernel), as (schedule string, #factorisations, #with another sequence)."""
        tstep = self.netlist.tstep if tstep is None else tstep
        pos = np.zeros(self.N, dtype=np.int32)
        nlu, ndiff = C.c_int64(), C.c_int64()
        capi.check(capi.lib().csim_record_pivot_schedule(self._h, params.data_ptr(), params.shape[1], instance,
                                                         float(tstep), int(n_steps), pos.ctypes.data,
                                                         C.byref(nlu), C.byref(ndiff)))
        sched = ",".join("%d:%d" % (k, p) for k, p in enumerate(pos) if p != k)
        return sched, nlu.value, ndiff.value

    def record_pivot_schedules(self, params, instance=0, tstep=None, n_steps=200, max_alts=8):
        """Planner: every distinct pivot sequence of one instance's transient factorisations,
        most frequent first: ([(schedule string, count), ...], n_other)."""
        tstep = self.netlist.tstep if tstep is None else tstep
        pos = np.zeros((max_alts, self.N), dtype=np.int32)
        counts = np.zeros(max_alts, dtype=np.int64)
        n_alts, other = C.c_int32(), C.c_int64()
        capi.check(capi.lib().csim_record_pivot_schedules(self._h, params.data_ptr(), params.shape[1], instance,
                                                          float(tstep), int(n_steps), max_alts, pos.ctypes.data,
                                                          counts.ctypes.data, C.byref(n_alts), C.byref(other)))
        out = []
        for a in range(n_alts.value):
            sched = ",".join("%d:%d" % (k, p) for k, p in enumerate(pos[a]) if p != k) or "-"
            out.append((sched, int(counts[a])))
        return out, other.value

    def record_dc_pivot_schedules(self, params, instance=0, max_alts=8):
        """Planner on the DC operating point of one instance: ([(schedule string, count), ...], n_other)."""
        pos = np.zeros((max_alts, self.N), dtype=np.int32)
        counts = np.zeros(max_alts, dtype=np.int64)
        n_alts, other = C.c_int32(), C.c_int64()
        capi.check(capi.lib().csim_record_dc_pivot_schedules(self._h, params.data_ptr(), params.shape[1], instance,
                                                             max_alts, pos.ctypes.data, counts.ctypes.data,
                                                             C.byref(n_alts), C.byref(other)))
        out = []
        for a in range(n_alts.value):
            sched = ",".join("%d:%d" % (k, p) for k, p in enumerate(pos[a]) if p != k) or "-"
            out.append((sched, int(counts[a])))
        return out, other.value

    def close(self):
        if self._h:
            capi.lib().csim_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lu_solve_batch(A, b, device=0):
    """Batched Solver::solveLinearSystemLU on the GPU.  A [B][n][n], b [B][n] numpy."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    B, n = b.shape
    x = np.zeros((B, n))
    flags = np.zeros(B, dtype=np.uint32)
    capi.check(capi.lib().csim_lu_solve_batch(device, n, B, A.ctypes.data, b.ctypes.data, x.ctypes.data,
                                              flags.ctypes.data))
    return x, flags


# the kernel selector of the *_solve_batch entries (include/csim.h); "block" covers AC and noise, n <= 1024
_AC_KERNELS = {"auto": 0, "wave": 1, "packed": 2, "block": 4}


def ac_solve_batch(G, Cm, J, omega, kernel="auto", device=0):
    """Batched complex solve (G + j w C) x = J through the AC sweep kernels (csim_ac_solve_batch).
    G, Cm [B][n][n] real, J [B][n] complex, omega [F] rad/s; kernel auto | wave | packed | block (n <= 1024).
    -> (x complex128 [B][F][n], flags [B])"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    J = np.ascontiguousarray(J, dtype=np.complex128)
    omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
    B, n = J.shape
    x = np.zeros((B, len(omega), n), dtype=np.complex128)
    flags = np.zeros(B, dtype=np.uint32)
    capi.check(capi.lib().csim_ac_solve_batch(device, n, B, G.ctypes.data, Cm.ctypes.data, J.ctypes.data,
                                              omega.ctypes.data, len(omega), _AC_KERNELS[kernel],
                                              x.ctypes.data, flags.ctypes.data))
    return x, flags


def noise_solve_batch(G, Cm, out, src_a, src_b, psd, omega, gain_in=None, kernel="auto", device=0, want_y=True):
    """Batched noise solve through the noise kernels (csim_noise_solve_batch): A^T y = d with A = G + j w C.
    G, Cm [B][n][n] real; out = (out_p, out_m), -1 = ground; generators src_a, src_b [S] with psd [B][S];
    omega [F] rad/s; gain_in None | ("v", k) | ("i", a, b): H = y[k] | y[a] - y[b]; kernel auto | wave | packed | block
    (n <= 1024).
    -> dict(onoise [B][F], contrib [B][F][S], gain complex [B][F] or None, y complex [B][F][n] or None, flags [B])"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
    src_a = np.ascontiguousarray(src_a, dtype=np.int32).reshape(-1)
    src_b = np.ascontiguousarray(src_b, dtype=np.int32).reshape(-1)
    B, n = G.shape[0], G.shape[1]
    S, F = len(src_a), len(omega)
    psd = np.ascontiguousarray(psd, dtype=np.float64).reshape(B, S)
    kind, in_a, in_b = 0, -1, -1
    if gain_in is not None:
        kind = {"v": 1, "i": 2}[gain_in[0]]
        in_a = int(gain_in[1])
        in_b = int(gain_in[2]) if kind == 2 else -1
    onoise = np.zeros((B, F))
    contrib = np.zeros((B, F, S))
    gain = np.zeros((B, F), dtype=np.complex128) if kind else None
    y = np.zeros((B, F, n), dtype=np.complex128) if want_y else None
    flags = np.zeros(B, dtype=np.uint32)
    capi.check(capi.lib().csim_noise_solve_batch(
        device, n, B, G.ctypes.data, Cm.ctypes.data, int(out[0]), int(out[1]), S, src_a.ctypes.data, src_b.ctypes.data,
        psd.ctypes.data, kind, in_a, in_b, omega.ctypes.data, F, _AC_KERNELS[kernel],
        onoise.ctypes.data, contrib.ctypes.data, gain.ctypes.data if gain is not None else None,
        y.ctypes.data if y is not None else None, flags.ctypes.data))
    return dict(onoise=onoise, contrib=contrib, gain=gain, y=y, flags=flags)


def disto_solve_batch(G, Cm, J, dev_d, dev_g, dev_s, coef, out, omega, kernel="auto", device=0, want_h=True):
    """The distortion kernels on systems and device tables given directly (csim_disto_solve_batch): (G + j k w C) x_k
    = rhs_k for k = 1, 2, 3.  G, Cm [B][n][n] real; J [B][n] complex; devices dev_d, dev_g, dev_s [M] (equations, -1 =
    ground) with coef [B][M][7]; out = (out_p, out_m), -1 = ground; omega [F] rad/s; kernel auto | wave | packed
    (block is refused: CSIM_ERR_UNSUPPORTED).
    -> dict(h complex [B][F][3][n] or None, hd [B][F][2], flags [B])"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    J = np.ascontiguousarray(J, dtype=np.complex128)
    omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
    dev_d = np.ascontiguousarray(dev_d, dtype=np.int32).reshape(-1)
    dev_g = np.ascontiguousarray(dev_g, dtype=np.int32).reshape(-1)
    dev_s = np.ascontiguousarray(dev_s, dtype=np.int32).reshape(-1)
    B, n = J.shape
    M, F = len(dev_d), len(omega)
    if len(dev_g) != M or len(dev_s) != M:
        raise ValueError("dev_d, dev_g and dev_s differ in length")
    coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(B, M, 7)
    h = np.zeros((B, F, 3, n), dtype=np.complex128) if want_h else None
    hd = np.zeros((B, F, 2))
    flags = np.zeros(B, dtype=np.uint32)
    capi.check(capi.lib().csim_disto_solve_batch(
        device, n, B, G.ctypes.data, Cm.ctypes.data, J.ctypes.data, M, dev_d.ctypes.data, dev_g.ctypes.data,
        dev_s.ctypes.data, coef.ctypes.data, int(out[0]), int(out[1]), omega.ctypes.data, F, _AC_KERNELS[kernel],
        h.ctypes.data if h is not None else None, hd.ctypes.data, flags.ctypes.data))
    return dict(h=h, hd=hd, flags=flags)


def imd_solve_batch(G, Cm, J, dev_d, dev_g, dev_s, coef, out, omega1, omega2, J2=None, kernel="auto", device=0,
                    want_h=True):
    """The intermodulation kernels on systems and device tables given directly (csim_imd_solve_batch): six solves per
    tone pair, at w1, w2, w1 + w2, w1 - w2, 2 w1 and 2 w1 - w2.  G, Cm [B][n][n] real; J [B][n] complex excites the
    first tone, J2 the second (None: J); devices dev_d, dev_g, dev_s [M] (equations, -1 = ground) with coef [B][M][7];
    out = (out_p, out_m), -1 = ground; omega1, omega2 [F] rad/s, any finite values; kernel auto | wave | packed (block
    is refused: CSIM_ERR_UNSUPPORTED).
    -> dict(h complex [B][F][6][n] or None, im [B][F][3] (IM2+, IM2-, IM3), flags [B])"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    J = np.ascontiguousarray(J, dtype=np.complex128)
    J2 = np.ascontiguousarray(J2, dtype=np.complex128) if J2 is not None else None
    omega1 = np.ascontiguousarray(omega1, dtype=np.float64).reshape(-1)
    omega2 = np.ascontiguousarray(omega2, dtype=np.float64).reshape(-1)
    dev_d = np.ascontiguousarray(dev_d, dtype=np.int32).reshape(-1)
    dev_g = np.ascontiguousarray(dev_g, dtype=np.int32).reshape(-1)
    dev_s = np.ascontiguousarray(dev_s, dtype=np.int32).reshape(-1)
    B, n = J.shape
    M, F = len(dev_d), len(omega1)
    if len(dev_g) != M or len(dev_s) != M:
        raise ValueError("dev_d, dev_g and dev_s differ in length")
    if len(omega2) != F:
        raise ValueError("omega1 and omega2 differ in length")
    if J2 is not None and J2.shape != J.shape:
        raise ValueError("J and J2 differ in shape")
    coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(B, M, 7)
    h = np.zeros((B, F, 6, n), dtype=np.complex128) if want_h else None
    im = np.zeros((B, F, 3))
    flags = np.zeros(B, dtype=np.uint32)
    capi.check(capi.lib().csim_imd_solve_batch(
        device, n, B, G.ctypes.data, Cm.ctypes.data, J.ctypes.data, J2.ctypes.data if J2 is not None else None, M,
        dev_d.ctypes.data, dev_g.ctypes.data, dev_s.ctypes.data, coef.ctypes.data, int(out[0]), int(out[1]),
        omega1.ctypes.data, omega2.ctypes.data, F, _AC_KERNELS[kernel], h.ctypes.data if h is not None else None,
        im.ctypes.data, flags.ctypes.data))
    return dict(h=h, im=im, flags=flags)


def oip3(h_or_v0, im3):
    """Output-referred third-order intercept amplitude |v0| sqrt(|v0| / |v5|) = |v0| / sqrt(IM3), from the fundamental
    at the output (complex phasor or magnitude; numpy or torch) and IM3; inf where IM3 is 0."""
    if hasattr(im3, "sqrt"):                                  # torch
        return abs(h_or_v0) / im3.sqrt()
    with np.errstate(divide="ignore"):
        return np.abs(h_or_v0) / np.sqrt(np.asarray(im3, dtype=np.float64))


def stb_solve_batch(G, Cm, probe, omega, kernel="auto", device=0, want_x=True, freqs=None):
    """The loop-gain kernels on systems given directly (csim_stb_solve_batch): (G + j w C) X = [e_k, e_x] and T from the
    two solutions.  G, Cm [B][n][n] real; probe = (eq_p, eq_m, eq_br), the equations of the probe's + node, - node and
    branch; omega [F] rad/s; kernel auto | wave | packed (block is refused: CSIM_ERR_UNSUPPORTED); freqs [F] in Hz,
    strictly increasing and positive: the margins are computed too.
    -> dict(t complex [B][F], x complex [B][F][2][n] or None, pm, fc, gm, f180, found [B] or None, flags [B])"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
    B, n = G.shape[0], G.shape[1]
    F = len(omega)
    if freqs is not None:
        freqs = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        if len(freqs) != F:
            raise ValueError("freqs and omega differ in length")
    t = np.zeros((B, F), dtype=np.complex128)
    x = np.zeros((B, F, 2, n), dtype=np.complex128) if want_x else None
    mg = np.full((B, 4), np.nan) if freqs is not None else None
    fd = np.zeros(B, dtype=np.int32) if freqs is not None else None
    flags = np.zeros(B, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None else None    # noqa: E731
    capi.check(capi.lib().csim_stb_solve_batch(
        device, n, B, G.ctypes.data, Cm.ctypes.data, int(probe[0]), int(probe[1]), int(probe[2]), omega.ctypes.data, F,
        _AC_KERNELS[kernel], t.ctypes.data, ptr(x), flags.ctypes.data, ptr(freqs), ptr(mg), ptr(fd)))
    r = Engine._stb_dict(None, t, x, mg, fd, None, 1)
    del r["freqs"], r["status"]
    r["flags"] = flags
    return r


def pz_solve_batch(G, Cm, fmax, sigma0=0.0, device=0):
    """The pole kernel on systems given directly (csim_pz_solve_batch): the finite poles of det(G + s C) = 0.  G, Cm
    [B][n][n] real, n <= 63; fmax in Hz (the cut), sigma0 in rad/s (the shift).
    -> dict(poles complex [B][n] (dominant first, NaN beyond n_poles), n_poles, n_rhp [B], max_re [B], flags [B])"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    B, n = G.shape[0], G.shape[1]
    poles = np.zeros((B, n), dtype=np.complex128)
    n_poles = np.zeros(B, dtype=np.int32)
    n_rhp = np.zeros(B, dtype=np.int32)
    max_re = np.zeros(B)
    flags = np.zeros(B, dtype=np.uint32)
    capi.check(capi.lib().csim_pz_solve_batch(device, n, B, G.ctypes.data, Cm.ctypes.data, float(fmax), float(sigma0),
                                              poles.ctypes.data, n_poles.ctypes.data, n_rhp.ctypes.data, max_re.ctypes.data,
                                              flags.ctypes.data))
    return dict(poles=poles, n_poles=n_poles, n_rhp=n_rhp, max_re=max_re, flags=flags)


def sp_solve_batch(G, Cm, J, omega, kernel="auto", device=0, port_eq=None, z0=None, want_s=True):
    """The S-parameter kernels on systems given directly (csim_sp_solve_batch): (G + j w C) X = J with K = 1 .. 4
    right-hand sides.  G, Cm [B][n][n] real; omega [F] rad/s; kernel auto | wave | packed (block is refused:
    CSIM_ERR_UNSUPPORTED).
    J [B][K][n] complex -> (x complex [B][F][K][n], flags [B]).
    With port_eq [P] and z0 [P] (J is ignored, may be None) the right-hand sides are the unit vectors at port_eq
    -> dict(x [B][F][P][n], y [B][F][P][P], s the same or None, flags [B])."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
    B, n, F = G.shape[0], G.shape[1], len(omega)
    which = _AC_KERNELS[kernel]
    flags = np.zeros(B, dtype=np.uint32)
    L = capi.lib()
    if port_eq is None:
        J = np.ascontiguousarray(J, dtype=np.complex128)
        K = J.shape[1] if J.ndim == 3 else 0
        x = np.zeros((B, F, K, n), dtype=np.complex128)
        capi.check(L.csim_sp_solve_batch(device, n, B, K, G.ctypes.data, Cm.ctypes.data, J.ctypes.data, omega.ctypes.data,
                                         F, which, x.ctypes.data, flags.ctypes.data, None, None, None, None))
        return x, flags
    pe = np.ascontiguousarray(port_eq, dtype=np.int32).reshape(-1)
    z = np.ascontiguousarray(z0, dtype=np.float64).reshape(-1)
    P = len(pe)
    if len(z) != P:
        raise ValueError("port_eq and z0 differ in length")
    x = np.zeros((B, F, P, n), dtype=np.complex128)
    y = np.zeros((B, F, P, P), dtype=np.complex128)
    s = np.zeros((B, F, P, P), dtype=np.complex128) if want_s else None
    capi.check(L.csim_sp_solve_batch(device, n, B, P, G.ctypes.data, Cm.ctypes.data, None, omega.ctypes.data, F, which,
                                     x.ctypes.data, flags.ctypes.data, pe.ctypes.data, z.ctypes.data, y.ctypes.data,
                                     s.ctypes.data if s is not None else None))
    return dict(x=x, y=y, s=s, flags=flags)


def sp_noise_solve_batch(G, Cm, port_eq, z0, src_a, src_b, psd, omega, kernel="auto", device=0, noise_params=None,
                         want_x=True):
    """The two-port noise kernels on systems given directly (csim_spnoise_solve_batch): (G + j w C)^T L = unit vectors
    at port_eq.  G, Cm [B][n][n] real; port_eq, z0 [P]; generators src_a, src_b [S] (-1 = ground) with psd [B][S];
    omega [F] rad/s; kernel auto | wave | packed (block is refused: CSIM_ERR_UNSUPPORTED).  noise_params: None = for two ports; True with any other port count
    is a ValueError.
    -> dict(y, cy complex [B][F][P][P], x complex [B][F][P][n] or None, flags [B]) and, for two ports, nf, fmin, rn
       [B][F], yopt complex [B][F]."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
    pe = np.ascontiguousarray(port_eq, dtype=np.int32).reshape(-1)
    z = np.ascontiguousarray(z0, dtype=np.float64).reshape(-1)
    src_a = np.ascontiguousarray(src_a, dtype=np.int32).reshape(-1)
    src_b = np.ascontiguousarray(src_b, dtype=np.int32).reshape(-1)
    B, n, F, P, S = G.shape[0], G.shape[1], len(omega), len(pe), len(src_a)
    if len(z) != P:
        raise ValueError("port_eq and z0 differ in length")
    if noise_params and P != 2:
        raise ValueError("NF, Fmin, Rn and Yopt exist for two ports only (%d given)" % P)
    two = P == 2 if noise_params is None else bool(noise_params)
    psd = np.ascontiguousarray(psd, dtype=np.float64).reshape(B, S)
    y = np.zeros((B, F, P, P), dtype=np.complex128)
    cy = np.zeros((B, F, P, P), dtype=np.complex128)
    nf, fmin, rn = (np.zeros((B, F)) for _ in range(3)) if two else (None,) * 3
    yopt = np.zeros((B, F), dtype=np.complex128) if two else None
    x = np.zeros((B, F, P, n), dtype=np.complex128) if want_x else None
    flags = np.zeros(B, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None else None    # noqa: E731
    capi.check(capi.lib().csim_spnoise_solve_batch(
        device, n, B, P, G.ctypes.data, Cm.ctypes.data, pe.ctypes.data, z.ctypes.data, S, src_a.ctypes.data,
        src_b.ctypes.data, psd.ctypes.data, omega.ctypes.data, F, _AC_KERNELS[kernel], y.ctypes.data,
        cy.ctypes.data, ptr(nf), ptr(fmin), ptr(rn), ptr(yopt), ptr(x), flags.ctypes.data))
    r = dict(y=y, cy=cy, x=x, flags=flags)
    if two:
        r.update(nf=nf, fmin=fmin, rn=rn, yopt=yopt)
    return r


def gs_solve_batch(A, b, x0=None, max_iters=1000, tol=1e-10, device=0):
    """Batched Solver::solveLinearSystemGaussSeidel on the GPU.  A [B][n][n], b/x0 [B][n] -> (x [B][n], sweeps [B])."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    B, n = b.shape
    x0a = np.ascontiguousarray(x0, dtype=np.float64) if x0 is not None else None
    x = np.zeros((B, n))
    sweeps = np.zeros(B, dtype=np.int32)
    capi.check(capi.lib().csim_gs_solve_batch(device, n, B, A.ctypes.data, b.ctypes.data,
                                              x0a.ctypes.data if x0a is not None else None, int(max_iters), float(tol),
                                              x.ctypes.data, sweeps.ctypes.data))
    return x, sweeps


def lu_decompose_batch(A, device=0):
    """Batched Solver::luDecompose on the GPU.  A [B][n][n] -> (LU [B][n][n], perm [B][n], flags [B])."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, n, _ = A.shape
    LU = np.zeros_like(A)
    perm = np.zeros((B, n), dtype=np.int32)
    flags = np.zeros(B, dtype=np.uint32)
    capi.check(capi.lib().csim_lu_decompose_batch(device, n, B, A.ctypes.data, LU.ctypes.data, perm.ctypes.data,
                                                  flags.ctypes.data))
    return LU, perm, flags
