"""ctypes binding of the C-ABI in include/csim.h (libcsim.so, built in-tree).

Plumbing only: every numeric result comes from the HIP kernels behind the
C-ABI.  There is no Python or CPU arithmetic fallback; if the library is
missing this module raises, and without a HIP device Engine() raises
CsimError(CSIM_ERR_NO_DEVICE).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcsim.so")

CSIM_OK = 0
CSIM_ERR_ARG = -1
CSIM_ERR_IO = -2
CSIM_ERR_NO_DEVICE = -3
CSIM_ERR_HIP = -4
CSIM_ERR_UNSUPPORTED = -5
CSIM_ERR_EMPTY = -6
CSIM_ERR_CONFIG = -7

# per-instance status bits (include/csim_ir.h)
ST_TRAN_NONFINITE = 0x0001
ST_TRAN_NONCONV = 0x0002
ST_LU_TINY_PIVOT = 0x0004
ST_DC_NONCONV = 0x0008
ST_DC_NONFINITE = 0x0010
ST_SCHED_FALLBACK = 0x0020
ST_SCHED_FALLBACK_DC = 0x0080
ST_SCHED_FAITHFUL = 0x0100
ST_LU_ZERO_DIAG = 0x0040
ST_PSS_NONCONV = 0x0200
ST_PSS_SINGULAR = 0x0400
ST_PAC_SINGULAR = 0x0800

# every symbol include/csim.h declares: name -> (restype, argtypes)
_vp, _i32, _i64, _u64, _dbl, _cp = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double, C.c_char_p
_pi32 = C.POINTER(C.c_int32)
_pdbl = C.POINTER(C.c_double)
PROTOTYPES = {
    "csim_last_error": (_cp, []),
    "csim_version": (_cp, []),
    "csim_netlist_parse_file": (C.c_int, [_cp, C.POINTER(_vp)]),
    "csim_netlist_parse_text": (C.c_int, [_cp, _i64, C.POINTER(_vp)]),
    "csim_netlist_free": (None, [_vp]),
    "csim_netlist_ir": (_vp, [_vp]),
    "csim_netlist_counts": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pi32, _pi32]),
    "csim_netlist_nominal_params": (C.c_int, [_vp, _vp]),
    "csim_netlist_eq_name": (_cp, [_vp, _i32]),
    "csim_netlist_node_eq": (C.c_int, [_vp, _cp]),
    "csim_netlist_tran": (C.c_int, [_vp, _pi32, _pdbl, _pdbl, _pdbl]),
    "csim_netlist_num_probes": (C.c_int, [_vp]),
    "csim_netlist_probe_eq": (C.c_int, [_vp, _i32]),
    "csim_netlist_num_dc_sweeps": (C.c_int, [_vp]),
    "csim_netlist_dc_sweep": (C.c_int, [_vp, _i32, _pi32, _pdbl, _pdbl, _pdbl]),
    "csim_netlist_dc_sweep_points": (_i64, [_vp, _i32]),
    "csim_netlist_dc_sweep_params": (C.c_int, [_vp, _i32, _i64, _vp, _vp]),
    "csim_netlist_csv_header": (C.c_int, [_vp, _cp, _i32]),
    "csim_netlist_mc_kinds": (C.c_int, [_vp, _vp]),
    "csim_netlist_ac": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pdbl, _pdbl]),
    "csim_netlist_ac_source": (C.c_int, [_vp, _i32, _pdbl, _pdbl]),
    "csim_netlist_noise": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pi32, _pi32, _pi32, _pdbl, _pdbl]),
    "csim_netlist_num_noise_sources": (C.c_int, [_vp]),
    "csim_netlist_noise_source": (C.c_int, [_vp, _i32, _pi32, _pi32, _pi32]),
    "csim_noise_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csim_noise_batch": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "csim_noise_solve_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32,
                                         _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "csim_netlist_disto": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pi32, _pi32, _pdbl, _pdbl]),
    "csim_netlist_imd": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pi32, _pi32, _pdbl, _pdbl, _pdbl]),
    "csim_imd_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "csim_imd_batch": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _dbl, _i32, _i32, _vp, _vp, _vp, _vp]),
    "csim_imd_solve_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp,
                                       _i32, _i32, _vp, _vp, _vp]),
    "csim_netlist_num_disto_devices": (C.c_int, [_vp]),
    "csim_netlist_disto_device": (C.c_int, [_vp, _i32, _pi32, _pi32, _pi32, _pi32]),
    "csim_disto_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "csim_disto_batch": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "csim_disto_solve_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32,
                                         _i32, _vp, _vp, _vp]),
    "csim_netlist_stb": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pi32, _pi32, _pi32, _pi32, _pdbl, _pdbl]),
    "csim_stb_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csim_stb_batch": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "csim_stb_solve_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                                       _vp]),
    "csim_netlist_hb": (C.c_int, [_vp, _pi32, _pdbl, _pi32]),
    "csim_pss_num_steps": (_i64, [_dbl, _dbl]),
    "csim_pss_twiddles": (C.c_int, [_i64, _vp, _vp]),
    "csim_pss_batch_dev": (C.c_int, [_vp, _vp, _i32, _dbl, _dbl, _i32, _vp, _i32, _dbl, _i32, _vp, _vp, _vp, _vp, _vp]),
    "csim_pss_batch": (C.c_int, [_vp, _vp, _i32, _dbl, _dbl, _i32, _vp, _i32, _dbl, _i32, _vp, _vp, _vp, _vp]),
    "csim_netlist_pac": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pdbl, _pdbl, _pi32]),
    "csim_pac_batch_dev": (C.c_int, [_vp, _vp, _i32, _dbl, _dbl, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "csim_pac_batch": (C.c_int, [_vp, _vp, _i32, _dbl, _dbl, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "csim_netlist_pnoise": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pi32, _pi32, _pi32, _pdbl, _pdbl, _pi32]),
    "csim_pnoise_batch_dev": (C.c_int, [_vp, _vp, _i32, _dbl, _dbl, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp,
                                        _vp, _vp, _vp]),
    "csim_pnoise_batch": (C.c_int, [_vp, _vp, _i32, _dbl, _dbl, _vp, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp]),
    "csim_netlist_pz": (C.c_int, [_vp, _pi32, _pdbl, _pdbl]),
    "csim_pz_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csim_pz_batch": (C.c_int, [_vp, _vp, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "csim_pz_solve_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "csim_netlist_num_ports": (C.c_int, [_vp]),
    "csim_netlist_port": (C.c_int, [_vp, _i32, _pi32, _pi32, _pdbl]),
    "csim_netlist_sp": (C.c_int, [_vp, _pi32, _pi32, _pi32, _pdbl, _pdbl]),
    "csim_sp_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "csim_sp_batch": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "csim_netlist_sp_noise": (C.c_int, [_vp, _pi32]),
    "csim_spnoise_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csim_spnoise_batch": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csim_spnoise_solve_batch": (C.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csim_sp_solve_batch": (C.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "csim_ac_num_freqs": (_i64, [_i32, _i32, _dbl, _dbl]),
    "csim_ac_freqs": (C.c_int, [_i32, _i32, _dbl, _dbl, _vp]),
    "csim_ac_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "csim_ac_batch": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp]),
    "csim_ac_system_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "csim_engine_create": (C.c_int, [_vp, _i32, C.POINTER(_vp)]),
    "csim_engine_destroy": (None, [_vp]),
    "csim_engine_tran_kernel": (_cp, [_vp]),
    "csim_engine_set_kernel": (C.c_int, [_vp, _i32]),
    "csim_engine_sched_info": (_cp, [_vp]),
    "csim_engine_lanes_for_batch": (C.c_int, [_vp, _i32]),
    "csim_mc_params_dev": (C.c_int, [_vp, _u64, _dbl, _i64, _i32, _vp, _vp]),
    "csim_mc_params_host": (C.c_int, [_vp, _u64, _dbl, _i64, _i32, _vp]),
    "csim_dc_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "csim_tran_batch_dev": (C.c_int, [_vp, _vp, _i32, _dbl, _i64, _i64, _vp, _i32, _i32,
                                      _vp, _vp, _vp, _vp, _vp, _vp]),
    "csim_dc_batch": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "csim_tran_batch": (C.c_int, [_vp, _vp, _i32, _dbl, _dbl, _dbl, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "csim_tran_write_csv": (C.c_int, [_vp, _vp, _i32, _i32, _dbl, _dbl, _dbl, _vp, _i32, _cp]),
    "csim_tran_num_rows": (_i64, [_dbl, _dbl, _dbl, _i32]),
    "csim_tran_num_steps": (_i64, [_dbl, _dbl]),
    "csim_lu_solve_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "csim_ac_solve_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "csim_lu_decompose_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "csim_gs_solve_batch": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _i32, _dbl, _vp, _vp]),
    "csim_dc_gs_batch_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "csim_dc_gs_batch": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "csim_engine_jit_scheduled": (C.c_int, [_vp, _vp, _i32, _dbl, _i64]),
    "csim_engine_jit_with_schedules": (C.c_int, [_vp, _vp, _i32, _vp, _i32]),
    "csim_engine_set_option": (C.c_int, [_vp, _cp, _cp]),
    "csim_engine_stat": (_i64, [_vp, _cp]),
    "csim_record_pivot_schedules": (C.c_int, [_vp, _vp, _i32, _i32, _dbl, _i64, _i32, _vp, _vp, _pi32,
                                              C.POINTER(C.c_int64)]),
    "csim_record_dc_pivot_schedules": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _pi32, C.POINTER(C.c_int64)]),
    "csim_record_pivot_schedule": (C.c_int, [_vp, _vp, _i32, _i32, _dbl, _i64, _vp, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]),
}


class CsimError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("csim error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load libcsim.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "circuitsimulator_amd: %s is missing -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                "There is no fallback path." % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64
        # (same SONAME as /opt/rocm's).  Importing torch first makes libcsim's
        # NEEDED libamdhip64.so.7 resolve to that already-loaded copy, so
        # device pointers and streams are shared; loading libcsim first would
        # pull in a second runtime that cannot see the device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc):
    if rc != CSIM_OK:
        raise CsimError(rc, lib().csim_last_error().decode("utf-8", "replace"))
    return rc
