"""circuitsimulator_amd -- MI355X-native batched DC / transient MNA solve engine.

Drop-in for one path of ZyuRao/CircuitSimulator: stamp -> pivoted dense LU ->
damped Newton update, for a batch of independent circuit instances, behind
the C-ABI declared in include/csim.h (libcsim.so, HIP kernels for gfx950).
"""
from .capi import CsimError, lib  # noqa: F401
from .engine import (Engine, Netlist, ac_solve_batch, disto_solve_batch, gs_solve_batch, imd_solve_batch,  # noqa: F401
                     lu_decompose_batch, lu_solve_batch, noise_solve_batch, oip3, pss_num_steps, pss_twiddles,
                     pz_solve_batch, sp_noise_solve_batch, sp_solve_batch, stb_solve_batch)

__all__ = ["Engine", "Netlist", "CsimError", "lu_solve_batch", "lu_decompose_batch", "gs_solve_batch", "ac_solve_batch",
           "disto_solve_batch", "imd_solve_batch", "oip3", "noise_solve_batch", "sp_noise_solve_batch", "sp_solve_batch",
           "stb_solve_batch", "pz_solve_batch", "pss_num_steps", "pss_twiddles", "lib"]
