"""The block kernels (kernels_ac.hip ac_sweep_block_kernel, kernels_noise.hip ac_noise_block_kernel: one 256-thread
workgroup per system, the matrix in a global scratch, 1 <= n <= 1024) fed directly through csim_ac_solve_batch and
csim_noise_solve_batch with kernel="block" and compared bit for bit with tests/ac_reference.py and
tests/noise_reference.py (which tests/test_ac_block_cpu.py holds against the host-compiled ac_lu_solve() on these same
inputs), and with the wave kernel where both run.

Inputs: tests/ac_block_cases.py.  The planes never live in LDS, so no size switches their placement; 97 to 100 and
128 / 129 stay as the sizes around a power of two and around where an LDS placement would have ended.

NaN and singular inputs are ordinary data for these kernels: only arithmetic results depend on them, never an
address or a loop bound (the row list of a column holds row indices the kernel itself produced).  The equation
indices that index LDS are checked on the host before a launch.  Nothing here provokes a fault.
"""
import numpy as np
import pytest

import ac_block_cases as bc
import ac_cases as cs
import noise_reference as nref
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

KEYS = ("onoise", "contrib", "gain", "y")


@pytest.mark.parametrize("n", bc.GPU_SIZES)
def test_block_equals_reference_bitwise(n):
    from circuitsimulator_amd import ac_solve_batch
    for kind in cs.KINDS:
        c = bc.case(kind, n)
        flags, xref, per_f, _ = bc.reference(kind, n)
        for B in (1, 3):
            x, fl = ac_solve_batch(c["G"][:B], c["C"][:B], c["J"][:B], bc.OMEGA, kernel="block")
            where = (kind, n, B)
            assert x.shape == (B, len(bc.OMEGA), n)
            assert np.array_equal(fl, flags[:B]), where + (fl.tolist(), flags[:B].tolist())
            bc.same(x, xref[:B], kind in cs.HAS_NAN, where)
            bc.failed_are_plus_zero(x, per_f[:B], where)


@pytest.mark.parametrize("kind", bc.BIG_KINDS)
def test_block_equals_reference_bitwise_257(kind):
    from circuitsimulator_amd import ac_solve_batch
    n = bc.BIG_N
    c = bc.case(kind, n, 1)
    flags, xref, per_f, _ = bc.reference(kind, n, 1)
    x, fl = ac_solve_batch(c["G"][:1], c["C"][:1], c["J"][:1], bc.OMEGA, kernel="block")
    assert np.array_equal(fl, flags), (kind, fl.tolist(), flags.tolist())
    bc.same(x, xref, kind in cs.HAS_NAN, (kind, n))
    bc.failed_are_plus_zero(x, per_f, (kind, n))


def test_block_equals_reference_bitwise_tri1024():
    from circuitsimulator_amd import ac_solve_batch
    G, C, J = bc.tri1024()
    flags, xref, per_f, _ = bc.tri1024_reference()
    x, fl = ac_solve_batch(G[None], C[None], J[None], bc.OMEGA, kernel="block")
    assert fl.tolist() == [flags] == [0]
    bc.same(x[0], xref, False, ("tri1024",))


@pytest.mark.parametrize("n", bc.SMALL_SIZES)
def test_block_equals_wave_bitwise_below_64(n):
    from circuitsimulator_amd import ac_solve_batch
    ran = 0
    for kind in cs.KINDS:
        c = bc.case(kind, n, cs.NSYS)
        if c is None:
            continue
        xw, fw = ac_solve_batch(c["G"], c["C"], c["J"], bc.OMEGA, kernel="wave")
        xb, fb = ac_solve_batch(c["G"], c["C"], c["J"], bc.OMEGA, kernel="block")
        assert np.array_equal(fw, fb), (kind, n, fw.tolist(), fb.tolist())
        bc.same(xb, xw, kind in cs.HAS_NAN and np.isnan(xw.view(np.float64)).any(), (kind, n))
        ran += 1
    assert ran >= len(cs.KINDS) - 3


# ---- noise
def _noise_reference(c, st, nsys):
    res = [nref.solve_sweep(c["G"][s], c["C"][s], bc.OMEGA, st["out"], st["src_a"], st["src_b"], st["psd"][s],
                            st["gain_in"]) for s in range(nsys)]
    out = {k: np.stack([r[k] for r in res]) for k in KEYS}
    out["flags"] = np.array([r["flags"] for r in res], dtype=np.uint32)
    out["per_f"] = [r["per_f"] for r in res]
    return out


def _noise_run(c, st, B, kernel):
    from circuitsimulator_amd import noise_solve_batch
    return noise_solve_batch(c["G"][:B], c["C"][:B], st["out"], st["src_a"], st["src_b"], st["psd"][:B], bc.OMEGA,
                             gain_in=st["gain_in"], kernel=kernel)


@pytest.mark.parametrize("n", bc.NOISE_SIZES)
def test_noise_block_equals_reference_bitwise(n):
    """the systems transposed (noise_reference.adjoint_case), with the seeded output pairs, generator tables (ground
    terminals and a == b among them, up to 3 n generators) and gain inputs of noise_reference.setup()"""
    seen_ground = seen_same = False
    for kind in cs.KINDS:
        c = nref.adjoint_case(bc.case(kind, n))
        st = nref.setup(cs.KINDS.index(kind), n)
        a, b = st["src_a"], st["src_b"]
        seen_ground |= bool(np.any(a < 0) or np.any(b < 0))
        seen_same |= bool(np.any(a == b))
        ref = _noise_reference(c, st, bc.NSYS)
        for B in (1, 3):
            r = _noise_run(c, st, B, "block")
            where = (kind, n, B)
            assert np.array_equal(r["flags"], ref["flags"][:B]), where + (r["flags"].tolist(), ref["flags"][:B].tolist())
            for k in KEYS:
                bc.same(r[k], ref[k][:B], kind in cs.HAS_NAN, where + (k,))
                bc.failed_are_plus_zero(r[k], ref["per_f"][:B], where + (k,))
    assert seen_ground and seen_same


def test_noise_block_equals_wave_bitwise_at_63():
    n = 63
    for kind in cs.KINDS:
        c = nref.adjoint_case(bc.case(kind, n, cs.NSYS))
        st = nref.setup(cs.KINDS.index(kind), n)
        rw, rb = _noise_run(c, st, cs.NSYS, "wave"), _noise_run(c, st, cs.NSYS, "block")
        assert np.array_equal(rw["flags"], rb["flags"]), kind
        for k in KEYS:
            bc.same(rb[k], rw[k], kind in cs.HAS_NAN, (kind, k))


# ---- refusals
def test_block_beyond_1024_is_refused():
    from circuitsimulator_amd import CsimError, ac_solve_batch, capi, noise_solve_batch
    n = 1025
    G = np.eye(n)[None]
    with pytest.raises(CsimError) as e:
        ac_solve_batch(G, np.zeros_like(G), np.ones((1, n), dtype=complex), bc.OMEGA, kernel="block")
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
    with pytest.raises(CsimError) as e:
        noise_solve_batch(G, np.zeros_like(G), (0, -1), [0], [-1], np.ones((1, 1)), bc.OMEGA, kernel="block")
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED


@pytest.mark.parametrize("n", [5, 65])
def test_port_analyses_refuse_the_block_kernel(n):
    from circuitsimulator_amd import CsimError, capi, sp_noise_solve_batch, sp_solve_batch
    G = np.eye(n)[None]
    Z = np.zeros_like(G)
    with pytest.raises(CsimError) as e:
        sp_solve_batch(G, Z, np.ones((1, 2, n), dtype=complex), bc.OMEGA, kernel="block")
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED and "AC and noise" in str(e.value)
    with pytest.raises(CsimError) as e:
        sp_solve_batch(G, Z, None, bc.OMEGA, kernel="block", port_eq=[0, 1], z0=[50.0, 50.0])
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED
    with pytest.raises(CsimError) as e:
        sp_noise_solve_batch(G, Z, [0, 1], [50.0, 50.0], [0], [-1], np.ones((1, 1)), bc.OMEGA, kernel="block")
    assert e.value.code == capi.CSIM_ERR_UNSUPPORTED and "AC and noise" in str(e.value)
