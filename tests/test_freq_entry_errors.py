"""Argument refusals of the four engine-free frequency-domain entries (csim_{ac,noise,sp,spnoise}_solve_batch).

Every call of the table is refused before the entry looks for a device, so the code it returns is the same with and
without a GPU.  The expected codes were recorded from the library as it was before the entries moved to
engine_freq.cpp and began to share their helpers; they pin the order of the checks, not only their presence.
Shapes: n = 2, B = 1, F = 1 unless a case says otherwise.
"""
import numpy as np
import pytest

from circuitsimulator_amd import capi
from conftest import has_gpu

ARG, NO_DEVICE, CONFIG = capi.CSIM_ERR_ARG, capi.CSIM_ERR_NO_DEVICE, capi.CSIM_ERR_CONFIG
INF = float("inf")

# argument names in the order of include/csim.h
ORDER = {
    "ac": "device n B G Cm J omega F kernel x flags".split(),
    "noise": ("device n B G Cm out_p out_m S src_a src_b psd in_kind in_a in_b omega F kernel "
              "onoise contrib gain y flags").split(),
    "sp": "device n B K G Cm J omega F kernel x flags port_eq z0 y s".split(),
    "spnoise": "device n B P G Cm port_eq z0 S src_a src_b psd omega F kernel y cy nf fmin rn yopt x flags".split(),
}


def _valid(entry):
    """A call that every argument check lets through: one 2 x 2 system, one frequency, two ports, one generator."""
    f8 = lambda *shape: np.zeros(shape)            # noqa: E731
    i4 = lambda *v: np.array(v, dtype=np.int32)     # noqa: E731
    a = dict(device=0, n=2, B=1, F=1, kernel=0, G=np.eye(2)[None].copy(), Cm=f8(1, 2, 2), omega=np.ones(1),
             flags=np.zeros(1, dtype=np.uint32))
    if entry == "ac":
        a.update(J=f8(1, 2, 2), x=f8(1, 1, 2, 2))
    elif entry == "noise":
        a.update(out_p=0, out_m=-1, S=1, src_a=i4(0), src_b=i4(-1), psd=np.ones((1, 1)), in_kind=1, in_a=1, in_b=-1,
                 onoise=f8(1, 1), contrib=f8(1, 1, 1), gain=f8(1, 1, 2), y=f8(1, 1, 2, 2))
    elif entry == "sp":       # the port form; J and x are the right-hand-side form's
        a.update(K=2, J=None, x=None, port_eq=i4(0, 1), z0=np.array([50.0, 50.0]), y=f8(1, 1, 2, 2, 2), s=f8(1, 1, 2, 2, 2))
    else:
        a.update(P=2, port_eq=i4(0, 1), z0=np.array([50.0, 50.0]), S=1, src_a=i4(0), src_b=i4(-1), psd=np.ones((1, 1)),
                 y=f8(1, 1, 2, 2, 2), cy=f8(1, 1, 2, 2, 2), nf=f8(1, 1), fmin=f8(1, 1), rn=f8(1, 1), yopt=f8(1, 1, 2),
                 x=f8(1, 1, 2, 2, 2))
    return a


def call(entry, **change):
    a = _valid(entry)
    for k, v in change.items():
        assert k in a, k
        a[k] = np.asarray(v, dtype=a[k].dtype) if isinstance(a[k], np.ndarray) and v is not None else v
    keep = [v for v in a.values() if isinstance(v, np.ndarray)]          # alive during the call
    args = [a[k].ctypes.data if isinstance(a[k], np.ndarray) else a[k] for k in ORDER[entry]]
    rc = getattr(capi.lib(), "csim_%s_solve_batch" % entry)(*args)
    del keep
    return rc


SP_RHS = dict(port_eq=None, z0=None, y=None, s=None, J=np.zeros((1, 2, 2, 2)), x=np.zeros((1, 1, 2, 2, 2)))   # K given vectors
THREE_PORTS = dict(n=3, P=3, G=np.eye(3)[None], Cm=np.zeros((1, 3, 3)), port_eq=[0, 1, 2], z0=[50.0, 50.0, 50.0])

# (entry, what changes against _valid(entry), code recorded from the parent commit's library)
CASES = [
    # negative sizes
    ("ac", dict(n=-1), ARG), ("ac", dict(B=-1), ARG), ("ac", dict(F=-1), ARG),
    ("noise", dict(n=-1), ARG), ("noise", dict(B=-1), ARG), ("noise", dict(F=-1), ARG), ("noise", dict(S=-1), ARG),
    ("sp", dict(n=-1), ARG), ("sp", dict(B=-1), ARG), ("sp", dict(F=-1), ARG),
    ("spnoise", dict(n=-1), ARG), ("spnoise", dict(B=-1), ARG), ("spnoise", dict(F=-1), ARG), ("spnoise", dict(S=-1), ARG),
    # kernel selectors that do not exist (4 is the block kernel)
    ("ac", dict(kernel=3), ARG), ("ac", dict(kernel=5), ARG), ("noise", dict(kernel=3), ARG), ("noise", dict(kernel=5), ARG),
    ("sp", dict(kernel=3), ARG), ("sp", dict(kernel=5), ARG), ("spnoise", dict(kernel=3), ARG), ("spnoise", dict(kernel=5), ARG),
    # a required pointer is null although there is work
    ("ac", dict(G=None), ARG), ("ac", dict(Cm=None), ARG), ("ac", dict(J=None), ARG), ("ac", dict(omega=None), ARG),
    ("ac", dict(x=None), ARG),
    ("noise", dict(G=None), ARG), ("noise", dict(Cm=None), ARG), ("noise", dict(omega=None), ARG),
    ("noise", dict(onoise=None), ARG), ("noise", dict(src_a=None), ARG), ("noise", dict(src_b=None), ARG),
    ("noise", dict(psd=None), ARG),
    ("sp", dict(G=None), ARG), ("sp", dict(Cm=None), ARG), ("sp", dict(omega=None), ARG), ("sp", dict(z0=None), ARG),
    ("sp", dict(y=None), ARG), ("sp", dict(SP_RHS, J=None), ARG), ("sp", dict(SP_RHS, x=None), ARG),
    ("spnoise", dict(G=None), ARG), ("spnoise", dict(Cm=None), ARG), ("spnoise", dict(omega=None), ARG),
    ("spnoise", dict(cy=None), ARG), ("spnoise", dict(port_eq=None), ARG), ("spnoise", dict(z0=None), ARG),
    ("spnoise", dict(src_a=None), ARG), ("spnoise", dict(src_b=None), ARG), ("spnoise", dict(psd=None), ARG),
    # right-hand sides / ports: 1 to 4
    ("sp", dict(K=0), ARG), ("sp", dict(K=5), ARG), ("sp", dict(SP_RHS, K=0), ARG), ("sp", dict(SP_RHS, K=5), ARG),
    ("spnoise", dict(P=0), ARG), ("spnoise", dict(P=5), ARG),
    # an equation index equal to n
    ("noise", dict(out_p=2), ARG), ("noise", dict(out_m=2), ARG), ("noise", dict(src_a=[2]), ARG),
    ("noise", dict(src_b=[2]), ARG), ("noise", dict(in_a=2), ARG), ("noise", dict(in_kind=2, in_b=2), ARG),
    ("sp", dict(port_eq=[0, 2]), ARG), ("spnoise", dict(port_eq=[2, 1]), ARG), ("spnoise", dict(src_a=[2]), ARG),
    # the output needs two different equations
    ("noise", dict(out_p=1, out_m=1), ARG),
    # reference impedances: finite and positive
    ("sp", dict(z0=[50.0, 0.0]), ARG), ("sp", dict(z0=[INF, 50.0]), ARG),
    ("spnoise", dict(z0=[0.0, 50.0]), ARG), ("spnoise", dict(z0=[50.0, INF]), ARG),
    # kinds of input source: none, V, I
    ("noise", dict(in_kind=3), ARG), ("noise", dict(in_kind=-1), ARG),
    # noise parameters exist for two ports only
    ("spnoise", dict(THREE_PORTS), CONFIG),
    ("spnoise", dict(THREE_PORTS, fmin=None, rn=None, yopt=None), CONFIG),
    ("spnoise", dict(THREE_PORTS, nf=None, fmin=None, rn=None), CONFIG),
    # ... and the first failing check decides: a bad selector before a bad index, a bad count before a bad Z0,
    # a bad index before the three-port refusal
    ("noise", dict(kernel=3, out_p=2), ARG), ("sp", dict(K=5, z0=[0.0, 50.0]), ARG),
    ("spnoise", dict(THREE_PORTS, port_eq=[0, 1, 3]), ARG), ("spnoise", dict(THREE_PORTS, kernel=5), ARG),
]


def _id(case):
    entry, change, _ = case
    return entry + "-" + "-".join("%s=%s" % (k, "null" if v is None else getattr(v, "shape", v)) for k, v in change.items())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_refused_at_the_argument_stage(case):
    entry, change, code = case
    assert call(entry, **change) == code, capi.lib().csim_last_error()


def test_empty_calls_pass_the_argument_stage_with_null_buffers():
    """n, B or F of zero asks for no buffer: such a call gets as far as the device check (and is CSIM_OK with one)"""
    after = capi.CSIM_OK if has_gpu() else NO_DEVICE
    for entry in ORDER:
        nulls = {k: None for k in ("G", "Cm", "omega")}
        assert call(entry, F=0, **nulls) == after
        assert call(entry, B=0, **nulls) == after


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
@pytest.mark.parametrize("entry", sorted(ORDER))
def test_valid_calls_need_a_device(entry):
    """the device check comes after the argument checks and before sizes and kernel: also before the port entries'
    refusal of the block kernel (kernel = 4) and before the size limits (n = 64)"""
    assert call(entry) == NO_DEVICE
    assert call(entry, kernel=4) == NO_DEVICE
    big = dict(n=64, G=np.eye(64)[None], Cm=np.zeros((1, 64, 64)))
    if entry == "ac":
        big.update(J=np.zeros((1, 64, 2)), x=np.zeros((1, 1, 64, 2)))
    assert call(entry, **big) == NO_DEVICE
