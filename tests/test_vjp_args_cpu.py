"""The vector-Jacobian products (include/grbda_hip_vjp.h) without a GPU: the symbols, the second signature table against that header
parameter by parameter, and the argument rules -- every refusal is decided before a device is looked at, so a machine without one
answers GRBDA_EINVAL to a bad call and GRBDA_ENODEVICE only to a good one.  The arrays are host buffers standing in for device arrays:
the rules never read them, and no call that passes the rules is made where a device is present."""
import ctypes
import os

import numpy as np
import pytest

import generalized_rbda_amd as G
import test_abi_table_cpu as abi
from generalized_rbda_amd._abi import SIGNATURES, VJP_SIGNATURES
from id_derivative_refs import blob_of

EINVAL, ENODEVICE, OK = -1, -3, 0
ENTRY_POINTS = ("grbda_rnea_vjp_f64", "grbda_rnea_vjp_f32", "grbda_rnea_vjp_host_f64", "grbda_aba_vjp_f64", "grbda_aba_vjp_f32", "grbda_aba_vjp_host_f64")
VJP_HEADER = os.path.join(os.path.dirname(abi.HEADER), "grbda_hip_vjp.h")


def test_the_six_symbols_are_exported_and_bound():
    L = ctypes.CDLL(G.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in VJP_SIGNATURES and name not in SIGNATURES
    for method in ("id_vjp", "fd_vjp", "forward_dynamics_ad", "inverse_dynamics_ad"):
        assert callable(getattr(G.Plan, method))


def test_the_first_table_is_still_the_first_header():
    assert len(SIGNATURES) == 96 and len(G.C_ABI_SYMBOLS) == 96
    assert not set(SIGNATURES) & set(VJP_SIGNATURES)


def test_the_second_table_declares_what_the_second_header_does(monkeypatch):
    monkeypatch.setattr(abi, "HEADER", VJP_HEADER)
    protos = abi.header_prototypes()
    assert set(ENTRY_POINTS) <= set(protos) and len(protos) == len(ENTRY_POINTS) + 1  # (+ grbda_vjp_contract_launch)
    assert protos["grbda_aba_vjp_f32"][1][5] == ("double", "step") and protos["grbda_aba_vjp_f64"][1][-3] == ("size_t", "B")
    assert [p for _, p in protos["grbda_rnea_vjp_host_f64"][1]][-1] == "device"
    abi.compare(VJP_SIGNATURES, protos)
    # (the comparison does fail on a defect: the step declared as a pointer)
    broken = dict(VJP_SIGNATURES)
    args = list(broken["grbda_rnea_vjp_f64"][1])
    args[5] = ctypes.c_void_p
    broken["grbda_rnea_vjp_f64"] = (ctypes.c_int, tuple(args))
    with pytest.raises(AssertionError):
        abi.compare(broken, protos)


def test_the_loaded_library_carries_the_second_table(monkeypatch):
    monkeypatch.setattr(G, "_lib", None)  # (a fresh load)
    L = G.lib()
    for name, (restype, argtypes) in VJP_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(argtypes), name
        assert fn.restype is restype, name
    assert len(L.grbda_aba_vjp_f64.argtypes) == 13 and len(L.grbda_rnea_vjp_host_f64.argtypes) == 11


class _Call:
    """one plan, host buffers of B states standing in for the arrays"""

    def __init__(self, model="tree16_fixed", B=3):
        self.plan = G.Plan(blob_of(model))
        nq, nv = self.plan.nq, self.plan.nv
        self.B, self.nv = B, nv
        self.q, self.qd, self.x, self.g = np.zeros((B, nq)), np.zeros((B, nv)), np.zeros((B, nv)), np.zeros((B, nv))
        self.out = np.zeros((4, B, nv))

    def __call__(self, fn_name, q="q", qd="qd", x="x", g="g", step=1e-6, grad_q=0, grad_qd=1, grad_x=2, ydd=3, B=None, plan=True):
        def ptr(a):
            if a is None:
                return None
            if isinstance(a, str):
                return getattr(self, a).ctypes.data
            if isinstance(a, int) and 0 <= a < 4:
                return self.out[a].ctypes.data
            return a  # a raw address

        args = [self.plan._h if plan else None, ptr(q), ptr(qd), ptr(x), ptr(g), step, ptr(grad_q), ptr(grad_qd), ptr(grad_x)]
        if "aba" in fn_name:
            args.append(ptr(ydd))
        args += [self.B if B is None else B, 0]
        if "host" not in fn_name:
            args.append(None)
        return getattr(G.lib(), fn_name)(*args)


def _item(fn):
    return 4 if fn.endswith("f32") and "host" not in fn else 8


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_null_arguments_are_refused(fn):
    c = _Call()
    assert c(fn, plan=False) == EINVAL
    assert c(fn, plan=False, q=None, B=0) == EINVAL
    for name in ("q", "qd", "x", "g"):
        assert c(fn, **{name: None}) == EINVAL, name
        assert c(fn, B=0, **{name: None}) == EINVAL, name
    assert c(fn, grad_q=None, grad_qd=None, grad_x=None) == EINVAL  # any gradient may be null, not all three ...
    assert c(fn, grad_q=None, grad_qd=None, grad_x=None, B=0) == EINVAL
    assert "no output" in G.lib().grbda_last_error().decode()      # ... and ydd (the forward side) does not count


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_overlapping_arguments_are_refused(fn):
    c = _Call()
    last = (c.B * c.nv - 1) * _item(fn)
    assert c(fn, grad_q=0, grad_qd=0) == EINVAL                                  # the same array twice
    assert c(fn, grad_q=0, grad_x=c.out[0].ctypes.data + last) == EINVAL         # the last element of one is the first of the other
    assert c(fn, grad_qd=None, grad_x=None, grad_q=c.qd.ctypes.data) == EINVAL   # an output on an input
    assert c(fn, grad_q=None, grad_x=None, grad_qd=c.g.ctypes.data + last) == EINVAL
    assert c(fn, grad_q=None, grad_qd=None, grad_x=c.x.ctypes.data) == EINVAL
    if "aba" in fn:
        assert c(fn, ydd=0) == EINVAL                                            # ydd on grad_q
        assert c(fn, ydd=c.x.ctypes.data + last) == EINVAL                       # ydd on tau


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_step_is_checked_where_a_difference_route_needs_it(fn):
    c = _Call("tree65_fixed")  # 65 velocities: off the analytic route
    for step in (0.0, -1e-6, float("nan")):
        assert c(fn, step=step) == EINVAL, step
        assert c(fn, step=step, grad_qd=None, grad_x=None) == EINVAL
    assert "step" in G.lib().grbda_last_error().decode()
    assert c(fn, step=0.0, B=0, grad_q=None) == OK  # (no position gradient, no difference in q: nothing needs the step)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_an_empty_batch_is_ok(fn):
    c = _Call()
    assert c(fn, B=0) == OK
    assert c(fn, B=0, grad_q=None, grad_x=None, ydd=None) == OK
    assert c(fn, B=0, step=0.0) == OK  # (the analytic route never uses the step)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_a_good_call_needs_a_device(fn):
    if G.device_count() > 0:
        pytest.skip("a HIP device is present")
    for model in ("tree16_fixed", "tree65_fixed"):
        c = _Call(model)
        assert c(fn) == ENODEVICE
        assert c(fn, grad_q=None, grad_qd=None, ydd=None) == ENODEVICE
        assert c(fn, step=0.0, grad_q=None) == ENODEVICE  # (no position gradient: the step is not looked at)
    assert _Call("tree16_fixed")(fn, step=0.0) == ENODEVICE


def test_python_refuses_a_bad_want_and_host_tensors():
    import torch

    plan = G.Plan(blob_of("tree16_fixed"))
    z = torch.zeros((1, plan.nv), dtype=torch.float64)
    q = torch.zeros((1, plan.nq), dtype=torch.float64)
    for method in (plan.id_vjp, plan.fd_vjp):
        for want in ((), ("dq",), ("q", "H")):
            with pytest.raises(ValueError):
                method(q, z, z, z, want=want)
        with pytest.raises(G.GrbdaError):  # (no CPU fallback)
            method(q, z, z, z)
    with pytest.raises(ValueError):
        plan.id_vjp(q, z, z, z, want=("q", "ydd", "tau"))
    with pytest.raises(ValueError):
        plan.fd_vjp(q, z, z, z, want=("ydd",))  # (ydd alone is forward_dynamics)


def test_a_position_gradient_needs_as_many_positions_as_velocities():
    import torch

    plan = G.Plan(blob_of("mini_cheetah"))  # quaternion base: nq = nv + 1
    assert plan.nq == plan.nv + 1
    q = torch.zeros((1, plan.nq), dtype=torch.float64, requires_grad=True)
    z = torch.zeros((1, plan.nv), dtype=torch.float64)
    with pytest.raises(ValueError, match="fd_vjp"):
        plan.forward_dynamics_ad(q, z, z)
    with pytest.raises(ValueError, match="id_vjp"):
        plan.inverse_dynamics_ad(q, z, z)


def test_the_contraction_launch_rule():
    """units: packs of floor(64 / nv) states up to nv = 32, one state up to 64, blocks of 64 columns beyond; the grid: sixteen
    one-wavefront workgroups per CU, at most one per unit"""
    launch = G.vjp_contract_launch
    assert launch(4, 1, 256) == (1, 1) and launch(4, 16, 256) == (1, 1) and launch(4, 17, 256) == (2, 2)
    assert launch(18, 70, 256) == (24, 24)          # three per wavefront
    assert launch(31, 5, 256) == (3, 3) and launch(32, 5, 256) == (3, 3) and launch(33, 5, 256) == (5, 5)
    assert launch(64, 70, 256) == (70, 70) and launch(65, 70, 256) == (140, 140)
    assert launch(4, 16 * 4096, 256) == (4096, 4096) and launch(4, 16 * 4096 + 1, 256) == (4097, 4096)  # the second trip
    assert launch(64, 10, 1) == (10, 10) and launch(64, 17, 1) == (17, 16)
    assert G.lib().grbda_vjp_contract_launch(0, 1, 256, None, None) == EINVAL
