"""The vector-Jacobian products of integrate, step and rollout (include/grbda_hip_step_vjp.h) without a GPU, in the manner of
test_vjp_args_cpu.py: the symbols, the third signature table against the third header parameter by parameter, and the argument rules --
every refusal is decided before a device is looked at, so a machine without one answers GRBDA_EINVAL / GRBDA_EUNSUPPORTED to a bad call and
GRBDA_ENODEVICE only to a good one.  The arrays are host buffers standing in for device arrays: the rules never read them, and no call
that passes the rules is made where a device is present."""
import ctypes
import os

import numpy as np
import pytest

import generalized_rbda_amd as G
import test_abi_table_cpu as abi
from generalized_rbda_amd._abi import SIGNATURES, STEP_VJP_SIGNATURES, VJP_SIGNATURES
from id_derivative_refs import blob_of

EINVAL, ENODEVICE, EUNSUPPORTED, OK = -1, -3, -2, 0
INTEGRATE = ("grbda_integrate_vjp_f64", "grbda_integrate_vjp_f32")
STEP = ("grbda_step_vjp_f64", "grbda_step_vjp_f32", "grbda_step_vjp_host_f64")
ROLLOUT = ("grbda_rollout_vjp_f64", "grbda_rollout_vjp_f32")
ENTRY_POINTS = INTEGRATE + STEP + ROLLOUT
HEADER = os.path.join(os.path.dirname(abi.HEADER), "grbda_hip_step_vjp.h")
T = 3


def test_the_seven_symbols_are_exported_and_bound():
    L = ctypes.CDLL(G.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in STEP_VJP_SIGNATURES and name not in SIGNATURES and name not in VJP_SIGNATURES
    for method in ("integrate_vjp", "step_vjp", "rollout_vjp", "tangent_cotangent", "step_ad", "rollout_ad"):
        assert callable(getattr(G.Plan, method))


def test_the_first_two_tables_keep_their_counts():
    assert len(SIGNATURES) == 96 and len(G.C_ABI_SYMBOLS) == 96 and len(VJP_SIGNATURES) == 7 and len(STEP_VJP_SIGNATURES) == 7
    assert not set(SIGNATURES) & set(STEP_VJP_SIGNATURES) and not set(VJP_SIGNATURES) & set(STEP_VJP_SIGNATURES)


def test_the_third_table_declares_what_the_third_header_does(monkeypatch):
    monkeypatch.setattr(abi, "HEADER", HEADER)
    protos = abi.header_prototypes()
    assert set(protos) == set(ENTRY_POINTS)
    assert protos["grbda_integrate_vjp_f32"][1][2] == ("double", "dt") and protos["grbda_step_vjp_f64"][1][8] == ("double", "step")
    assert protos["grbda_rollout_vjp_f32"][1][8] == ("int", "T") and protos["grbda_rollout_vjp_f64"][1][-3] == ("size_t", "B")
    assert [p for _, p in protos["grbda_step_vjp_host_f64"][1]][-1] == "device"
    abi.compare(STEP_VJP_SIGNATURES, protos)
    # (the comparison does fail on a defect: g_steps declared as a pointer)
    broken = dict(STEP_VJP_SIGNATURES)
    args = list(broken["grbda_rollout_vjp_f64"][1])
    assert args[11] is ctypes.c_int
    args[11] = ctypes.c_void_p
    broken["grbda_rollout_vjp_f64"] = (ctypes.c_int, tuple(args))
    with pytest.raises(AssertionError):
        abi.compare(broken, protos)


def test_the_loaded_library_carries_the_third_table(monkeypatch):
    monkeypatch.setattr(G, "_lib", None)  # (a fresh load)
    L = G.lib()
    for table in (STEP_VJP_SIGNATURES, VJP_SIGNATURES):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(argtypes), name
            assert fn.restype is restype, name
    assert len(L.grbda_integrate_vjp_f64.argtypes) == 11 and len(L.grbda_step_vjp_host_f64.argtypes) == 14 and len(L.grbda_rollout_vjp_f32.argtypes) == 19


class _Call:
    """one plan, host buffers of B states (T steps for the rollout) standing in for the arrays; an argument is a name of a buffer, an
    index into the three outputs, None, or a raw address"""

    def __init__(self, model="tree16_fixed", B=3):
        self.plan = G.Plan(blob_of(model))
        nq, nv = self.plan.nq, self.plan.nv
        self.B, self.nv, self.nq = B, nv, nq
        z = lambda *shape: np.zeros(shape)
        self.q, self.qd, self.tau, self.qd_next, self.g_q, self.g_qd = z(B, nq), z(B, nv), z(T, B, nv), z(B, nv), z(T, B, nv), z(T, B, nv)
        self.q_traj, self.qd_traj = z(T, B, nq), z(T, B, nv)
        self.out = z(3, T, B, nv)

    def ptr(self, a):
        if a is None:
            return None
        if isinstance(a, str):
            return getattr(self, a).ctypes.data
        if isinstance(a, int) and 0 <= a < 3:
            return self.out[a].ctypes.data
        return a

    def __call__(self, fn, plan=True, B=None, dt=0.01, step=1e-6, n_steps=T, tau_steps=1, g_steps=1, **over):
        a = dict(q="q", qd="qd", tau="tau", qd_next="qd_next", g_q="g_q", g_qd="g_qd", q_traj="q_traj", qd_traj="qd_traj", o0=0, o1=1, o2=2)
        a.update(over)
        p = {k: self.ptr(v) for k, v in a.items()}
        head = [self.plan._h if plan else None]
        if fn in INTEGRATE:
            args = head + [p["qd_next"], dt, p["g_q"], p["g_qd"], p["o0"], p["o1"], p["o2"]]
        elif fn in STEP:
            args = head + [p["q"], p["qd"], p["tau"], p["qd_next"], dt, p["g_q"], p["g_qd"], step, p["o0"], p["o1"], p["o2"]]
        else:
            args = head + [p["q"], p["qd"], p["q_traj"], p["qd_traj"], p["tau"], tau_steps, dt, n_steps, p["g_q"], p["g_qd"], g_steps, step,
                           p["o0"], p["o1"], p["o2"]]
        args += [self.B if B is None else B, 0]
        if "host" not in fn:
            args.append(None)
        return getattr(G.lib(), fn)(*args)


def _required(fn):
    return ("qd_next",) if fn in INTEGRATE else ("q", "qd", "tau", "qd_next") if fn in STEP else ("q", "qd", "q_traj", "qd_traj", "tau")


def _item(fn):
    return 4 if fn.endswith("f32") else 8


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_null_arguments_are_refused(fn):
    c = _Call()
    assert c(fn, plan=False) == EINVAL
    assert c(fn, plan=False, B=0) == EINVAL
    for name in _required(fn):
        assert c(fn, **{name: None}) == EINVAL, name
        assert c(fn, B=0, **{name: None}) == EINVAL, name
    assert c(fn, o0=None, o1=None, o2=None) == EINVAL  # any output may be null, not all three
    assert "no output" in G.lib().grbda_last_error().decode()
    assert c(fn, o0=None, o1=None, o2=None, B=0) == EINVAL
    assert c(fn, g_q=None, g_qd=None) == EINVAL        # either cotangent may be null, not both
    assert "cotangent" in G.lib().grbda_last_error().decode()
    assert c(fn, g_q=None, g_qd=None, B=0) == EINVAL


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_time_step_must_be_finite(fn):
    c = _Call()
    for dt in (float("nan"), float("inf"), -float("inf")):
        assert c(fn, dt=dt) == EINVAL, dt
        assert c(fn, dt=dt, B=0) == EINVAL
    assert "dt" in G.lib().grbda_last_error().decode()


@pytest.mark.parametrize("fn", ROLLOUT)
def test_the_step_counts_of_the_rollout_are_checked(fn):
    c = _Call()
    assert c(fn, n_steps=-1) == EINVAL and c(fn, n_steps=-1, tau_steps=-1, g_steps=-1) == EINVAL
    for bad in (0, 2, T + 1):
        assert c(fn, tau_steps=bad) == EINVAL, bad
        assert c(fn, g_steps=bad) == EINVAL, bad
        assert c(fn, g_steps=bad, B=0) == EINVAL
    assert c(fn, n_steps=0) == OK and c(fn, n_steps=0, tau_steps=0, g_steps=0) == OK  # (T == 0: nothing to do)
    assert c(fn, B=0, tau_steps=T, g_steps=T) == OK


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_overlapping_arguments_are_refused(fn):
    c = _Call()
    last = (c.B * c.nv - 1) * _item(fn)
    assert c(fn, o0=0, o1=0) == EINVAL                                   # the same array twice
    assert c(fn, o0=0, o2=c.out[0].ctypes.data + last) == EINVAL         # the last element of one is the first of the other
    for name in _required(fn) + ("g_q", "g_qd"):
        assert c(fn, o1=None, o2=None, o0=name) == EINVAL, name          # an output on an input
        assert c(fn, o0=None, o2=None, o1=name) == EINVAL, name
    assert c(fn, o0=None, o1=None, o2=c.g_qd.ctypes.data + last) == EINVAL
    if fn in ROLLOUT:  # (the arrays of T steps: their last block counts)
        block = c.B * c.nv * _item(fn)
        assert c(fn, o0=None, o1=None, o2=c.qd_traj.ctypes.data + (T - 1) * block) == EINVAL
        assert c(fn, o0=c.g_q.ctypes.data + (T - 1) * block, g_steps=T) == EINVAL
        assert c(fn, o0=c.tau.ctypes.data + (T - 1) * block, tau_steps=T) == EINVAL
        assert c(fn, o2=0, o1=None, o0=c.out[0].ctypes.data + (T - 1) * block, tau_steps=T) == EINVAL

@pytest.mark.parametrize("fn", STEP + ROLLOUT)
def test_the_step_is_checked_where_a_difference_route_needs_it(fn):
    c = _Call("tree65_fixed")  # 65 velocities: off the analytic route
    for step in (0.0, -1e-6, float("nan")):
        assert c(fn, step=step) == EINVAL, step
        assert c(fn, step=step, o1=None, o2=None) == EINVAL
    assert "step" in G.lib().grbda_last_error().decode()
    assert c(fn, step=0.0, B=0, o0=None, n_steps=1) == OK  # (no position gradient of any step: nothing needs the step)
    if fn in ROLLOUT:
        assert c(fn, step=0.0, o0=None) == EINVAL          # (T > 1: the steps hand their position gradient on)
    assert _Call()(fn, step=0.0, B=0) == OK                 # (the analytic route never uses the step)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
@pytest.mark.parametrize("model,why", [("four_bar", "implicit"), ("mini_cheetah_rpy", "roll-pitch-yaw")])
def test_plans_outside_the_contract_are_unsupported(fn, model, why):
    c = _Call(model)
    assert c(fn) == EUNSUPPORTED
    assert why in G.lib().grbda_last_error().decode()
    assert c(fn, B=0) == EUNSUPPORTED and c(fn, o0=None, o1=None) == EUNSUPPORTED


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_an_empty_batch_is_ok(fn):
    for model in ("tree16_fixed", "mini_cheetah"):
        c = _Call(model)
        assert c(fn, B=0) == OK
        assert c(fn, B=0, o0=None, o2=None, g_q=None) == OK
        assert c(fn, B=0, step=0.0) == OK


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_a_good_call_needs_a_device(fn):
    if G.device_count() > 0:
        pytest.skip("a HIP device is present")
    for model in ("tree16_fixed", "mini_cheetah", "tree65_fixed"):
        c = _Call(model)
        assert c(fn) == ENODEVICE
        assert c(fn, o0=None, o1=None, g_q=None) == ENODEVICE
        assert c(fn, tau_steps=T, g_steps=T) == ENODEVICE
    assert _Call("tree16_fixed")(fn, step=0.0) == ENODEVICE


def test_python_refuses_bad_arguments_before_the_library():
    import torch

    plan = G.Plan(blob_of("tree16_fixed"))
    z = torch.zeros((1, plan.nv), dtype=torch.float64)
    q = torch.zeros((1, plan.nq), dtype=torch.float64)
    zt, qt = z[None], q[None]
    calls = (lambda **k: plan.integrate_vjp(z, 0.01, **k), lambda **k: plan.step_vjp(q, z, z, z, 0.01, **k),
             lambda **k: plan.rollout_vjp(q, z, z, 0.01, qt, zt, **k))
    for call in calls:
        for want in ((), ("dq",), ("q", "H")):
            with pytest.raises(ValueError):
                call(g_q=z, want=want)
        with pytest.raises(ValueError):
            call()  # (both cotangents None)
        with pytest.raises(G.GrbdaError):  # (no CPU fallback)
            call(g_qd=z)
    with pytest.raises(ValueError):
        plan.step_vjp(q, z, z, z, 0.01, g_q=z, want=("q", "ydd"))
    with pytest.raises(ValueError):
        plan.integrate_vjp(z, 0.01, g_q=z, want=("tau",))


def test_a_position_gradient_needs_as_many_positions_as_velocities():
    import torch

    plan = G.Plan(blob_of("mini_cheetah"))
    assert plan.nq == plan.nv + 1
    q = torch.zeros((1, plan.nq), dtype=torch.float64, requires_grad=True)
    z = torch.zeros((1, plan.nv), dtype=torch.float64)
    with pytest.raises(ValueError, match="step_vjp"):
        plan.step_ad(q, z, z, 0.01)
    with pytest.raises(ValueError, match="rollout_vjp"):
        plan.rollout_ad(q, z, z, 0.01, 2)
