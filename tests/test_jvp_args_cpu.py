"""The Jacobian-vector products (include/grbda_hip_jvp.h) without a GPU, in the manner of test_vjp_args_cpu.py and
test_step_vjp_args_cpu.py: the symbols, the signature table JVP_SIGNATURES against the header parameter by parameter, the launch rule of the
contraction kernel, and the argument rules -- every refusal is decided before a device is looked at, so a machine without one answers
GRBDA_EINVAL / GRBDA_EUNSUPPORTED to a bad call and GRBDA_ENODEVICE only to a good one.  The arrays are host buffers standing in for device
arrays: the rules never read them, and no call that passes the rules is made where a device is present.

The order of the checks is pinned by calls that break two rules at once: a NULL plan before everything; a missing state input before the
tangents; the tangents before the outputs; the outputs before dt; dt before the overlap; the overlap before the plan; the plan before the
step."""
import ctypes
import os

import numpy as np
import pytest

import generalized_rbda_amd as G
import test_abi_table_cpu as abi
from generalized_rbda_amd._abi import JVP_SIGNATURES, SIGNATURES, STEP_VJP_SIGNATURES, VJP_SIGNATURES, WRENCH_SIGNATURES
from id_derivative_refs import blob_of

EINVAL, ENODEVICE, EUNSUPPORTED, OK = -1, -3, -2, 0
RNEA = ("grbda_rnea_jvp_f64", "grbda_rnea_jvp_f32", "grbda_rnea_jvp_host_f64")
ABA = ("grbda_aba_jvp_f64", "grbda_aba_jvp_f32", "grbda_aba_jvp_host_f64")
INTEGRATE = ("grbda_integrate_jvp_f64", "grbda_integrate_jvp_f32")
STEP = ("grbda_step_jvp_f64", "grbda_step_jvp_f32", "grbda_step_jvp_host_f64")
ENTRY_POINTS = RNEA + ABA + INTEGRATE + STEP
HEADER = os.path.join(os.path.dirname(abi.HEADER), "grbda_hip_jvp.h")


def _error():
    return G.lib().grbda_last_error().decode()


def test_the_symbols_are_exported_and_bound():
    L = ctypes.CDLL(G.LIB_PATH)
    for name in ENTRY_POINTS + ("grbda_jvp_contract_launch",):
        assert hasattr(L, name), name
        assert name in JVP_SIGNATURES and not any(name in t for t in (SIGNATURES, VJP_SIGNATURES, STEP_VJP_SIGNATURES, WRENCH_SIGNATURES))
    assert len(JVP_SIGNATURES) == len(ENTRY_POINTS) + 1 == 12
    for method in ("id_jvp", "fd_jvp", "integrate_jvp", "step_jvp"):
        assert callable(getattr(G.Plan, method))
    assert callable(G.jvp_contract_launch)


def test_the_first_header_keeps_its_count():
    assert len(SIGNATURES) == 96 and len(G.C_ABI_SYMBOLS) == 96


def test_the_table_declares_what_the_header_does(monkeypatch):
    monkeypatch.setattr(abi, "HEADER", HEADER)
    protos = abi.header_prototypes()
    assert set(protos) == set(ENTRY_POINTS) | {"grbda_jvp_contract_launch"}
    assert protos["grbda_rnea_jvp_f32"][1][7] == ("double", "step") and protos["grbda_aba_jvp_f64"][1][-3] == ("size_t", "B")
    assert protos["grbda_integrate_jvp_f32"][1][2] == ("double", "dt") and protos["grbda_step_jvp_f64"][1][9] == ("double", "step")
    assert [p for _, p in protos["grbda_step_jvp_host_f64"][1]][-1] == "device"
    abi.compare(JVP_SIGNATURES, protos)
    # (the comparison does fail on a defect: the step declared as a pointer)
    broken = dict(JVP_SIGNATURES)
    args = list(broken["grbda_aba_jvp_f64"][1])
    assert args[7] is ctypes.c_double
    args[7] = ctypes.c_void_p
    broken["grbda_aba_jvp_f64"] = (ctypes.c_int, tuple(args))
    with pytest.raises(AssertionError):
        abi.compare(broken, protos)


def test_the_loaded_library_carries_the_table(monkeypatch):
    monkeypatch.setattr(G, "_lib", None)  # (a fresh load)
    L = G.lib()
    for table in (JVP_SIGNATURES, STEP_VJP_SIGNATURES, VJP_SIGNATURES):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(argtypes), name
            assert fn.restype is restype, name
    assert len(L.grbda_rnea_jvp_f64.argtypes) == 12 and len(L.grbda_aba_jvp_host_f64.argtypes) == 12
    assert len(L.grbda_integrate_jvp_f32.argtypes) == 11 and len(L.grbda_step_jvp_f64.argtypes) == 15


class _Call:
    """one plan, host buffers of B states standing in for the arrays; an argument is the name of a buffer, an index into the outputs,
    None, or a raw address"""

    def __init__(self, model="tree16_fixed", B=3):
        self.plan = G.Plan(blob_of(model))
        nq, nv = self.plan.nq, self.plan.nv
        self.B, self.nv, self.nq = B, nv, nq
        z = lambda *shape: np.zeros(shape)
        self.q, self.qd, self.x, self.qd_next, self.dq, self.dqd, self.dx = z(B, nq), z(B, nv), z(B, nv), z(B, nv), z(B, nv), z(B, nv), z(B, nv)
        self.out = z(2, B, nv)

    def ptr(self, a):
        if a is None:
            return None
        if isinstance(a, str):
            return getattr(self, a).ctypes.data
        if isinstance(a, int) and 0 <= a < 2:
            return self.out[a].ctypes.data
        return a

    def __call__(self, fn, plan=True, B=None, dt=0.01, step=1e-6, **over):
        a = dict(q="q", qd="qd", x="x", qd_next="qd_next", dq="dq", dqd="dqd", dx="dx", o0=0, o1=1)
        a.update(over)
        p = {k: self.ptr(v) for k, v in a.items()}
        head = [self.plan._h if plan else None]
        if fn in RNEA:
            args = head + [p["q"], p["qd"], p["x"], p["dq"], p["dqd"], p["dx"], step, p["o0"]]
        elif fn in ABA:
            args = head + [p["q"], p["qd"], p["x"], p["dq"], p["dqd"], p["dx"], step, p["o0"], p["o1"]]
        elif fn in INTEGRATE:
            args = head + [p["qd_next"], dt, p["dq"], p["dqd"], p["dx"], p["o0"], p["o1"]]
        else:
            args = head + [p["q"], p["qd"], p["x"], p["qd_next"], dt, p["dq"], p["dqd"], p["dx"], step, p["o0"], p["o1"]]
        args += [self.B if B is None else B, 0]
        if "host" not in fn:
            args.append(None)
        return getattr(G.lib(), fn)(*args)


def _required(fn):
    return ("qd_next",) if fn in INTEGRATE else ("q", "qd", "x", "qd_next") if fn in STEP else ("q", "qd", "x")


def _no_output(fn):
    """the outputs that must not all be missing: the product itself (ydd of the forward side does not count), or both stepped tangents"""
    return dict(o0=None) if fn in RNEA + ABA else dict(o0=None, o1=None)


def _item(fn):
    return 4 if fn.endswith("f32") else 8


TANGENTS = ("dq", "dqd", "dx")
NO_TANGENT = dict(dq=None, dqd=None, dx=None)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_null_arguments_are_refused(fn):
    c = _Call()
    assert c(fn, plan=False) == EINVAL and "plan" in _error()
    assert c(fn, plan=False, B=0, **NO_TANGENT) == EINVAL and "plan" in _error()
    for name in _required(fn):
        assert c(fn, **{name: None}) == EINVAL, name
        assert c(fn, B=0, **{name: None}) == EINVAL, name
        assert c(fn, **{name: None}, **NO_TANGENT) == EINVAL and "null argument" in _error(), name  # (the state before the tangents)
    assert c(fn, **NO_TANGENT) == EINVAL and "tangents" in _error()
    assert c(fn, B=0, **NO_TANGENT) == EINVAL
    assert c(fn, **NO_TANGENT, **_no_output(fn)) == EINVAL and "tangents" in _error()  # (the tangents before the outputs)
    assert c(fn, **_no_output(fn)) == EINVAL and "no output" in _error()
    assert c(fn, B=0, **_no_output(fn)) == EINVAL
    for alone in TANGENTS:  # any tangent alone will do
        assert c(fn, B=0, **{k: None for k in TANGENTS if k != alone}) == OK, alone


@pytest.mark.parametrize("fn", INTEGRATE + STEP)
def test_either_stepped_tangent_may_be_left_out(fn):
    c = _Call()
    assert c(fn, B=0, o0=None) == OK and c(fn, B=0, o1=None) == OK


@pytest.mark.parametrize("fn", ABA)
def test_ydd_is_optional_and_is_no_output_of_its_own(fn):
    c = _Call()
    assert c(fn, B=0, o1=None) == OK
    assert c(fn, o0=None, o1=1) == EINVAL and "no output" in _error()


@pytest.mark.parametrize("fn", INTEGRATE + STEP)
def test_the_time_step_must_be_finite(fn):
    c = _Call()
    for dt in (float("nan"), float("inf"), -float("inf")):
        assert c(fn, dt=dt) == EINVAL, dt
        assert c(fn, dt=dt, B=0) == EINVAL
    assert "dt" in _error()
    assert c(fn, dt=float("nan"), **_no_output(fn)) == EINVAL and "no output" in _error()  # (the outputs before dt)
    assert c(fn, dt=float("nan"), o0=0, o1=0) == EINVAL and "dt" in _error()              # (dt before the overlap)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_overlapping_arguments_are_refused(fn):
    c = _Call()
    last = (c.B * c.nv - 1) * _item(fn)
    two = fn not in RNEA
    if two:
        assert c(fn, o0=0, o1=0) == EINVAL and "overlap" in _error()        # the same array twice
        assert c(fn, o0=0, o1=c.out[0].ctypes.data + last) == EINVAL        # the last element of one is the first of the other
    for name in _required(fn) + TANGENTS:
        assert c(fn, o0=name, o1=None) == EINVAL and "overlap" in _error(), name   # an output on an input
        assert c(fn, o0=getattr(c, name).ctypes.data + (getattr(c, name).size - 1) * _item(fn), o1=None) == EINVAL, name
        if two:
            assert c(fn, o1=name) == EINVAL, name


@pytest.mark.parametrize("fn", RNEA + ABA + STEP)
def test_the_step_is_checked_where_a_difference_route_needs_it(fn):
    c = _Call("tree65_fixed")  # 65 velocities: off the analytic route
    for step in (0.0, -1e-6, float("nan")):
        assert c(fn, step=step) == EINVAL, step
        assert c(fn, step=step, dqd=None, dx=None) == EINVAL
    assert "step" in _error()
    assert c(fn, step=0.0, B=0, dq=None) == OK   # (no position tangent, no difference in q: nothing needs the step)
    assert c(fn, step=0.0, o0=0, o1=0) == EINVAL and ("overlap" in _error() or fn in RNEA)  # (the overlap before the step)
    assert _Call()(fn, step=0.0, B=0) == OK        # (the analytic route never uses the step)


@pytest.mark.parametrize("fn", INTEGRATE + STEP)
@pytest.mark.parametrize("model,why", [("four_bar", "implicit"), ("mini_cheetah_rpy", "roll-pitch-yaw")])
def test_plans_outside_the_contract_of_the_step_are_unsupported(fn, model, why):
    c = _Call(model)
    assert c(fn) == EUNSUPPORTED and why in _error()
    assert c(fn, B=0) == EUNSUPPORTED and c(fn, o0=None, dq=None) == EUNSUPPORTED
    assert c(fn, o0=0, o1=0) == EINVAL and "overlap" in _error()   # (the overlap before the plan)
    if fn in STEP:
        assert c(fn, step=0.0) == EUNSUPPORTED                      # (the plan before the step)


@pytest.mark.parametrize("fn", RNEA + ABA)
@pytest.mark.parametrize("model", ["four_bar", "mini_cheetah_rpy", "mini_cheetah", "tree65_fixed"])
def test_the_dynamics_products_accept_every_plan_their_vjp_twins_accept(fn, model):
    c = _Call(model)
    assert c(fn, B=0) == OK and c(fn, B=0, dq=None, dx=None) == OK
    if G.device_count() == 0:
        assert c(fn) == ENODEVICE


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_an_empty_batch_is_ok(fn):
    for model in ("tree16_fixed", "mini_cheetah"):
        c = _Call(model)
        assert c(fn, B=0) == OK
        assert c(fn, B=0, o1=None, dq=None, dx=None) == OK
        assert c(fn, B=0, step=0.0) == OK


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_a_good_call_needs_a_device(fn):
    if G.device_count() > 0:
        pytest.skip("a HIP device is present")
    for model in ("tree16_fixed", "mini_cheetah", "tree65_fixed"):
        c = _Call(model)
        assert c(fn) == ENODEVICE
        assert c(fn, o1=None, dq=None, dqd=None) == ENODEVICE
        assert c(fn, step=0.0, dq=None) == ENODEVICE  # (no position tangent: the step is not looked at)
    assert _Call("tree16_fixed")(fn, step=0.0) == ENODEVICE


def test_python_refuses_bad_arguments_before_the_library():
    import torch

    plan = G.Plan(blob_of("tree16_fixed"))
    z = torch.zeros((1, plan.nv), dtype=torch.float64)
    q = torch.zeros((1, plan.nq), dtype=torch.float64)
    calls = (lambda **k: plan.id_jvp(q, z, z, **k), lambda **k: plan.fd_jvp(q, z, z, **k), lambda **k: plan.integrate_jvp(z, 0.01, **k),
             lambda **k: plan.step_jvp(q, z, z, z, 0.01, **k))
    for call in calls:
        with pytest.raises(ValueError):
            call()  # (all tangents None)
        with pytest.raises(G.GrbdaError) as e:  # (no CPU fallback)
            call(dqd=z)
        assert e.value.code == -3


def test_the_contraction_launch_rule():
    """units: packs of floor(64 / nv) states up to nv = 32, one state up to 64, blocks of 64 rows beyond; the grid: at most sixteen
    one-wavefront workgroups per CU, no more than the LDS of a CU holds tiles of, and at most one per unit"""
    launch = G.jvp_contract_launch
    units = lambda nv, B: launch(nv, B, 256)[0]
    assert [units(4, B) for B in (1, 16, 17, 70)] == [1, 1, 2, 5]              # sixteen states per unit
    assert [units(31, B) for B in (1, 2, 3, 5)] == [1, 1, 2, 3] and [units(32, B) for B in (2, 3, 5)] == [1, 2, 3]  # two per unit
    assert [units(33, B) for B in (1, 5)] == [1, 5] and [units(64, B) for B in (1, 70)] == [1, 70]                 # one per unit
    assert [units(65, B) for B in (1, 70)] == [2, 140] and units(128, 3) == 6 and units(129, 3) == 9               # blocks of 64 rows
    for nv in (4, 31, 32, 33, 64, 65, 128):
        for n_cu in (1, 256):
            cap = launch(nv, 1 << 40, n_cu)[1]  # the grid when there is no end of units
            assert n_cu <= cap <= 16 * n_cu and cap % n_cu == 0, (nv, n_cu, cap)
            u, g = launch(nv, 3, n_cu)
            assert g == min(u, cap)
    assert launch(4, 1 << 40, 256)[1] == 16 * 256  # (small tiles: the sixteen)
    assert launch(64, 1 << 40, 256)[1] < 16 * 256  # (a tile of 64 x 65 doubles: the LDS bounds it)
    for n_cu in (1, 8, 256):                       # the second trip
        grid = launch(4, 1 << 40, n_cu)[1]
        assert launch(4, 16 * grid, n_cu) == (grid, grid) and launch(4, 16 * grid + 1, n_cu) == (grid + 1, grid)
    assert G.lib().grbda_jvp_contract_launch(0, 1, 256, None, None) == EINVAL
    assert G.lib().grbda_jvp_contract_launch(4, 1, 0, None, None) == EINVAL
    assert G.lib().grbda_jvp_contract_launch(4, 1, 1, None, None) == OK
