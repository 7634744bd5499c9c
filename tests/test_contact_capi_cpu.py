"""The contact entry points of the C ABI without a device: the symbols exist, and everything grbda_contact_points_* /
grbda_contact_dynamics_* refuse is refused on the host, before a device is looked for (GRBDA_EINVAL with text in grbda_last_error());
B == 0 is GRBDA_OK.  What a valid call returns without a device is not asserted."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_size_t, c_void_p

import pytest

import generalized_rbda_amd as G
from entry_points import _model

OK, EINVAL = 0, -1
SYMBOLS = ["grbda_contact_points_f64", "grbda_contact_points_f32", "grbda_contact_dynamics_f64", "grbda_contact_dynamics_f32",
           "grbda_contact_points_host_f64", "grbda_contact_dynamics_host_f64"]


@pytest.fixture(scope="module")
def plan():
    return G.Plan(_model("urdf_mini_cheetah"))


@pytest.fixture(scope="module")
def arrays():
    """non-NULL dummy arrays, one per argument, large enough for B = 1 of the Mini Cheetah (never dereferenced: the calls are refused on
    the host)"""
    return {k: (c_double * 512)() for k in ("q", "qd", "tau", "ydd", "lam", "free", "pos", "vel", "acc", "a_des")}


def _ptr(a):
    return None if a is None else ctypes.cast(a, c_void_p)


def points(plan, a, n, bodies, B=1, outs=("pos", "vel", "acc")):
    L = G.lib()
    L.grbda_last_error.restype = ctypes.c_char_p
    bod = (c_int * max(len(bodies), 1))(*bodies)
    off = (c_double * 27)()
    o = [_ptr(a[k]) if k in outs else None for k in ("pos", "vel", "acc")]
    return L.grbda_contact_points_f64(plan._h, _ptr(a["q"]), _ptr(a["qd"]), _ptr(a["ydd"]), n, bod, off, o[0], o[1], o[2], B, 0, None)


def dynamics(plan, a, n, bodies, damping=0.0, B=1, ydd="ydd"):
    L = G.lib()
    L.grbda_last_error.restype = ctypes.c_char_p
    bod = (c_int * max(len(bodies), 1))(*bodies)
    off = (c_double * 27)()
    return L.grbda_contact_dynamics_f64(plan._h, _ptr(a["q"]), _ptr(a["qd"]), _ptr(a["tau"]), None, n, bod, off, _ptr(a["a_des"]), damping,
                                        _ptr(a[ydd]), _ptr(a["lam"]), _ptr(a["free"]), B, 0, None)


def _refused(rc):
    assert rc == EINVAL
    assert G.lib().grbda_last_error()


def test_symbols_exist():
    L = G.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name


@pytest.mark.parametrize("call", [points, dynamics], ids=["points", "dynamics"])
def test_contact_count_and_body_range(call, plan, arrays):
    _refused(call(plan, arrays, 0, []))
    _refused(call(plan, arrays, 9, [1] * 9))
    _refused(call(plan, arrays, 2, [1, plan.n_bodies]))
    _refused(call(plan, arrays, 1, [-1]))


def test_damping_must_be_finite_and_not_negative(plan, arrays):
    _refused(dynamics(plan, arrays, 1, [1], damping=-1.0))
    _refused(dynamics(plan, arrays, 1, [1], damping=float("nan")))
    _refused(dynamics(plan, arrays, 1, [1], damping=float("inf")))


def test_points_without_an_output(plan, arrays):
    _refused(points(plan, arrays, 1, [1], outs=()))


def test_outputs_must_not_alias_inputs(plan, arrays):
    _refused(dynamics(plan, arrays, 1, [1], ydd="tau"))
    _refused(dynamics(plan, arrays, 1, [1], ydd="lam"))


def test_null_required_pointers(plan, arrays):
    a = dict(arrays, q=None)
    _refused(points(plan, a, 1, [1]))
    _refused(dynamics(plan, a, 1, [1]))
    _refused(points(plan, dict(arrays, qd=None), 1, [1]))            # vel and acc need qd
    _refused(points(plan, dict(arrays, ydd=None), 1, [1]))           # acc needs ydd


def test_empty_batch_is_ok(plan, arrays):
    assert points(plan, arrays, 1, [1], B=0) == OK
    assert dynamics(plan, arrays, 1, [1], B=0) == OK
    L = G.lib()
    bod, off, p = (c_int * 1)(1), (c_double * 3)(), lambda k: _ptr(arrays[k])
    assert L.grbda_contact_points_host_f64(plan._h, p("q"), p("qd"), p("ydd"), 1, bod, off, p("pos"), p("vel"), p("acc"), 0, 0) == OK
    assert L.grbda_contact_dynamics_host_f64(plan._h, p("q"), p("qd"), p("tau"), None, 1, bod, off, None, 0.0, p("ydd"), p("lam"), None, 0,
                                             0) == OK
    assert L.grbda_contact_dynamics_host_f64(plan._h, p("q"), p("qd"), p("tau"), None, 1, bod, off, None, -1.0, p("ydd"), p("lam"), None, 1,
                                             0) == EINVAL
