"""The scheduled contacts (include/grbda_hip_contact_step.h) without a GPU: the symbols, their signature table against that header
parameter by parameter, and the argument rules -- every refusal is decided before a device is looked at, so a machine without one answers
GRBDA_EINVAL / GRBDA_EUNSUPPORTED to a bad call and GRBDA_ENODEVICE only to a good one.  The arrays are host buffers standing in for
device arrays: the rules never read them, and no call that passes the rules is made where a device is present."""
import ctypes
import os

import numpy as np
import pytest

import entry_points as EP
import generalized_rbda_amd as G
import test_abi_table_cpu as abi
from generalized_rbda_amd._abi import CONTACT_STEP_SIGNATURES, SIGNATURES, WRENCH_SIGNATURES
from id_derivative_refs import blob_of

EINVAL, EUNSUPPORTED, ENODEVICE, OK = -1, -2, -3, 0
HEADER = os.path.join(os.path.dirname(abi.HEADER), "grbda_hip_contact_step.h")
STEMS = ("contact_dynamics_active", "contact_impulse_active", "contact_step", "contact_rollout")
DEVICE_CALLS = tuple(f"grbda_{s}_{p}" for s in STEMS for p in ("f64", "f32"))
ENTRY_POINTS = DEVICE_CALLS + ("grbda_contact_step_host_f64",)


def test_the_symbols_are_exported_and_bound():
    L = ctypes.CDLL(G.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in CONTACT_STEP_SIGNATURES and name not in SIGNATURES and name not in WRENCH_SIGNATURES
    assert set(CONTACT_STEP_SIGNATURES) == set(ENTRY_POINTS)
    for method in ("contact_dynamics_active", "contact_impulse_active", "contact_step", "contact_rollout", "contact_step_host"):
        assert callable(getattr(G.Plan, method))
    assert G._ContactStepMethods in G.Plan.__mro__ and len(SIGNATURES) == 96


def test_the_table_declares_what_the_header_does(monkeypatch):
    monkeypatch.setattr(abi, "HEADER", HEADER)
    protos = abi.header_prototypes()
    assert set(protos) == set(CONTACT_STEP_SIGNATURES)
    names = lambda fn: [p for _, p in protos[fn][1]]
    assert names("grbda_contact_step_f32")[7:13] == ["active", "prev_active", "kd", "restitution", "damping", "dt"]
    assert protos["grbda_contact_rollout_f64"][1][16] == ("int", "T") and names("grbda_contact_rollout_f64")[9:12] == ["active_steps", "active_prev", "with_impulses"]
    assert names("grbda_contact_step_host_f64")[-1] == "device" and names("grbda_contact_step_f64")[-1] == "stream"
    abi.compare(CONTACT_STEP_SIGNATURES, protos)
    broken = dict(CONTACT_STEP_SIGNATURES)  # (the comparison does fail on a defect: kd declared as a pointer)
    args = list(broken["grbda_contact_step_f64"][1])
    args[9] = ctypes.c_void_p
    broken["grbda_contact_step_f64"] = (ctypes.c_int, tuple(args))
    with pytest.raises(AssertionError):
        abi.compare(broken, protos)


def test_the_loaded_library_carries_the_table(monkeypatch):
    monkeypatch.setattr(G, "_lib", None)  # (a fresh load)
    L = G.lib()
    for name, (restype, argtypes) in CONTACT_STEP_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(argtypes), name
        assert fn.restype is restype, name
    assert len(L.grbda_contact_step_f64.argtypes) == 22 and len(L.grbda_contact_rollout_f32.argtypes) == 25


class _Call:
    """one plan, host buffers of B states standing in for the arrays; every argument of every entry point by name"""

    def __init__(self, model="tree16_fixed", B=3, n=2, T=2):
        self.plan = G.Plan(EP._model(model) if model.startswith("urdf_") else blob_of(model))
        nq, nv = self.plan.nq, self.plan.nv
        self.B, self.n, self.T, self.nq, self.nv = B, n, T, nq, nv
        z = lambda *s: np.zeros(s)
        self.q, self.qd, self.tau, self.ydd, self.free = z(B, nq), z(B, nv), z(T, B, nv), z(B, nv), z(B, nv)
        self.q_next, self.qd_next, self.q_traj, self.qd_traj = z(B, nq), z(B, nv), z(T, B, nq), z(T, B, nv)
        self.des, self.lam, self.imp, self.lam_traj = z(B, 8, 3), z(B, 8, 3), z(B, 8, 3), z(T, B, 8, 3)
        self.active, self.prev, self.ok = np.zeros((T, B), dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)

    def __call__(self, fn, plan=True, bodies=(0, 1), offsets=True, **k):
        a = dict(q="q", qd="qd", tau="tau", active="active", prev="prev", des="des", ydd="ydd", lam="lam", free="free", imp="imp", q_next="q_next",
                 qd_next="qd_next", ok="ok", q_traj="q_traj", qd_traj="qd_traj", lam_traj="lam_traj", n=self.n, kd=0.0, e=0.0, mu=0.0, dt=0.01,
                 T=self.T, tau_steps=1, active_steps=1, with_impulses=1, B=self.B)
        a.update(k)
        p = lambda key: None if a[key] is None else getattr(self, a[key]).ctypes.data if isinstance(a[key], str) else a[key]
        bod = None if bodies is None else (ctypes.c_int * max(len(bodies), 1))(*bodies)
        off = (ctypes.c_double * 24)() if offsets else None
        c = (a["n"], bod, off)
        if "dynamics_active" in fn:
            args = [p("q"), p("qd"), p("tau"), *c, p("active"), p("des"), a["kd"], a["mu"], p("ydd"), p("lam"), p("free")]
        elif "impulse_active" in fn:
            args = [p("q"), p("qd"), *c, p("active"), p("des"), a["e"], a["mu"], p("qd_next"), p("imp")]
        elif "rollout" in fn:
            args = [p("q"), p("qd"), p("tau"), a["tau_steps"], *c, p("active"), a["active_steps"], p("prev"), a["with_impulses"], a["kd"], a["e"],
                    a["mu"], a["dt"], a["T"], p("ydd"), p("q_traj"), p("qd_traj"), p("lam_traj"), p("ok")]
        else:
            args = [p("q"), p("qd"), p("tau"), *c, p("active"), p("prev"), a["kd"], a["e"], a["mu"], a["dt"], p("ydd"), p("lam"), p("imp"),
                    p("q_next"), p("qd_next"), p("ok")]
        args += [a["B"], 0] + ([] if "host" in fn else [None])
        return getattr(G.lib(), fn)(self.plan._h if plan else None, *args)


def _err():
    return G.lib().grbda_last_error().decode()


def _required(fn):
    if "dynamics_active" in fn:
        return ("q", "qd", "tau", "active", "ydd", "lam")
    if "impulse_active" in fn:
        return ("q", "qd", "active", "qd_next", "imp")
    if "rollout" in fn:
        return ("q", "qd", "tau", "active", "ydd")
    return ("q", "qd", "tau", "active", "ydd", "lam", "q_next", "qd_next")


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_null_arguments_are_refused(fn):
    c = _Call()
    assert c(fn, plan=False) == EINVAL and "null plan" in _err()
    for name in _required(fn):
        assert c(fn, **{name: None}) == EINVAL and "null argument" in _err(), name
        assert c(fn, B=0, **{name: None}) == EINVAL, name
    assert c(fn, bodies=None) == EINVAL and c(fn, offsets=False) == EINVAL and "null argument" in _err()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_contacts_and_the_gains_are_checked(fn):
    c = _Call()
    nb = c.plan.n_bodies
    assert c(fn, n=0) == EINVAL and c(fn, n=9, bodies=(0,) * 9) == EINVAL and "1..8" in _err()
    assert c(fn, bodies=(0, nb)) == EINVAL and c(fn, bodies=(-1, 0)) == EINVAL and "body index" in _err()
    assert c(fn, n=1, bodies=(0, nb), B=0) == OK  # (only the first n entries are the list)
    for bad in (-1e-3, float("nan"), float("inf")):
        assert c(fn, mu=bad) == EINVAL and "damping" in _err(), bad
        if "impulse_active" not in fn:
            assert c(fn, kd=bad) == EINVAL and "kd must be" in _err(), bad
    if "dynamics_active" not in fn:
        for bad in (-0.1, 1.1, float("nan")):
            assert c(fn, e=bad) == EINVAL and "restitution" in _err(), bad
        assert c(fn, e=1.0, B=0) == OK
    if "step" in fn or "rollout" in fn:
        for bad in (float("nan"), float("inf")):
            assert c(fn, dt=bad) == EINVAL and "dt is not finite" in _err()


@pytest.mark.parametrize("fn", [f for f in ENTRY_POINTS if "rollout" in f])
def test_the_rollouts_counts_are_checked(fn):
    c = _Call(T=3)
    assert c(fn, T=-1) == EINVAL and "T is negative" in _err()
    assert c(fn, tau_steps=2) == EINVAL and "tau_steps" in _err()
    assert c(fn, active_steps=2) == EINVAL and "active_steps" in _err()
    assert c(fn, tau_steps=3, active_steps=3, B=0) == OK and c(fn, T=0) == OK and c(fn, T=0, tau_steps=0, active_steps=0) == OK
    for optional in ("prev", "q_traj", "qd_traj", "lam_traj", "ok"):
        assert c(fn, B=0, **{optional: None}) == OK, optional


@pytest.mark.parametrize("fn", [f for f in ENTRY_POINTS if "contact_step" in f])
def test_an_impulse_array_needs_prev_active(fn):
    c = _Call()
    assert c(fn, prev=None) == EINVAL and "impulse needs prev_active" in _err()
    assert c(fn, prev=None, imp=None, B=0) == OK and c(fn, imp=None, B=0) == OK and c(fn, ok=None, B=0) == OK


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_overlapping_arrays_are_refused(fn):
    c = _Call()
    item = 4 if fn.endswith("f32") else 8
    if "dynamics_active" in fn:
        pairs = [("ydd", "q"), ("ydd", "tau"), ("lam", "des"), ("free", "qd"), ("lam", "active"), ("free", "ydd")]
    elif "impulse_active" in fn:
        pairs = [("qd_next", "q"), ("imp", "des"), ("imp", "active"), ("imp", "qd_next")]
    elif "rollout" in fn:
        pairs = [("ydd", "tau"), ("q_traj", "q"), ("qd_traj", "active"), ("lam_traj", "qd"), ("ok", "prev"), ("q_traj", "qd_traj")]
    else:
        pairs = [("ydd", "q"), ("lam", "tau"), ("imp", "active"), ("q_next", "prev"), ("qd_next", "tau"), ("ok", "active"), ("q_next", "qd_next"),
                 ("ydd", "qd_next")]
    for out, other in pairs:
        assert c(fn, **{out: getattr(c, other).ctypes.data}) == EINVAL and "overlap" in _err(), (out, other)
    if "dynamics_active" in fn:  # the last element of tau's first block is the first of the output
        assert c(fn, ydd=c.tau.ctypes.data + (c.B * c.nv - 1) * item) == EINVAL
        assert c(fn, ydd=c.tau.ctypes.data + c.B * c.nv * item, B=0) == OK  # (right behind the block the call reads)
    if "impulse_active" in fn:
        assert c(fn, qd_next=c.qd.ctypes.data + item) == EINVAL
    if "contact_step" in fn:
        assert c(fn, q_next=c.q.ctypes.data + item) == EINVAL and "only q_next == q" in _err()
    # What is allowed passes every rule, so it is tried only where no device can take the host buffers for device arrays (on a device:
    # tests/test_contact_step_gpu.py, the in-place outputs).
    if G.device_count() == 0:
        if "dynamics_active" in fn:
            assert c(fn, ydd=c.tau.ctypes.data + c.B * c.nv * item) == ENODEVICE
        if "impulse_active" in fn:
            assert c(fn, qd_next="qd") == ENODEVICE
        if "contact_step" in fn:
            assert c(fn, q_next="q", qd_next="qd") == ENODEVICE


@pytest.mark.parametrize("fn", [f for f in ENTRY_POINTS if "step" in f or "rollout" in f])
def test_what_step_refuses_is_unsupported(fn):
    c = _Call("urdf_mini_cheetah_rpy")
    assert c(fn) == EUNSUPPORTED and "quaternion floating base only" in _err()
    assert c(fn, B=0) == EUNSUPPORTED


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_winner_of_two_broken_rules(fn):
    c = _Call("urdf_mini_cheetah_rpy")
    assert c(fn, q=None, n=9) == EINVAL and "null argument" in _err()            # a NULL array before the count
    assert c(fn, n=9, mu=-1.0, bodies=(0,) * 9) == EINVAL and "1..8" in _err()    # the contacts before the gains
    if "step" in fn or "rollout" in fn:
        assert c(fn, mu=-1.0) == EINVAL and "damping" in _err()                   # EINVAL of the gains before EUNSUPPORTED
        assert c(fn, dt=float("nan")) == EINVAL                                   # ... and so the time step
    if "rollout" in fn:
        assert c(fn, T=-1, tau_steps=5) == EINVAL and "T is negative" in _err()
    if "dynamics_active" in fn:
        assert c(fn, kd=-1.0, mu=-1.0) == EINVAL and "kd must be" in _err()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_an_empty_batch_is_ok_and_a_good_call_needs_a_device(fn):
    c = _Call()
    assert c(fn, B=0) == OK
    if G.device_count() == 0:
        assert c(fn) == ENODEVICE


def test_python_argument_rules_without_a_device():
    import torch

    plan = _Call().plan
    q, z = torch.zeros((2, plan.nq), dtype=torch.float64), torch.zeros((2, plan.nv), dtype=torch.float64)
    mask = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):  # (a host mask)
        plan.contact_dynamics_active(q, z, z, [0], [(0, 0, 0)], mask)
    with pytest.raises(ValueError):
        plan.contact_step(q, z, z, [0, 1], [(0, 0, 0)], mask, 0.01)
