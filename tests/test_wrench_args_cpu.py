"""The sparse body wrenches (include/grbda_hip_wrench.h) without a GPU: the symbols, the fourth signature table against that header
parameter by parameter, and the argument rules -- every refusal is decided before a device is looked at, so a machine without one answers
GRBDA_EINVAL to a bad call and GRBDA_ENODEVICE only to a good one.  The arrays are host buffers standing in for device arrays: the rules
never read them, and no call that passes the rules is made where a device is present."""
import ctypes
import os

import numpy as np
import pytest

import generalized_rbda_amd as G
import test_abi_table_cpu as abi
from generalized_rbda_amd._abi import SIGNATURES, STEP_VJP_SIGNATURES, VJP_SIGNATURES, WRENCH_SIGNATURES
from id_derivative_refs import blob_of

EINVAL, ENODEVICE, OK = -1, -3, 0
BODY, WORLD = 0, 1
DEVICE_CALLS = ("grbda_aba_wrench_f64", "grbda_aba_wrench_f32", "grbda_rnea_wrench_f64", "grbda_rnea_wrench_f32")
HOST_CALLS = ("grbda_aba_wrench_host_f64", "grbda_rnea_wrench_host_f64")
ENTRY_POINTS = DEVICE_CALLS + HOST_CALLS
WRENCH_HEADER = os.path.join(os.path.dirname(abi.HEADER), "grbda_hip_wrench.h")


def test_the_symbols_are_exported_and_bound():
    L = ctypes.CDLL(G.LIB_PATH)
    for name in ENTRY_POINTS + ("grbda_wrench_kernel_name",):
        assert hasattr(L, name), name
        assert name in WRENCH_SIGNATURES and name not in SIGNATURES
    for method in ("forward_dynamics_wrench", "inverse_dynamics_wrench", "wrench_kernel_name", "forward_dynamics_wrench_host",
                   "inverse_dynamics_wrench_host"):
        assert callable(getattr(G.Plan, method))


def test_the_other_tables_keep_their_sizes():
    assert len(SIGNATURES) == 96 and len(VJP_SIGNATURES) == 7 and len(STEP_VJP_SIGNATURES) == 7 and len(WRENCH_SIGNATURES) == 7
    assert not set(WRENCH_SIGNATURES) & (set(SIGNATURES) | set(VJP_SIGNATURES) | set(STEP_VJP_SIGNATURES))


def test_the_fourth_table_declares_what_the_fourth_header_does(monkeypatch):
    monkeypatch.setattr(abi, "HEADER", WRENCH_HEADER)
    protos = abi.header_prototypes()
    assert set(protos) == set(WRENCH_SIGNATURES)
    assert protos["grbda_aba_wrench_f32"][1][4] == ("int", "n") and protos["grbda_aba_wrench_f32"][1][7] == ("int", "frame")
    assert [p for _, p in protos["grbda_rnea_wrench_host_f64"][1]][-1] == "device"
    abi.compare(WRENCH_SIGNATURES, protos)
    broken = dict(WRENCH_SIGNATURES)  # (the comparison does fail on a defect: the frame declared as a pointer)
    args = list(broken["grbda_aba_wrench_f64"][1])
    args[7] = ctypes.c_void_p
    broken["grbda_aba_wrench_f64"] = (ctypes.c_int, tuple(args))
    with pytest.raises(AssertionError):
        abi.compare(broken, protos)
    text = open(WRENCH_HEADER).read()
    assert "TreeModel::setExternalForces" in text and "#define GRBDA_WRENCH_BODY 0" in text and "#define GRBDA_WRENCH_WORLD 1" in text


def test_the_loaded_library_carries_the_fourth_table(monkeypatch):
    monkeypatch.setattr(G, "_lib", None)  # (a fresh load)
    L = G.lib()
    for name, (restype, argtypes) in WRENCH_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(argtypes), name
        assert fn.restype is restype, name
    assert len(L.grbda_aba_wrench_f64.argtypes) == 12 and len(L.grbda_rnea_wrench_host_f64.argtypes) == 11


class _Call:
    """one plan, host buffers of B states standing in for the arrays"""

    def __init__(self, B=3, n=2):
        self.plan = G.Plan(blob_of("tree16_fixed"))
        nq, nv = self.plan.nq, self.plan.nv
        self.B, self.nv, self.n = B, nv, n
        self.q, self.qd, self.x, self.out = np.zeros((B, nq)), np.zeros((B, nv)), np.zeros((B, nv)), np.zeros((B, nv))
        self.w = np.zeros((B, 16, 6))

    def __call__(self, fn, q="q", qd="qd", x="x", n=None, bodies=(0, 1), w="w", frame=BODY, out="out", B=None, plan=True):
        ptr = lambda a: None if a is None else getattr(self, a).ctypes.data if isinstance(a, str) else a
        n = self.n if n is None else n
        arr = None if bodies is None else (ctypes.c_int * max(len(bodies), 1))(*bodies)
        args = [self.plan._h if plan else None, ptr(q), ptr(qd), ptr(x), n, arr, ptr(w), frame, ptr(out), self.B if B is None else B, 0]
        if "host" not in fn:
            args.append(None)
        return getattr(G.lib(), fn)(*args)


def _item(fn):
    return 4 if fn.endswith("f32") and "host" not in fn else 8


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_null_arguments_are_refused(fn):
    c = _Call()
    assert c(fn, plan=False) == EINVAL
    for name in ("q", "qd", "x", "out"):
        assert c(fn, **{name: None}) == EINVAL, name
        assert c(fn, B=0, **{name: None}) == EINVAL, name
    assert c(fn, w=None) == EINVAL and c(fn, bodies=None) == EINVAL
    assert c(fn, w=None, B=0) == EINVAL


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_list_and_the_frame_are_checked(fn):
    c = _Call()
    n_bodies = c.plan.n_bodies
    assert c(fn, n=-1) == EINVAL and c(fn, n=17, bodies=tuple(range(16)) + (0,)) == EINVAL
    assert "0..16" in G.lib().grbda_last_error().decode()
    assert c(fn, bodies=(0, n_bodies)) == EINVAL and c(fn, bodies=(-1, 0)) == EINVAL
    assert "body index" in G.lib().grbda_last_error().decode()
    assert c(fn, frame=2) == EINVAL and c(fn, frame=-1) == EINVAL
    assert "frame" in G.lib().grbda_last_error().decode()
    assert c(fn, n=1, bodies=(0, n_bodies), B=0) == OK  # (only the first n entries are the list)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_overlapping_arguments_are_refused(fn):
    c = _Call()
    last = (c.B * c.nv - 1) * _item(fn)
    for name in ("q", "qd", "x", "w"):
        assert c(fn, out=getattr(c, name).ctypes.data) == EINVAL, name
    assert c(fn, out=c.x.ctypes.data + last) == EINVAL                          # the last element of tau is the first of the output
    assert c(fn, out=c.w.ctypes.data + (c.B * c.n * 6 - 1) * _item(fn)) == EINVAL
    assert "overlaps" in G.lib().grbda_last_error().decode()
    assert c(fn, out=c.w.ctypes.data + c.B * c.n * 6 * _item(fn), B=0) == OK   # (right behind the wrenches of this n)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_an_empty_batch_or_list_is_ok_up_to_the_device(fn):
    c = _Call()
    assert c(fn, B=0) == OK and c(fn, B=0, frame=WORLD) == OK
    assert c(fn, B=0, n=0, bodies=None, w=None) == OK
    assert c(fn, B=0, n=16, bodies=(1,) * 16) == OK
    if G.device_count() == 0:  # a good call needs a device, and says so
        assert c(fn) == ENODEVICE and c(fn, frame=WORLD) == ENODEVICE
        assert c(fn, n=0, bodies=None, w=None) == ENODEVICE


def test_the_kernel_name_call_checks_its_arguments():
    c = _Call()
    buf = ctypes.create_string_buffer(64)
    name = lambda **k: G.lib().grbda_wrench_kernel_name(*[{**dict(plan=c.plan._h, algo=0, precision=32, n=1, bodies=(ctypes.c_int * 1)(0), frame=BODY,
                                                                   B=64, device=0, buf=buf, cap=64), **k}[a]
                                                          for a in ("plan", "algo", "precision", "n", "bodies", "frame", "B", "device", "buf", "cap")])
    for bad in (dict(plan=None), dict(algo=2), dict(precision=16), dict(n=17), dict(n=-1), dict(bodies=None), dict(frame=3), dict(buf=None),
                dict(cap=0), dict(bodies=(ctypes.c_int * 1)(c.plan.n_bodies))):
        assert name(**bad) == EINVAL, bad
    if G.device_count() == 0:
        assert name() == ENODEVICE


def test_python_argument_rules_without_a_device():
    import torch

    plan = _Call().plan
    q, z = torch.zeros((2, plan.nq), dtype=torch.float64), torch.zeros((2, plan.nv), dtype=torch.float64)
    w = torch.zeros((2, 1, 6), dtype=torch.float64)
    for method in (plan.forward_dynamics_wrench, plan.inverse_dynamics_wrench):
        with pytest.raises(ValueError):
            method(q, z, z, [0], w, frame="local")
        with pytest.raises(G.GrbdaError):  # (host tensors: no CPU fallback)
            method(q, z, z, [0], w)
    with pytest.raises(ValueError):
        plan.forward_dynamics_wrench_host(q.numpy(), z.numpy(), z.numpy(), [0, 1], w.numpy())
