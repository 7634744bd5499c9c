"""J v and J^T f at a listed few body frames (include/grbda_hip_jacobian_products.h) without a GPU: the symbols, the signature table against
that header parameter by parameter, and the argument rules -- every refusal is decided before a device is looked at, with its text in
grbda_last_error.  The arrays are host buffers standing in for device arrays: the rules never read them, and no call that passes the rules
is made where a device is present."""
import ctypes
import os

import numpy as np
import pytest

import generalized_rbda_amd as G
import test_abi_table_cpu as abi
from generalized_rbda_amd._abi import (BODIES_SIGNATURES, JACOBIAN_PRODUCT_SIGNATURES, JACOBIAN_SIGNATURES, JVP_SIGNATURES, SIGNATURES,
                                       STEP_VJP_SIGNATURES, VJP_SIGNATURES, WRENCH_SIGNATURES)
from id_derivative_refs import blob_of

EINVAL, ENODEVICE, OK = -1, -3, 0
BODY, WORLD = 0, 1
ENTRY_POINTS = ("grbda_frame_jacobian_products_f64", "grbda_frame_jacobian_products_f32", "grbda_frame_jacobian_products_host_f64")
HEADER = os.path.join(os.path.dirname(abi.HEADER), "grbda_hip_jacobian_products.h")


def _last_error():
    return G.lib().grbda_last_error().decode()


def test_the_symbols_are_exported_and_bound():
    L = ctypes.CDLL(G.LIB_PATH)
    assert len(JACOBIAN_PRODUCT_SIGNATURES) == 3 and set(JACOBIAN_PRODUCT_SIGNATURES) == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    others = (SIGNATURES, VJP_SIGNATURES, STEP_VJP_SIGNATURES, WRENCH_SIGNATURES, JVP_SIGNATURES, BODIES_SIGNATURES, JACOBIAN_SIGNATURES)
    assert len(others) == 7 and not any(set(JACOBIAN_PRODUCT_SIGNATURES) & set(t) for t in others)
    for method in ("frame_jacobian_products", "frame_jv", "frame_jtf", "frame_jacobian_products_host"):
        assert callable(getattr(G.Plan, method))


def test_the_table_declares_what_the_header_does(monkeypatch):
    monkeypatch.setattr(abi, "HEADER", HEADER)
    protos = abi.header_prototypes()
    assert set(protos) == set(JACOBIAN_PRODUCT_SIGNATURES)
    assert protos["grbda_frame_jacobian_products_f32"][1][4] == ("int", "n") and protos["grbda_frame_jacobian_products_f64"][1][7] == ("int", "frame")
    assert [p for _, p in protos["grbda_frame_jacobian_products_f64"][1]][1:4] == ["q", "v", "f"]
    assert [p for _, p in protos["grbda_frame_jacobian_products_f64"][1]][8:10] == ["Jv", "JTf"]
    assert [p for _, p in protos["grbda_frame_jacobian_products_host_f64"][1]][-1] == "device"
    abi.compare(JACOBIAN_PRODUCT_SIGNATURES, protos)
    broken = dict(JACOBIAN_PRODUCT_SIGNATURES)  # (the comparison does fail on a defect: n declared as a pointer)
    args = list(broken["grbda_frame_jacobian_products_f64"][1])
    args[4] = ctypes.c_void_p
    broken["grbda_frame_jacobian_products_f64"] = (ctypes.c_int, tuple(args))
    with pytest.raises(AssertionError):
        abi.compare(broken, protos)
    text = open(HEADER).read()  # the header states why the Jacobian walk's LDS budget covers this walk
    assert "18 saved + 6 n" in text and "saved < n" in text and "grbda_frame_jacobians_route()" in text


def test_the_loaded_library_carries_the_table(monkeypatch):
    monkeypatch.setattr(G, "_lib", None)  # (a fresh load)
    L = G.lib()
    for name, (restype, argtypes) in JACOBIAN_PRODUCT_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(argtypes), name
        assert fn.restype is restype, name
    assert len(L.grbda_frame_jacobian_products_f64.argtypes) == 13 and len(L.grbda_frame_jacobian_products_host_f64.argtypes) == 12


class _Call:
    """one plan, host buffers of B states standing in for the arrays"""

    def __init__(self, B=3, n=2):
        self.plan = G.Plan(blob_of("tree16_fixed"))
        nq, nv = self.plan.nq, self.plan.nv
        self.B, self.n = B, n
        self.q, self.v, self.f = np.zeros((B, nq)), np.zeros((B, nv)), np.zeros((B, 16, 6))
        self.Jv, self.JTf = np.full((B, 16, 6), 7.0), np.full((B, nv), 7.0)

    def __call__(self, fn, q="q", v="v", f="f", n=None, bodies=(0, 1), offsets=((0.1, 0.2, 0.3),) * 16, frame=BODY, Jv="Jv", JTf="JTf", B=None,
                 plan=True):
        ptr = lambda a: None if a is None else getattr(self, a).ctypes.data if isinstance(a, str) else a
        n = self.n if n is None else n
        arr = None if bodies is None else (ctypes.c_int * max(len(bodies), 1))(*bodies)
        off = None if offsets is None else (ctypes.c_double * (3 * len(offsets)))(*[x for o in offsets for x in o])
        args = [self.plan._h if plan else None, ptr(q), ptr(v), ptr(f), n, arr, off, frame, ptr(Jv), ptr(JTf), self.B if B is None else B, 0]
        if "host" not in fn:
            args.append(None)
        return getattr(G.lib(), fn)(*args)


def _item(fn):
    return 4 if fn.endswith("f32") else 8


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_null_arguments_are_refused(fn):
    c = _Call()
    assert c(fn, plan=False) == EINVAL and "null plan" in _last_error()
    for B in (None, 0):
        assert c(fn, q=None, B=B) == EINVAL and "null argument" in _last_error()
        assert c(fn, bodies=None, B=B) == EINVAL and "null argument" in _last_error()
        assert c(fn, v=None, f=None, Jv=None, JTf=None, B=B) == EINVAL and "no output" in _last_error()
        assert c(fn, Jv=None, JTf=None, B=B) == EINVAL and "no output" in _last_error()
        assert c(fn, v=None, B=B) == EINVAL and "Jv needs v" in _last_error()
        assert c(fn, v=None, f=None, JTf=None, B=B) == EINVAL and "Jv needs v" in _last_error()
        assert c(fn, f=None, B=B) == EINVAL and "JTf needs f" in _last_error()
        assert c(fn, v=None, f=None, Jv=None, B=B) == EINVAL and "JTf needs f" in _last_error()
        # both pointers of a pair are NULL, or neither is
        assert c(fn, Jv=None, B=B) == EINVAL and "without Jv" in _last_error()
        assert c(fn, JTf=None, B=B) == EINVAL and "without JTf" in _last_error()
    # what may be left out: either pair, the offsets
    assert c(fn, v=None, Jv=None, B=0) == OK and c(fn, f=None, JTf=None, B=0) == OK and c(fn, offsets=None, B=0) == OK


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_list_and_the_frame_are_checked(fn):
    c = _Call()
    n_bodies = c.plan.n_bodies
    assert c(fn, n=-1) == EINVAL and c(fn, n=17, bodies=tuple(range(16)) + (0,)) == EINVAL
    assert "0..16" in _last_error()
    assert c(fn, bodies=(0, n_bodies)) == EINVAL and c(fn, bodies=(-1, 0)) == EINVAL
    assert "body index" in _last_error()
    assert c(fn, n=1, bodies=(0, n_bodies), B=0) == OK  # (only the first n entries are the list)
    for frame in (-1, 2):
        assert c(fn, frame=frame) == EINVAL and c(fn, frame=frame, B=0) == EINVAL
        assert "frame must be GRBDA_WRENCH_BODY or GRBDA_WRENCH_WORLD" in _last_error()
    assert c(fn, frame=WORLD, B=0) == OK


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_overlapping_arguments_are_refused(fn):
    c = _Call()
    item, nv = _item(fn), c.plan.nv
    for out, per_state in (("Jv", c.n * 6), ("JTf", nv)):
        for name, in_per_state in (("q", c.plan.nq), ("v", nv), ("f", c.n * 6)):
            a = getattr(c, name)
            assert c(fn, **{out: a.ctypes.data}) == EINVAL, (out, name)
            # the input's last element (of the B states the call reads) is the output's first
            assert c(fn, **{out: a.ctypes.data + (c.B * in_per_state - 1) * item}) == EINVAL, (out, name)
            assert "overlaps an input" in _last_error()
        assert c(fn, **{out: c.q.ctypes.data - c.B * per_state * item + item}) == EINVAL  # the output's last element is the input's first
        assert c(fn, B=0, **{out: c.q.ctypes.data - c.B * per_state * item}) == OK       # (right in front of q)
    assert c(fn, JTf=c.Jv.ctypes.data) == EINVAL and "two output arrays overlap" in _last_error()
    assert c(fn, JTf=c.Jv.ctypes.data + (c.B * c.n * 6 - 1) * item) == EINVAL
    assert c(fn, v=None, Jv=None, JTf=c.v.ctypes.data, B=0) == OK  # (v is no input without Jv)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_an_empty_batch_or_list_is_ok_without_a_device(fn):
    c = _Call()
    assert c(fn, B=0) == OK and c(fn, B=0, n=16, bodies=(1,) * 16) == OK
    assert c(fn, n=0) == OK and c(fn, n=0, bodies=None, offsets=None, v=None, f=None, Jv=None, JTf=None) == OK
    assert c(fn, n=0, B=0, bodies=None, v=None, Jv=None, JTf=None) == OK
    assert (c.Jv == 7.0).all() and (c.JTf == 7.0).all()  # nothing written
    if G.device_count() == 0:  # a good call needs a device, and says so
        assert c(fn) == ENODEVICE and c(fn, frame=WORLD, v=None, Jv=None) == ENODEVICE


def test_python_argument_rules_without_a_device():
    import torch

    plan = _Call().plan
    q, z = torch.zeros((2, plan.nq), dtype=torch.float64), torch.zeros((2, plan.nv), dtype=torch.float64)
    f = torch.zeros((2, 2, 6), dtype=torch.float64)
    with pytest.raises(G.GrbdaError):  # (host tensors: no CPU fallback)
        plan.frame_jv(q, z, [0])
    with pytest.raises(G.GrbdaError):
        plan.frame_jtf(q, f, [0, 1])
    with pytest.raises(G.GrbdaError):
        plan.frame_jacobian_products(q, [0, 1], v=z, f=f, frame="world")
    with pytest.raises(ValueError):
        plan.frame_jacobian_products(q, [0], v=z, frame="base")
    with pytest.raises(ValueError):
        plan.frame_jacobian_products(q, [0])
    with pytest.raises(ValueError):
        plan.frame_jv(q, None, [0])
    with pytest.raises(ValueError):
        plan.frame_jtf(q, None, [0])
    with pytest.raises(ValueError):
        plan.frame_jacobian_products(q, [0, 1], v=z, offsets=[(0, 0, 0)])
    qn = np.zeros((2, plan.nq))
    with pytest.raises(ValueError):
        plan.frame_jacobian_products_host(qn, [0])
    with pytest.raises(ValueError):
        plan.frame_jacobian_products_host(qn, [0], v=np.zeros((2, plan.nv + 1)))
    with pytest.raises(ValueError):
        plan.frame_jacobian_products_host(qn, [0, 1], f=np.zeros((2, 1, 6)))
    with pytest.raises(ValueError):
        plan.frame_jacobian_products_host(qn, [0], v=np.zeros((2, plan.nv)), frame="base")
