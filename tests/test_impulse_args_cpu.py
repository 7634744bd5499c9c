"""What grbda_contact_impulse_f64 / _f32 / _host_f64 refuse, on the host and before any device call (include/grbda_hip.h "contact
impulses").  No device is needed: a call that passes the argument checks answers GRBDA_ENODEVICE on a machine without one; on a machine
WITH a device those rows are not called (the arrays of this file are host memory).

One case per rule: a NULL plan, q, qd, qd_next, impulse, bodies, offsets; 0 and 9 contacts; body index -1 and n_bodies; damping negative,
NaN and infinite; restitution -0.1, 1.5, NaN and infinite; qd_next and impulse each aliasing each input, each other, and qd_next
overlapping qd by part of a row.  qd_next == qd (equal pointers) passes the checks, v_des == NULL passes, B == 0 returns GRBDA_OK."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_size_t, c_void_p

import pytest

import generalized_rbda_amd as G
from entry_points import _model

OK, EINVAL, ENODEVICE = 0, -1, -3
VARIANTS = ["grbda_contact_impulse_f64", "grbda_contact_impulse_f32", "grbda_contact_impulse_host_f64"]
N = 2


@pytest.fixture(scope="module")
def plan():
    return G.Plan(_model("urdf_mini_cheetah"))


def _call(plan, variant, B=1, **change):
    """(return code, error text) of the valid call of `variant` with `change` applied: one 8 KiB host array per pointer argument"""
    G.lib()
    L = ctypes.CDLL(G.LIB_PATH)  # a handle of its own: the argument types set here stay here
    L.grbda_last_error.restype = ctypes.c_char_p
    host = variant.endswith("host_f64")
    fn = getattr(L, variant)
    fn.argtypes = [c_void_p, c_void_p, c_void_p, c_int, POINTER(c_int), POINTER(c_double), c_void_p, c_double, c_double, c_void_p, c_void_p,
                   c_size_t, c_int] + ([] if host else [c_void_p])
    keep = {k: (c_double * 1024)() for k in ("q", "qd", "v_des", "qd_next", "impulse")}
    a = {k: ctypes.addressof(v) for k, v in keep.items()}
    a.update(handle=plan._h, n=N, bodies=[1, 2] + [1] * 7, offsets=(c_double * 27)(), restitution=0.0, damping=0.0)
    for k, v in change.items():
        a[k] = a[v[1:].rstrip("+")] + (8 if v.endswith("+") else 0) if isinstance(v, str) and v.startswith("=") else v
    bodies = None if a["bodies"] is None else (c_int * 9)(*a["bodies"])
    rc = fn(a["handle"], a["q"], a["qd"], a["n"], bodies, a["offsets"], a["v_des"], a["restitution"], a["damping"], a["qd_next"], a["impulse"], B, 0,
            *([] if host else [None]))
    return rc, (L.grbda_last_error().decode() if rc else "")


def test_the_symbols_exist_in_the_library_and_the_bindings(plan):
    for name in VARIANTS:
        assert name in G.C_ABI_SYMBOLS
        assert hasattr(G.lib(), name)
    assert callable(plan.contact_impulse)
    for sfx in ("f64", "f32"):
        assert len(getattr(G.lib(), "grbda_contact_impulse_" + sfx).argtypes) == 14


_NULL, _PLAN, _BODY = "null argument", "null plan", "body index out of range"
_IN, _OUT = "an output array overlaps an input array", "two output arrays overlap"
_DAMP, _REST, _COUNT = "damping must be finite and not negative", "restitution must lie in [0, 1]", "1..8 contact points per call"
REFUSED = [
    ("null-plan", dict(handle=None), _PLAN),
    ("null-q", dict(q=None), _NULL), ("null-qd", dict(qd=None), _NULL), ("null-qd_next", dict(qd_next=None), _NULL),
    ("null-impulse", dict(impulse=None), _NULL), ("null-bodies", dict(bodies=None), _NULL), ("null-offsets", dict(offsets=None), _NULL),
    ("n=0", dict(n=0), _COUNT), ("n=9", dict(n=9), _COUNT),
    ("body=-1", dict(bodies=[-1, 2] + [1] * 7), _BODY), ("body=n_bodies", dict(bodies=[1, "top"] + [1] * 7), _BODY),
    ("damping<0", dict(damping=-1.0), _DAMP), ("damping=nan", dict(damping=float("nan")), _DAMP), ("damping=inf", dict(damping=float("inf")), _DAMP),
    ("restitution=-0.1", dict(restitution=-0.1), _REST), ("restitution=1.5", dict(restitution=1.5), _REST),
    ("restitution=nan", dict(restitution=float("nan")), _REST), ("restitution=inf", dict(restitution=float("inf")), _REST),
    ("qd_next==q", dict(qd_next="=q"), _IN), ("qd_next==v_des", dict(qd_next="=v_des"), _IN),
    ("qd_next overlaps qd in part", dict(qd_next="=qd+"), _IN),
    ("impulse==q", dict(impulse="=q"), _IN), ("impulse==qd", dict(impulse="=qd"), _IN), ("impulse==v_des", dict(impulse="=v_des"), _IN),
    ("impulse==qd_next", dict(impulse="=qd_next"), _OUT),
    ("impulse==qd_next==qd", dict(qd_next="=qd", impulse="=qd"), _OUT),
]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rid,change,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_on_the_host(rid, change, text, variant, plan):
    if "bodies" in change and change["bodies"] is not None:
        change = dict(change, bodies=[plan.n_bodies if b == "top" else b for b in change["bodies"]])
    assert _call(plan, variant, **change) == (EINVAL, text)


PASSES = [("valid", {}), ("qd_next==qd", dict(qd_next="=qd")), ("null-v_des", dict(v_des=None)), ("restitution=1", dict(restitution=1.0)),
          ("restitution=0, damping=0", dict(restitution=0.0, damping=0.0))]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rid,change", PASSES, ids=[r[0] for r in PASSES])
def test_passes_the_argument_checks(rid, change, variant, plan):
    """past the checks the call looks for its device: without one it fails only with GRBDA_ENODEVICE"""
    if G.device_count() > 0:
        return  # (host arrays: not called on a machine with a device, as test_contact_args_cpu.py; test_impulse_gpu.py runs these calls there)
    rc, text = _call(plan, variant, **change)
    assert rc == ENODEVICE, (rc, text)


@pytest.mark.parametrize("variant", VARIANTS)
def test_empty_batch_is_ok(variant, plan):
    assert _call(plan, variant, B=0) == (OK, "")
    assert _call(plan, variant, B=0, qd_next="=qd") == (OK, "")
    # the argument rules hold for an empty batch too
    assert _call(plan, variant, B=0, restitution=1.5) == (EINVAL, _REST)
