"""grbda_rnea_derivatives_* without a GPU: the symbols, the argument rules (checked before anything touches a device), and the
references the GPU test relies on -- the numpy statement of the analytic recursion against differences of the oracle's inverse dynamics
on the random trees of id_derivative_refs.py."""
import ctypes

import numpy as np
import pytest

import generalized_rbda_amd as G
from entry_points import _rel
from id_derivative_refs import RANDOM_TREES, blob_of, is_explicit, oracle_dq, oracle_dqd, recursion_refs, related_mask, states_of

EINVAL, ENODEVICE, OK = -1, -3, 0
SYMBOLS = ("grbda_rnea_derivatives_f64", "grbda_rnea_derivatives_f32", "grbda_rnea_derivatives_host_f64")


def test_the_symbols_exist_in_the_library_and_the_bindings():
    L = ctypes.CDLL(G.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in G.C_ABI_SYMBOLS
    assert callable(G.Plan.id_derivatives)


class _Call:
    """one plan, host buffers of B states standing in for the arrays (the argument rules never read them)"""

    def __init__(self, B=3):
        self.plan = G.Plan(blob_of("tree16_fixed"))
        nq, nv = self.plan.nq, self.plan.nv
        self.B, self.nn = B, nv * nv
        self.q, self.qd, self.ydd = np.zeros((B, nq)), np.zeros((B, nv)), np.zeros((B, nv))
        self.out = np.zeros((3, B, nv, nv))

    def __call__(self, fn_name, q="q", qd="qd", ydd="ydd", dq=0, dqd=1, dydd=2, B=None, plan=True):
        def ptr(a):
            if a is None:
                return None
            if isinstance(a, str):
                return getattr(self, a).ctypes.data
            if isinstance(a, int) and 0 <= a < 3:
                return self.out[a].ctypes.data
            return a  # a raw address

        fn = getattr(G.lib(), fn_name)
        args = [self.plan._h if plan else None, ptr(q), ptr(qd), ptr(ydd), 1e-6, ptr(dq), ptr(dqd), ptr(dydd), self.B if B is None else B, 0]
        if "host" not in fn_name:
            args.append(None)
        return fn(*args)


@pytest.mark.parametrize("fn", SYMBOLS)
def test_null_arguments_are_refused(fn):
    c = _Call()
    assert c(fn, plan=False) == EINVAL
    for name in ("q", "qd", "ydd"):
        assert c(fn, **{name: None}) == EINVAL, name
    assert c(fn, dq=None, dqd=None, dydd=None) == EINVAL  # any output may be null, not all three
    assert c(fn, dq=None, dqd=None, dydd=None, B=0) == EINVAL


@pytest.mark.parametrize("fn", SYMBOLS)
def test_overlapping_arguments_are_refused(fn):
    c = _Call()
    item = 4 if fn.endswith("f32") and "host" not in fn else 8
    assert c(fn, dq=0, dqd=0) == EINVAL                                         # the same array twice
    assert c(fn, dq=0, dydd=c.out[0].ctypes.data + (c.B * c.nn - 1) * item) == EINVAL   # the last element of one is the first of the other
    assert c(fn, dqd=None, dydd=None, dq=c.q.ctypes.data) == EINVAL             # an output on an input
    assert c(fn, dq=None, dydd=None, dqd=c.ydd.ctypes.data + (c.ydd.size - 1) * item) == EINVAL


@pytest.mark.parametrize("fn", SYMBOLS)
def test_an_empty_batch_is_ok(fn):
    c = _Call()
    assert c(fn, B=0) == OK
    assert c(fn, B=0, dq=None, dydd=None) == OK


@pytest.mark.parametrize("fn", SYMBOLS)
def test_a_real_call_needs_a_device(fn):
    if G.device_count() > 0:
        pytest.skip("a HIP device is present")
    c = _Call()
    assert c(fn) == ENODEVICE
    assert c(fn, dq=None, dqd=None) == ENODEVICE  # (H alone: the mass-matrix entry point)
    with pytest.raises(G.GrbdaError) as e:
        import torch

        z = torch.zeros((1, c.plan.nv), dtype=torch.float64)
        c.plan.id_derivatives(torch.zeros((1, c.plan.nq), dtype=torch.float64), z, z)
    assert e.value.code == ENODEVICE


@pytest.mark.parametrize("name", RANDOM_TREES)
def test_numpy_recursion_agrees_with_oracle_differences(name):
    """the analytic reference of the GPU test (deriv_recursion_numpy.rnea_derivs) against the difference references, on two states;
    and it is exactly zero where related_mask says two coordinates share no root path"""
    blob = blob_of(name)
    assert is_explicit(blob)
    idx = np.array([0, 69])
    s = {k: v[idx] for k, v in states_of(name).items()}
    dq, dqd = recursion_refs(blob, s, range(len(idx)))
    assert _rel(dqd, oracle_dqd(blob, s["q"], s["qd"], s["ydd"])) < 1e-8
    assert _rel(dq, oracle_dq(blob, s["q"], s["qd"], s["ydd"])) < 2e-5
    rel = related_mask(blob)
    assert not rel.all() and (rel == rel.T).all() and rel.diagonal().all()
    assert (dq[:, ~rel] == 0.0).all() and (dqd[:, ~rel] == 0.0).all()
