"""Both ends of every coordinate-count bucket of the derivative pipeline, against the oracle.

The SPD solve and H^-1 = W^T W are compiled for 16 / 24 / 32 / 40 / 48 / 64 coordinates (minv_nvb, launch_spd_mfma, launch_spd_solve);
a model's H is padded with the identity up to its bucket.  Random trees of revolute and rotor clusters, floating and fixed base, with nv
at the TOP of a bucket (16, 24, 32, 40, 48, 64: no padding; 64 also meets nv <= 64 lanes and the 160 KiB of LDS with equality), at the
BOTTOM of the next (17, 25, 33, 41, 49: the most padding) and at 65, where the analytic route must hand over to the difference
batches -- plus the two models of test_fd_derivatives_wide_models (46, 63), which that test compares route against route only.

For nv <= 64: the default route, GRBDA_NO_MINV=1 and, in fp32, GRBDA_SOLVE_F64=1; B = 70 (a tile and a half: seventeen groups of four
and a half one) and B = 5 (one full group and a single state in the second), the first rows of one draw, inputs and outputs in the
guarded buffers of guarded.py.  fp64: d ydd / d tau and mass_matrix and fd_dtau on every state, d ydd / d qd on the tile and group
edges, against unit differences of the oracle's forward / inverse dynamics (exact: affine in tau and ydd, quadratic in qd) at 1e-8 of
1 + max |ref|; d ydd / d q against central differences of the oracle along the reference's tangent step (h = 1e-6) at the reference's
2e-5 on five states, the first and the last among them; H^-1 H = 1 to 1e-7.  fp32: against the fp64 result of the rounded inputs at 1e-3.

fp32 needs a well-conditioned H: every model has cond(H) <= 4.4e3 over its 70 states in the ORACLE (the two older wide models have
4.26e3 and 4.36e3 and pass fp32 at 1e-3), asserted below.  Seeds are 500 + nv; where that draw is worse conditioned (48 and 49
floating, 64 fixed, 65 floating: 5.6e3, 7.2e3, 7.8e3, 5.1e3) the first of 1500 + nv, 2500 + nv, ... that meets the bound."""
import functools

import numpy as np
import pytest

import generalized_rbda_amd as G
from entry_points import TOL32, _dq_oracle, _fd_columns, _mass_oracle, _rel, edge_states, run_guarded
from models import random_cluster_tree, valid_states

pytestmark = pytest.mark.gpu

COND_MAX = 4.4e3
B_FULL, B_SMALL = 70, 5
# (nv, floating) -> seed, cond(H) of the draw in the comment
SEEDS = {
    (16, True): 516, (16, False): 516,    # 2.5e2, 6.9e2
    (17, True): 517, (17, False): 517,    # 6.1e2, 3.5e2
    (24, True): 524, (24, False): 524,    # 1.4e3, 8.1e2
    (25, True): 525, (25, False): 525,    # 5.1e2, 9.4e2
    (32, True): 532, (32, False): 532,    # 1.1e3, 2.4e3
    (33, True): 533, (33, False): 533,    # 6.2e2, 1.7e3
    (40, True): 540, (40, False): 540,    # 2.0e3, 8.5e2
    (41, True): 541, (41, False): 541,    # 1.4e3, 1.7e3
    (48, True): 1548, (48, False): 548,   # 1.8e3, 1.8e3
    (49, True): 1549, (49, False): 549,   # 2.6e3, 1.8e3
    (64, True): 564, (64, False): 1564,   # 1.7e3, 1.6e3
    (65, True): 3565, (65, False): 565,   # 2.9e3, 2.2e3
}
MODELS = [(nv, fl, seed) for (nv, fl), seed in SEEDS.items()] + [(46, True, 31), (63, True, 32)]  # (the last two: the older wide models)
ROUTES = [("default", {}, "f64"), ("no_minv", {"GRBDA_NO_MINV": "1"}, "f64"),
          ("default", {}, "f32"), ("no_minv", {"GRBDA_NO_MINV": "1"}, "f32"), ("solve_f64", {"GRBDA_SOLVE_F64": "1"}, "f32")]
CASES = [(m, r) for m in MODELS for r in ROUTES if m[0] <= 64 or r[0] == "default"]


def _case_id(case):
    (nv, fl, seed), (route, env, dt) = case
    return f"nv{nv}-{'floating' if fl else 'fixed'}-s{seed}-{route}-{dt}"


@functools.lru_cache(maxsize=None)
def _blob(nv, floating, seed):
    return random_cluster_tree(seed, nv - 6 if floating else nv, floating=floating, kinds=("rev", "rotor")).serialize()


def _round(a, dt):
    return a if dt == "f64" else a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=4)
def _states(nv, floating, seed, dt):
    """the 70 states, rounded to the type"""
    q, qd, tau = (_round(a, dt) for a in valid_states(_blob(nv, floating, seed), B_FULL, config_index=91))
    return {"q": q, "qd": qd, "tau": tau, "q_start": q}


@functools.lru_cache(maxsize=None)
def _cond(nv, floating, seed, dt):
    return float(np.linalg.cond(_mass_oracle(_blob(nv, floating, seed), _states(nv, floating, seed, dt)["q"])).max())


@functools.lru_cache(maxsize=2)
def _oracle(nv, floating, seed):
    """the oracle's mass matrix and d ydd / d tau (every state), d ydd / d qd (tile and group edges) and d ydd / d q (five states)"""
    blob, s = _blob(nv, floating, seed), _states(nv, floating, seed, "f64")
    q, qd, tau = s["q"], s["qd"], s["tau"]
    ref = {"H": _mass_oracle(blob, q), "dtau": _fd_columns(blob, q, qd, tau, "dtau")}
    ref["i_dqd"] = np.union1d(edge_states(B_FULL, 2, seed), edge_states(B_SMALL, 0))
    ref["dqd"] = _fd_columns(blob, q[ref["i_dqd"]], qd[ref["i_dqd"]], tau[ref["i_dqd"]], "dqd")
    ref["i_dq"] = np.array([0, 2, B_SMALL - 1, 64, B_FULL - 1])
    ref["dq"] = _dq_oracle(blob, q[ref["i_dq"]], qd[ref["i_dq"]], tau[ref["i_dq"]])
    return ref


@functools.lru_cache(maxsize=2)
def _f64_of_rounded(nv, floating, seed, B, gpu):
    """the default route's fp64 result of the fp32-rounded inputs (that route is held against the oracle by this test's fp64 case)"""
    import torch

    s = {k: v[:B] for k, v in _states(nv, floating, seed, "f32").items()}
    return run_guarded(G.Plan(_blob(nv, floating, seed)), _all, s, torch.float64, gpu, 0)


def _plan(blob, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = G.Plan(blob)
    for k in env:
        monkeypatch.delenv(k)
    return plan


def _all(plan, x):
    d = plan.fd_derivatives(x["q"], x["qd"], x["tau"])
    return d["dq"], d["dqd"], d["dtau"], plan.mass_matrix(x["q"]), plan.fd_dtau(x["q"])


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_bucket_edges_match_the_oracle(case, gpu, monkeypatch):
    import torch

    (nv, floating, seed), (route, env, dt) = case
    blob = _blob(nv, floating, seed)
    plan = _plan(blob, env, monkeypatch)
    assert plan.nv == nv and plan.info().analytic_derivatives == (1 if nv <= 64 else 0)
    s70 = _states(nv, floating, seed, dt)
    if dt == "f32":
        cond = _cond(nv, floating, seed, dt)
        assert cond <= COND_MAX, f"cond(H) = {cond:.3g}: draw another seed for this size"
    for B in (B_FULL, B_SMALL):
        s = {k: v[:B] for k, v in s70.items()}
        dq, dqd, dtau, H, Hinv = run_guarded(plan, _all, s, torch.float64 if dt == "f64" else torch.float32, gpu, 0)
        assert dq.shape == dqd.shape == dtau.shape == H.shape == Hinv.shape == (B, nv, nv)
        if dt == "f64":
            ref = _oracle(nv, floating, seed)
            assert _rel(dtau, ref["dtau"][:B]) < 1e-8 and _rel(Hinv, ref["dtau"][:B]) < 1e-8 and _rel(H, ref["H"][:B]) < 1e-9
            i, at = ref["i_dqd"][ref["i_dqd"] < B], np.flatnonzero(ref["i_dqd"] < B)
            assert _rel(dqd[i], ref["dqd"][at]) < 1e-8
            i, at = ref["i_dq"][ref["i_dq"] < B], np.flatnonzero(ref["i_dq"] < B)
            assert len(i) >= 3 and i[-1] == B - 1
            assert _rel(dq[i], ref["dq"][at]) < 2e-5
            assert np.abs(Hinv @ H - np.eye(nv)).max() < 1e-7
        else:
            want = _f64_of_rounded(nv, floating, seed, B, gpu)
            for name, a, b in zip(("dq", "dqd", "dtau", "H", "Hinv"), (dq, dqd, dtau, H, Hinv), want):
                assert _rel(a, b) < TOL32, name
