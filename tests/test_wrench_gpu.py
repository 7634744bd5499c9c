"""Forward and inverse dynamics with sparse body wrenches (include/grbda_hip_wrench.h) on the device: parity with the oracle on the dense
f_ext of tests/wrench_ref.py (pinned to the oracle by test_wrench_ref_cpu.py), fp64 at 1e-9 and fp32 at 1e-3 with the inputs rounded to
float first, both frames, on the chain route and on every fallback; agreement with the dense entry point; n = 0; capture, streams, the host
variants and the Python argument rules.

The launch rule gives batches of a few tiles to latency mode, which carries no wrench hook (such a call falls back, and one test holds
that); the chain-route cases therefore build their plans under GRBDA_NO_LATENCY_MODE=1 and assert, through wrench_kernel_name, that a
wrench-carrying chain kernel is what runs."""
import functools

import numpy as np
import pytest

import generalized_rbda_amd as G
import oracle_py as O
import wrench_ref as W
from models import chain_test_tree, valid_states, zoo

pytestmark = pytest.mark.gpu

TOL64, TOL32 = 1e-9, 1e-3
B_MAX = 130
BATCHES = (1, 63, 64, 65, 130)


def rel_err(a, b):
    return np.abs(a - b).max() / (1 + np.abs(b).max())


@functools.lru_cache(maxsize=None)
def _model(name):
    """(blob, q, qd, x, places) with B_MAX states"""
    blob = chain_test_tree(31).serialize() if name == "chain_test_tree_31" else zoo()[name]
    q, qd, x = valid_states(blob, B_MAX, config_index=43)
    return blob, q, qd, x, W.tree_places(blob)


def _lists(name):
    """the body lists of a model, by name"""
    p = _model(name)[4]
    if name == "rev_pair_rotor_chain_4":
        return dict(first_pair=list(p["pairs"][0]), all_links=[b for pr in p["pairs"] for b in pr])
    on_chain = [p["base"]] + p["links"] + [b for pr in p["pairs"] for b in pr]
    sixteen = on_chain[:15] + [on_chain[3]]
    out = dict(base=[p["base"]], mid=[p["mid"][1]], tip=[p["tips"][0]], pair=list(p["pairs"][0]), sixteen=sixteen)
    if p["forks"]:
        out["fork"] = [p["forks"][0]]
    if name == "urdf_mit_humanoid":
        out["feet"] = [pr[1] for pr in p["pairs"]]
    return out


@functools.lru_cache(maxsize=None)
def _wrench(n):
    return np.random.default_rng(7).uniform(-5, 5, (B_MAX, n, 6))


def _round(a, f32):
    return a.astype(np.float32).astype(np.float64) if f32 else a


@functools.lru_cache(maxsize=None)
def _reference(name, bodies, frame, algo, f32):
    """the oracle on the dense forces of the (rounded) inputs, and the same without forces"""
    blob, q, qd, x, _ = _model(name)
    q, qd, x, w = (_round(a, f32) for a in (q, qd, x, _wrench(len(bodies))))
    fn = O.forward_dynamics if algo == "aba" else O.inverse_dynamics
    return fn(blob, q, qd, x, W.dense_f_ext(blob, q, list(bodies), w, frame)), fn(blob, q, qd, x)


def _tensors(gpu, dt, *arrays):
    import torch

    return [torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=gpu) for a in arrays]


def _run(plan, algo, name, bodies, frame, dt, gpu, B=B_MAX, **kw):
    _, q, qd, x, _ = _model(name)
    tq, tqd, tx, tw = _tensors(gpu, dt, q[:B], qd[:B], x[:B], _wrench(len(bodies))[:B])
    fn = plan.forward_dynamics_wrench if algo == "aba" else plan.inverse_dynamics_wrench
    return fn(tq, tqd, tx, bodies, tw, frame=frame, **kw)


def _check(plan, name, bodies, gpu, chain, B=B_MAX, frames=("body", "world"), algos=("aba", "rnea")):
    import torch

    for algo in algos:
        for frame in frames:
            for dt, tol in ((torch.float64, TOL64), (torch.float32, TOL32)):
                f32 = dt == torch.float32
                kname = plan.wrench_kernel_name(algo, "f32" if f32 else "f64", bodies, frame, B)
                # (chain=None: by the launch rule -- the chain route exactly where the plain call runs a one-wavefront chain kernel)
                expect = "_chain_kernel<" in plan.kernel_name(algo, "f32" if f32 else "f64", B) if chain is None else chain
                assert ("_chain_wrench_kernel<" in kname) == expect, (kname, algo, frame)
                if not expect:
                    assert kname.startswith(f"grbda_hip::{algo}_kernel<"), kname
                ref, free = _reference(name, tuple(bodies), frame, algo, f32)
                assert rel_err(free[:B], ref[:B]) > 1e-3  # the forces matter
                got = _run(plan, algo, name, bodies, frame, dt, gpu, B).double().cpu().numpy()
                err = rel_err(got, ref[:B])
                print(f"{name} {algo} {frame} {'f32' if f32 else 'f64'} B={B} n={len(bodies)}: {err:.3e} ({kname})")
                assert err < tol, (algo, frame, dt, err)


CHAIN_CASES = [(m, l) for m in ("chain_test_tree_31", "urdf_mit_humanoid") for l in ("base", "mid", "tip", "pair", "fork", "sixteen", "feet")
               if not (m == "urdf_mit_humanoid" and l == "fork") and not (m == "chain_test_tree_31" and l == "feet")]


@pytest.mark.parametrize("name,which", CHAIN_CASES)
def test_chain_route_matches_the_oracle(name, which, gpu, monkeypatch):
    monkeypatch.setenv("GRBDA_NO_LATENCY_MODE", "1")
    _check(G.Plan(_model(name)[0]), name, _lists(name)[which], gpu, chain=True)


@pytest.mark.parametrize("B", BATCHES)
def test_chain_route_at_every_batch(B, gpu, monkeypatch):
    monkeypatch.setenv("GRBDA_NO_LATENCY_MODE", "1")
    name = "chain_test_tree_31"
    lists = _lists(name)
    _check(G.Plan(_model(name)[0]), name, lists["base"] + lists["pair"] + lists["tip"], gpu, chain=True, B=B)


@pytest.mark.parametrize("which", ["first_pair", "all_links"])
def test_fixed_base_pair_chain_matches_the_oracle(which, gpu, monkeypatch):
    """rev_pair_rotor_chain_4: pairs on the ground and on pairs run as generic and differential segments -- off the chain route"""
    monkeypatch.setenv("GRBDA_NO_LATENCY_MODE", "1")
    name = "rev_pair_rotor_chain_4"
    _check(G.Plan(_model(name)[0]), name, _lists(name)[which], gpu, chain=False)


def test_fallbacks_match_the_oracle(gpu, monkeypatch):
    for name in ("tello_with_arms", "urdf_six_bar"):
        nb = G.Plan(_model(name)[0]).n_bodies
        _check(G.Plan(_model(name)[0]), name, [0, nb - 1, nb // 2, nb - 1], gpu, chain=False)
    name = "chain_test_tree_31"
    lists, rotor = _lists(name), _model(name)[4]["rotors"][0]
    plan = G.Plan(_model(name)[0])
    assert "_lm_kernel<" in plan.kernel_name("aba", "f32", B_MAX)  # latency mode serves three tiles, and carries no wrench hook
    _check(plan, name, lists["pair"], gpu, chain=None)
    monkeypatch.setenv("GRBDA_NO_LATENCY_MODE", "1")
    _check(G.Plan(_model(name)[0]), name, lists["mid"] + [rotor], gpu, chain=False)           # a rotor evaluated in closed form
    monkeypatch.setenv("GRBDA_NO_CHAIN", "1")
    _check(G.Plan(_model(name)[0]), name, lists["pair"], gpu, chain=False)


def test_world_frame_agrees_with_the_dense_entry_point_and_duplicates_add(gpu, monkeypatch):
    import torch

    monkeypatch.setenv("GRBDA_NO_LATENCY_MODE", "1")
    name = "chain_test_tree_31"
    blob, q, qd, x, p = _model(name)
    plan = G.Plan(blob)
    a, b = p["pairs"][0][1], p["mid"][0]
    w = _wrench(3)
    dense = np.zeros((B_MAX, plan.n_bodies, 6))
    dense[:, a] = w[:, 0] + w[:, 2]
    dense[:, b] = w[:, 1]
    summed = np.stack([w[:, 0] + w[:, 2], w[:, 1]], axis=1)
    for dt, tol in ((torch.float64, TOL64), (torch.float32, TOL32)):
        tq, tqd, tx, tw, tf, ts = _tensors(gpu, dt, q, qd, x, w, dense, summed)
        for sparse, full in ((plan.forward_dynamics_wrench, plan.forward_dynamics), (plan.inverse_dynamics_wrench, plan.inverse_dynamics)):
            want = full(tq, tqd, tx, f_ext=tf).double().cpu().numpy()
            assert rel_err(sparse(tq, tqd, tx, [a, b, a], tw, frame="world").double().cpu().numpy(), want) < tol
            for frame in ("body", "world"):
                twice = sparse(tq, tqd, tx, [a, b, a], tw, frame=frame).double().cpu().numpy()
                once = sparse(tq, tqd, tx, [a, b], ts, frame=frame).double().cpu().numpy()
                assert rel_err(twice, once) < tol, (frame, dt)


def test_no_bodies_is_the_plain_call_and_zero_wrenches_change_nothing(gpu, monkeypatch):
    import torch

    monkeypatch.setenv("GRBDA_NO_LATENCY_MODE", "1")
    name = "urdf_mit_humanoid"
    blob, q, qd, x, p = _model(name)
    plan = G.Plan(blob)
    three = [p["base"], p["pairs"][0][1], p["mid"][0]]
    for dt, tol in ((torch.float64, TOL64), (torch.float32, TOL32)):
        tq, tqd, tx = _tensors(gpu, dt, q, qd, x)
        zero = torch.zeros((B_MAX, 3, 6), dtype=dt, device=gpu)
        for sparse, full in ((plan.forward_dynamics_wrench, plan.forward_dynamics), (plan.inverse_dynamics_wrench, plan.inverse_dynamics)):
            plain = full(tq, tqd, tx)
            for frame in ("body", "world"):
                assert torch.equal(sparse(tq, tqd, tx, [], None, frame=frame), plain)
                assert rel_err(sparse(tq, tqd, tx, three, zero, frame=frame).double().cpu().numpy(), plain.double().cpu().numpy()) < tol
    assert plan.wrench_kernel_name("aba", "f32", [], "body", B_MAX) == plan.kernel_name("aba", "f32", B_MAX)


def test_capture_replay_and_a_caller_stream(gpu, monkeypatch):
    import torch
    from graph_capture import capture

    monkeypatch.setenv("GRBDA_NO_LATENCY_MODE", "1")
    name = "chain_test_tree_31"
    blob, q, qd, x, _ = _model(name)
    plan = G.Plan(blob)
    bodies = _lists(name)["pair"]
    dt = torch.float32
    tq, tqd, tx, tw = _tensors(gpu, dt, q, qd, x, _wrench(2))
    for frame in ("body", "world"):
        eager = plan.forward_dynamics_wrench(tq, tqd, tx, bodies, tw, frame=frame)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        on_side = plan.forward_dynamics_wrench(tq, tqd, tx, bodies, tw, frame=frame, stream=side)
        side.synchronize()
        assert torch.equal(on_side, eager), frame
        out = torch.empty_like(eager)
        cap = capture(lambda: plan.inverse_dynamics_wrench(tq, tqd, tx, bodies, tw, frame=frame, out=out))
        want = plan.inverse_dynamics_wrench(tq, tqd, tx, bodies, tw, frame=frame).clone()
        out.zero_()
        tw.mul_(2.0)  # new wrenches in the captured array: the replay must read them
        twice = plan.inverse_dynamics_wrench(tq, tqd, tx, bodies, tw, frame=frame).clone()
        torch.cuda.synchronize()
        got = cap.replay().clone()
        tw.mul_(0.5)
        cap.drop()
        assert torch.equal(got, twice) and not torch.equal(got, want), frame
    assert plan.release_work() >= 0


def test_host_variants_and_python_argument_rules(gpu, monkeypatch):
    import torch

    monkeypatch.setenv("GRBDA_NO_LATENCY_MODE", "1")
    name = "chain_test_tree_31"
    blob, q, qd, x, _ = _model(name)
    plan = G.Plan(blob)
    bodies = _lists(name)["pair"]
    B = 5
    w = _wrench(2)[:B]
    for frame in ("body", "world"):
        assert rel_err(plan.forward_dynamics_wrench_host(q[:B], qd[:B], x[:B], bodies, w, frame=frame),
                       _reference(name, tuple(bodies), frame, "aba", False)[0][:B]) < TOL64
        assert rel_err(plan.inverse_dynamics_wrench_host(q[:B], qd[:B], x[:B], bodies, w, frame=frame),
                       _reference(name, tuple(bodies), frame, "rnea", False)[0][:B]) < TOL64
    tq, tqd, tx, tw = _tensors(gpu, torch.float64, q[:B], qd[:B], x[:B], w)
    good = plan.forward_dynamics_wrench(tq, tqd, tx, bodies, tw)
    with pytest.raises(TypeError):
        plan.forward_dynamics_wrench(tq, tqd, tx, bodies, tw.float())
    with pytest.raises(G.GrbdaError):
        plan.forward_dynamics_wrench(tq, tqd, tx, bodies, tw.cpu())
    with pytest.raises(ValueError):
        plan.forward_dynamics_wrench(tq, tqd, tx, bodies, tw[:, :1])
    with pytest.raises(ValueError):
        plan.forward_dynamics_wrench(tq, tqd, tx, bodies + [0], tw)
    with pytest.raises(ValueError):
        plan.forward_dynamics_wrench(tq, tqd, tx, bodies, tw, out=torch.empty((B, 2 * plan.nv), dtype=torch.float64, device=gpu)[:, ::2])
    with pytest.raises(G.GrbdaError):
        plan.forward_dynamics_wrench(tq, tqd, tx, [plan.n_bodies, 0], tw)
    strided = torch.empty((B, 2, 12), dtype=torch.float64, device=gpu)[:, :, ::2]
    strided.copy_(tw)
    assert not strided.is_contiguous() and torch.equal(plan.forward_dynamics_wrench(tq, tqd, tx, bodies, strided), good)
