"""grbda_rnea_derivatives_* on the GPU (run with -m gpu on an MI355X): d tau / d q, d tau / d qd, d tau / d ydd of the inverse dynamics.

Every call goes through entry_points.run_guarded: the outputs lie in arenas filled with NaN canaries, so a store outside an output, an
element left unwritten (the structural zeros the recursion never stores) and a changed input are all caught.  Batch sizes
id_derivative_refs.BATCHES are the first rows of one draw of 70 states per model: no full group of four states, the tail alone, one
group, a group and a tail state, a tile and a half.

fp64, every state: dydd against the oracle's mass matrix at 1e-9, dqd against unit central differences of the oracle's inverse dynamics
at 1e-8, dq against its central differences (h = 1e-6, along the reference's tangent step / the constraint manifold) at 2e-5, all
relative to 1 + max |ref|; on the analytic route also dq and dqd against the numpy recursion at 1e-9 on the tile and group edges, and
entries between coordinates that share no root path exactly 0.0.  fp32, every state: against this entry point's fp64 result of the
rounded inputs at 1e-3 (nothing is inverted, so no conditioning gate).  Models: id_derivative_refs.MODELS."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import generalized_rbda_amd as G
from entry_points import TOL32, TOL64, _host, _rel, edge_states, run_guarded, same_bits_np
from graph_capture import capture
from id_derivative_refs import BATCHES, MODELS, blob_of, is_explicit, oracle_dq, recursion_refs_of, refs_of, related_mask, states_of
from models import ROBOT_MODELS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dq", "dqd", "dydd")


def _plan(name):
    """the model's plan under its plan-time switches (entry_points.plan_for keeps plans by blob NAME: these are kept here)"""
    if name not in _plan.made:
        env = dict(MODELS[name][1])
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            _plan.made[name] = G.Plan(blob_of(name))
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return _plan.made[name]


_plan.made = {}


def _call(want=NAMES):
    return lambda plan, x: tuple(plan.id_derivatives(x["q"], x["qd"], x["ydd"], want=want).values())


def _dtype(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def _run(name, dt, B, gpu, want=NAMES):
    s = {k: v[:B] for k, v in states_of(name, dt).items()}
    return dict(zip([k for k in NAMES if k in want], run_guarded(_plan(name), _call(want), s, _dtype(dt), gpu, 0)))


_f64_of_rounded = {}


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", list(MODELS))
def test_matches_the_oracle_at_every_batch_size(name, dt, gpu):
    blob, analytic = blob_of(name), MODELS[name][2]
    plan = _plan(name)
    nv = plan.nv
    # (the analytic route of this entry point: explicit clusters, nv <= 64 -- implicit models report analytic_derivatives = 1 for the
    # manifold route of the forward-dynamics derivatives and take the difference batches here)
    assert (plan.info().analytic_derivatives == 1 and is_explicit(blob)) == analytic
    unrelated = ~related_mask(blob)
    for B in BATCHES:
        got = _run(name, dt, B, gpu)
        assert all(got[k].shape == (B, nv, nv) for k in NAMES)
        if dt == "f64":
            ref = refs_of(name)
            err = {k: _rel(got[k], ref[k][:B]) for k in NAMES}
            print(f"{name} f64 B={B}: dydd {err['dydd']:.2e} dqd {err['dqd']:.2e} dq {err['dq']:.2e}")
            assert err["dydd"] < 1e-9 and err["dqd"] < 1e-8 and err["dq"] < 2e-5, err
            if analytic:
                idx = edge_states(B, 2, seed=B)
                rq, rqd = recursion_refs_of(name, idx)
                e2 = (_rel(got["dq"][idx], rq), _rel(got["dqd"][idx], rqd))
                print(f"    against the numpy recursion on states {idx.tolist()}: dq {e2[0]:.2e} dqd {e2[1]:.2e}")
                assert e2[0] < TOL64 and e2[1] < TOL64, e2
        else:
            if (name, B) not in _f64_of_rounded:
                s = {k: v[:B] for k, v in states_of(name, "f32").items()}
                _f64_of_rounded[name, B] = dict(zip(NAMES, run_guarded(plan, _call(), s, _dtype("f64"), gpu, 0)))
            want = _f64_of_rounded[name, B]
            for k in NAMES:
                per_state = np.abs(got[k] - want[k]).reshape(B, -1).max(axis=1) / (1.0 + np.abs(want[k]).max())
                print(f"{name} f32 B={B} {k}: worst state {per_state.max():.2e}")
                assert (per_state < TOL32).all(), (k, per_state.max())
        if analytic:
            for k in NAMES:
                assert (got[k][:, unrelated] == 0.0).all(), f"{k}: a structural zero is not exactly 0.0"


def test_consistent_with_the_forward_dynamics_derivatives(gpu):
    """Mini Cheetah, fp64, B = 70, ydd = FD(q, qd, tau): d ydd / d q = -H^-1 d tau / d q and the same for qd at 1e-8; d tau / d ydd has
    the bits of mass_matrix(q) (it is that entry point)"""
    import torch

    plan, s = _plan("mini_cheetah"), states_of("mini_cheetah")
    q, qd, tau = (torch.as_tensor(s[k], dtype=torch.float64, device=gpu) for k in ("q", "qd", "ydd"))
    ydd = plan.forward_dynamics(q, qd, tau)
    fd = plan.fd_derivatives(q, qd, tau)
    idd = plan.id_derivatives(q, qd, ydd)
    H = plan.mass_matrix(q)
    torch.cuda.synchronize()
    fd, idd, H = {k: v.cpu().numpy() for k, v in fd.items()}, {k: v.cpu().numpy() for k, v in idd.items()}, H.cpu().numpy()
    for k in ("dq", "dqd"):
        err = _rel(fd[k], -(fd["dtau"] @ idd[k]))
        print(f"fd {k} against -H^-1 id {k}: {err:.2e}")
        assert err < 1e-8, k
    assert np.array_equal(idd["dydd"], H)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["mini_cheetah", "tree45_fixed", "mini_cheetah_no_analytic"])
def test_every_subset_of_the_outputs_has_the_bits_of_the_full_call(name, dt, gpu):
    B = 7  # a group and a tail of three
    full = _run(name, dt, B, gpu)
    for n in (1, 2):
        for want in itertools.combinations(NAMES, n):
            got = _run(name, dt, B, gpu, want)
            assert list(got) == list(want)
            for k in want:
                assert np.array_equal(got[k], full[k]), f"{k} of want={want} differs from the call for all three"


def test_position_derivative_follows_gravity(gpu):
    """after set_gravity the analytic d tau / d q is that of the new gravity (read at launch): oracle differences on the plan's blob"""
    blob = blob_of("mini_cheetah")
    plan = G.Plan(blob)
    plan.set_gravity((1.0, -2.0, -7.0))
    s = {k: v[:5] for k, v in states_of("mini_cheetah").items()}
    dq, = run_guarded(plan, _call(("dq",)), s, _dtype("f64"), gpu, 0)
    ref = oracle_dq(plan.blob, s["q"], s["qd"], s["ydd"])
    assert _rel(ref, refs_of("mini_cheetah")["dq"][:5]) > 1e-3  # (the gravity matters to the reference)
    err = _rel(dq, ref)
    print(f"dq at gravity (1, -2, -7): {err:.2e}")
    assert err < 2e-5


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,B", [("mini_cheetah", 70), ("tree45_fixed", 7), ("four_bar", 37), ("mini_cheetah_no_analytic", 37)])
def test_a_captured_call_replays_the_bits_of_the_eager_call(name, B, dt, gpu):
    import torch

    plan = _plan(name)
    x = {k: torch.as_tensor(v[:B], dtype=_dtype(dt), device=gpu) for k, v in states_of(name, dt).items()}
    cap = capture(lambda: _call()(plan, x))
    try:
        assert cap.nodes["kernel"] >= 1
        # (new inputs in place: the states in reverse order)
        for k in x:
            x[k].copy_(x[k].flip(0))
        got = _host(cap.replay())
        with torch.cuda.stream(cap.stream):
            want = _host(_call()(plan, x))
        cap.stream.synchronize()
        assert same_bits_np(got, want)
        assert all(np.isfinite(a).all() for a in got)
    finally:
        cap.drop()


def test_cpp_facade_overloads_match_the_c_abi(tmp_path):
    """ClusterTreeModel<double>::inverseDynamicsDerivativesBatch on host arrays and on device arrays against grbda_rnea_derivatives_f64
    (tests/cpp/id_derivatives_facade_test.cpp, built the way test_urdf_and_facade.py builds the device mode of the facade test)"""
    out = tmp_path / "id_derivatives_facade_test"
    lib_dir = os.path.join(ROOT, "generalized_rbda_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I/opt/rocm/include", "-I" + os.path.join(lib_dir, "include"),
                    os.path.join(ROOT, "tests", "cpp", "id_derivatives_facade_test.cpp"), "-o", str(out), "-L" + lib_dir, "-lgrbda_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(out), os.path.join(ROBOT_MODELS, "mini_cheetah.urdf")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
