"""Poses and twists of a listed few bodies on the GPU (include/grbda_hip_bodies.h; run with -m gpu on an MI355X).

Slot i of a result is held to row bodies[i] of the CPU references the full kernels are held to -- oracle_py.body_poses and
kinematics_ref.body_twists (test_kinematics_ref_cpu.py pins it to the oracle) -- at the project's bounds, fp64 1e-9 and fp32 1e-3, as
max |got - ref| / (1 + max |ref|) over the batch; fp32 runs on float32-rounded states, which the reference is then fed.  Twists run at
nonzero qd and ydd and at an oblique gravity set through grbda_plan_set_gravity; the references read plan.blob, which carries it.

Batches 1, 63, 64, 65, 130: one state; a ragged tile; a full one; a tile and a state; two tiles and a ragged third, whose first two lanes were
busy and whose others idle.  Lists per model (lists()): one leaf; two leaves either side of a branch, the higher index first; a body with
its ancestor; a body twice among others; the first body alone; a rotor; the longest lists -- the first and the last sixteen bodies.  Every
list but tree_generic_float's last sixteen (a walk of 23 steps, past the cap: the full kernel and a gather) takes the walk, asserted
through body_list_walk.

Then: the list result against the rows of Plan.body_poses / body_twists on the device at the same bounds (the worst difference is printed,
DESIGN section 7h'' records it); the full-and-gather route of parallel_chain_exp_d10_l16; graph capture and a caller's stream; B = 130 in
three chunks under GRBDA_WORK_MAX_MB with the output seeded with NaN; world-frame (and a rotor's body-frame) sparse wrenches, whose poses
now come from the list kernels, against the oracle."""
import ctypes
import functools

import numpy as np
import pytest

import entry_points as EP
import kinematics_ref as K
import oracle_py as O
import term_states as TS
import wrench_ref as W
from deriv_recursion_numpy import parse
from id_derivative_refs import blob_of

pytestmark = pytest.mark.gpu
MODELS = ("rev_rotor_chain_3", "urdf_mini_cheetah", "tello_with_arms", "tree_generic_float")
BATCHES = (1, 63, 64, 65, 130)
B_TOP = BATCHES[-1]
SEED = 67
GRAVITY = (1.5, -2.5, -7.0)
KINDS = ("leaf", "two_leaves", "with_ancestor", "repeated", "first_body", "rotor", "first_sixteen", "last_sixteen")
FALLS_BACK = {("tree_generic_float", "last_sixteen")}


def _path(parent, b):
    out = []
    while b >= 0:
        out.append(b)
        b = parent[b]
    return out


@functools.lru_cache(maxsize=None)
def lists(name):
    """the body lists of a model, by kind, from its parent table"""
    blob = EP._model(name)
    parent = [b["parent"] for b in parse(blob)["bodies"]]
    places = W.tree_places(blob)
    nb = len(parent)
    leaves = [b for b in range(nb) if b not in parent]
    depth = lambda b: (len(_path(parent, b)), b)
    leaf = max((b for b in leaves if b not in places["rotors"]), key=depth)  # the deepest leaf that is no rotor
    # the other leaf: one that shares an ancestor with `leaf` (the walk branches there), as few as can be
    shared = {b: len(set(_path(parent, b)) & set(_path(parent, leaf))) for b in leaves if b != leaf}
    other = min((b for b in shared if shared[b] >= 1), key=lambda b: (shared[b], b))
    rotor = places["rotors"][-1]
    return {
        "leaf": [leaf],
        "two_leaves": sorted([leaf, other], reverse=True),
        "with_ancestor": [leaf, parent[leaf], _path(parent, leaf)[-1]],
        "repeated": [other, leaf, other, leaf],
        "first_body": [0],
        "rotor": [rotor],
        "first_sixteen": list(range(min(nb, 16))),
        "last_sixteen": list(range(nb - 1, max(nb - 16, 0) - 1, -1)),
    }


@functools.lru_cache(maxsize=None)
def plan_at_gravity(name):
    """a plan of this file's own (entry_points.plan_for's are shared and keep their gravity)"""
    import generalized_rbda_amd as G

    plan = G.Plan(EP._model(name))
    plan.set_gravity(GRAVITY)
    return plan


@functools.lru_cache(maxsize=None)
def references(name, rounded):
    """(q, qd, ydd, poses [B_TOP, n_bodies, 12], twists [B_TOP, n_bodies, 12]) of B_TOP states, read-only, computed once per process"""
    blob = EP._model(name)
    q, qd, ydd = (TS.fp32_rounded(a) if rounded else a for a in EP._states(blob, B_TOP, SEED))
    at_g = plan_at_gravity(name).blob
    if EP._big(blob):
        EP._BIG.add(at_g)
    poses = K.body_poses(blob, q, big=EP._big(blob)) if EP._big(blob) else O.body_poses(blob, q, plan_at_gravity(name).n_bodies)
    twists = K.body_twists(at_g, q, qd, ydd, big=EP._big(blob))
    return tuple(TS._frozen(np.ascontiguousarray(a)) for a in (q, qd, ydd, poses, twists))


def _held(got, ref, tol, what):
    err = EP._rel(got.reshape(len(got), -1), ref.reshape(len(ref), -1))
    print(f"{what}: {err:.2e}")
    assert np.isfinite(got).all() and err < tol, (what, err, tol)
    return err


def _run(name, bodies, B, dt, gpu, stream=None):
    """(poses list, twists list, reference poses rows, reference twists rows) of the first B states"""
    import torch

    dtype = torch.float32 if dt == "f32" else torch.float64
    plan = plan_at_gravity(name)
    q, qd, ydd, poses, twists = references(name, dt == "f32")
    t = lambda a: torch.as_tensor(a[:B], dtype=dtype, device=gpu)
    X = plan.body_poses_list(t(q), bodies, stream=stream)
    V = plan.body_twists_list(t(q), t(qd), t(ydd), bodies, stream=stream)
    assert X.shape == V.shape == (B, len(bodies), 12) and X.dtype == V.dtype == dtype
    if stream is not None:
        stream.synchronize()
    return X.double().cpu().numpy(), V.double().cpu().numpy(), poses[:B][:, bodies], twists[:B][:, bodies]


CASES = [(m, k) for m in MODELS for k in KINDS]


@pytest.mark.parametrize("name,kind", CASES, ids=[f"{m}-{k}" for m, k in CASES])
def test_listed_poses_and_twists_match_the_oracle_rows(name, kind, gpu):
    bodies = lists(name)[kind]
    walk = plan_at_gravity(name).body_list_walk(bodies)
    print(f"{name} {kind} {bodies}: walk {walk}")
    assert walk[2] == int((name, kind) in FALLS_BACK)
    for dt, tol in (("f64", EP.TOL64), ("f32", EP.TOL32)):
        for B in BATCHES:
            X, V, X_ref, V_ref = _run(name, bodies, B, dt, gpu)
            _held(X, X_ref, tol, f"{name} {kind} {dt} B={B} poses")
            _held(V, V_ref, tol, f"{name} {kind} {dt} B={B} twists")


@pytest.mark.parametrize("name", MODELS)
def test_the_list_agrees_with_the_rows_of_the_full_kernels(name, gpu):
    """against Plan.body_poses / body_twists on the device, at the bounds of the oracle comparison: the same formulas on the same device
    functions, so rounding level is expected -- printed, not asserted to the bit"""
    import torch

    plan = plan_at_gravity(name)
    for dt, tol in (("f64", EP.TOL64), ("f32", EP.TOL32)):
        dtype = torch.float32 if dt == "f32" else torch.float64
        q, qd, ydd, _, _ = references(name, dt == "f32")
        t = lambda a: torch.as_tensor(a, dtype=dtype, device=gpu)
        X_full, V_full = plan.body_poses(t(q)).double().cpu().numpy(), plan.body_twists(t(q), t(qd), t(ydd)).double().cpu().numpy()
        worst = [0.0, 0.0]
        for kind in KINDS:
            bodies = lists(name)[kind]
            X, V, _, _ = _run(name, bodies, B_TOP, dt, gpu)
            worst[0] = max(worst[0], _held(X, X_full[:, bodies], tol, f"{name} {kind} {dt} poses against body_poses"))
            worst[1] = max(worst[1], _held(V, V_full[:, bodies], tol, f"{name} {kind} {dt} twists against body_twists"))
        print(f"WORST DIFFERENCE TO THE FULL KERNELS {name} {dt}: poses {worst[0]:.2e} twists {worst[1]:.2e}")


def test_the_full_and_gather_route_matches_the_oracle(gpu):
    name = "parallel_chain_exp_d10_l16"
    plan = plan_at_gravity(name)
    bodies = list(range(plan.n_bodies - 16, plan.n_bodies))
    assert plan.body_list_walk(bodies) == (20, 0, 1)
    for dt, tol in (("f64", EP.TOL64), ("f32", EP.TOL32)):
        for B in (1, 65, 130):
            X, V, X_ref, V_ref = _run(name, bodies, B, dt, gpu)
            _held(X, X_ref, tol, f"{name} gather {dt} B={B} poses")
            _held(V, V_ref, tol, f"{name} gather {dt} B={B} twists")


def test_capture_and_replay(gpu):
    """one eager call of the same B and n on the stream, then the calls captured; the replay reads new states from the same tensors"""
    import torch

    import graph_capture as GC

    name, B = "urdf_mini_cheetah", 65
    plan = plan_at_gravity(name)
    bodies = lists(name)["two_leaves"]
    q, qd, ydd, poses, twists = references(name, False)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=gpu)
    tq, tqd, ty = t(q[:B]), t(qd[:B]), t(ydd[:B])
    cap = GC.capture(lambda: (plan.body_poses_list(tq, bodies), plan.body_twists_list(tq, tqd, ty, bodies)))
    try:
        print(f"captured nodes: {cap.nodes}")
        assert cap.nodes["memcpy"] == 0 and cap.nodes["kernel"] >= 3  # poses; spanning rates and twists
        for a, src in ((tq, q), (tqd, qd), (ty, ydd)):
            a.copy_(t(src[B:2 * B]))
        X, V = (o.cpu().numpy() for o in cap.replay())
        _held(X, poses[B:2 * B][:, bodies], EP.TOL64, "replayed poses")
        _held(V, twists[B:2 * B][:, bodies], EP.TOL64, "replayed twists")
    finally:
        cap.drop()


def test_on_a_callers_stream(gpu):
    import torch

    name = "tello_with_arms"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    X, V, X_ref, V_ref = _run(name, lists(name)["last_sixteen"], B_TOP, "f64", gpu, stream=s)
    _held(X, X_ref, EP.TOL64, "side stream poses")
    _held(V, V_ref, EP.TOL64, "side stream twists")


def test_chunks_write_every_row(gpu, monkeypatch):
    """tree64_floating, its last sixteen bodies (past the cap: 90 x 12 scalars of full rows per state): under GRBDA_WORK_MAX_MB=1 the slab
    holds one tile of 64 states of the poses and of the twists, so B = 130 goes through in three passes, the last of two states.  The
    outputs are seeded with NaN."""
    import torch

    import generalized_rbda_amd as G

    blob = blob_of("tree64_floating")
    plan = G.Plan(blob)
    plan.set_gravity(GRAVITY)
    nb, B = plan.n_bodies, B_TOP
    bodies = list(range(nb - 16, nb))
    assert plan.body_list_walk(bodies)[2] == 1
    per_state = (nb * 12 + 2 * plan.n_span_vel) * 8
    assert (1 << 20) // (nb * 12 * 8) // 64 * 64 == 64 and (1 << 20) // per_state // 64 * 64 == 64  # states per pass: poses, twists
    q, qd, ydd = EP._states(blob, B, SEED)
    X_ref, V_ref = O.body_poses(blob, q, nb)[:, bodies], K.body_twists(plan.blob, q, qd, ydd)[:, bodies]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gpu)
    tq, tqd, ty = t(q), t(qd), t(ydd)
    X, V = (torch.full((B, 16, 12), float("nan"), dtype=torch.float64, device=gpu) for _ in range(2))
    arr = (ctypes.c_int * 16)(*bodies)
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", "1")
    plan.release_work()
    torch.cuda.synchronize()
    try:
        plan._dispatch("body_poses_list", torch.float64, tq.data_ptr(), 16, arr, X.data_ptr(), B, 0, None)
        plan._dispatch("body_twists_list", torch.float64, tq.data_ptr(), tqd.data_ptr(), ty.data_ptr(), 16, arr, V.data_ptr(), B, 0, None)
        torch.cuda.synchronize()
    finally:
        plan.release_work()
    _held(X.cpu().numpy(), X_ref, EP.TOL64, "chunked poses")
    _held(V.cpu().numpy(), V_ref, EP.TOL64, "chunked twists")


@pytest.mark.parametrize("algo", ["aba", "rnea"])
def test_world_frame_wrenches_on_the_listed_poses(algo, gpu):
    """grbda_aba_wrench_* / grbda_rnea_wrench_* with frame = world on the Mini Cheetah's feet (the chain route: the listed poses, the
    rotation, the wrench-carrying kernel) and with frame = body on a rotor (the dense route: the listed poses, the scatter) against the
    oracle's dynamics at the dense world-frame f_ext of wrench_ref"""
    import torch

    name, B = "urdf_mini_cheetah", 65
    blob, plan = EP._model(name), EP.plan_for(name, ())
    places = W.tree_places(blob)
    rng = np.random.default_rng(SEED)
    for bodies, frame in ((places["tips"][:2][::-1], "world"), (places["tips"] + [places["tips"][0]], "world"), ([places["rotors"][-1], places["tips"][0]], "body")):
        for dt, tol in (("f64", EP.TOL64), ("f32", EP.TOL32)):
            dtype = torch.float32 if dt == "f32" else torch.float64
            q, qd, x = (TS.fp32_rounded(a) if dt == "f32" else a for a in EP._states(blob, B, SEED))
            w = rng.uniform(-5, 5, size=(B, len(bodies), 6))
            w = TS.fp32_rounded(w) if dt == "f32" else w
            fext = W.dense_f_ext(blob, q, bodies, w, frame)
            ref = (O.forward_dynamics if algo == "aba" else O.inverse_dynamics)(blob, q, qd, x, fext)
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)
            call = plan.forward_dynamics_wrench if algo == "aba" else plan.inverse_dynamics_wrench
            got = call(t(q), t(qd), t(x), bodies, t(w), frame=frame).double().cpu().numpy()
            print(f"{algo} {frame} {bodies} {dt}: kernel {plan.wrench_kernel_name(algo, dt, bodies, frame, B)}")
            _held(got, ref, tol, f"{algo} {frame} {bodies} {dt}")
