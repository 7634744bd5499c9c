"""Frame Jacobians and their drift at a listed few body frames on the GPU (include/grbda_hip_jacobians.h; run with -m gpu on an MI355X).

J[B, n, 6, nv] and drift[B, n, 6] of Plan.frame_jacobians are held to frame_jacobian_ref (test_frame_jacobian_ref_cpu.py pins it to the
oracle's unit-wrench Jacobians and to contact_ref) in both frames at the project's bounds, fp64 1e-9 and fp32 1e-3, as
max |got - ref| / (1 + max |ref|) over the batch; fp32 runs on float32-rounded states, which the reference is then fed.  The plans sit at an
oblique gravity, which the drift must not see, and the states have nonzero qd.

Batches 1, 63, 64, 65, 130.  Lists per model (lists()): one leaf; two leaves either side of a branch; a body with its ancestor and the root;
a body twice with two offsets; the first body alone (offsets=None); a rotor (a model without one: its last body); the longest list the walk
accepts (grown from the last body down while the route stays 0; a model that never walks: its last sixteen); sixteen frames, past the
caps.  The route of every list is asserted against expected_route(), which derives it from the parent table and the cluster kinds.

Then, at B = 130: the structural zeros with the output seeded with NaN; the J of Plan.inv_osim and the velocities of Plan.body_twists_list
on the device; graph capture; a caller's stream; route 1 in three chunks under GRBDA_WORK_MAX_MB; J alone, the drift alone and both; the
host variant."""
import ctypes
import functools

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import frame_jacobian_ref as FJ
import term_states as TS
from deriv_recursion_numpy import parse

pytestmark = pytest.mark.gpu
MODELS = ("rev_rotor_chain_3", "urdf_mini_cheetah", "urdf_mini_cheetah_rpy", "tello_with_arms", "tree_generic_float", "parallel_chain_exp_d10_l16")
BATCHES = (1, 63, 64, 65, 130)
B_TOP = BATCHES[-1]
SEED = 73
GRAVITY = TS.OBLIQUE
KINDS = ("leaf", "two_leaves", "with_ancestor", "repeated", "first_body", "rotor", "longest", "past_caps")
FRAMES = ("body", "world")
MAX_WALK, MAX_SLOTS = 19, 10  # the caps of include/grbda_hip_jacobians.h
_OFF = [(0.03, -0.07, 0.11), (-0.05, 0.02, -0.2), (0.013, 0.09, 0.04), (0.08, 0.06, -0.03)]


def _offsets(n):
    return [tuple(x * (1 + 0.1 * (i // 4)) for x in _OFF[i % 4]) for i in range(n)]


def _path(parent, b):
    out = []
    while b >= 0:
        out.append(b)
        b = parent[b]
    return out


@functools.lru_cache(maxsize=None)
def plan_at_gravity(name):
    """a plan of this file's own (entry_points.plan_for's are shared and keep their gravity)"""
    import generalized_rbda_amd as G

    plan = G.Plan(EP._model(name))
    plan.set_gravity(GRAVITY)
    if EP._big(EP._model(name)):
        EP._BIG.add(plan.blob)
    return plan


@functools.lru_cache(maxsize=None)
def tree(name):
    """(parent table, per body whether an implicit cluster sits on its root path, rotors: leaves of clusters of several bodies and one
    coordinate whose parent is outside the cluster)"""
    m = parse(EP._model(name))
    bodies, clusters = m["bodies"], m["clusters"]
    parent = [b["parent"] for b in bodies]
    implicit = [clusters[b["cluster"]][9] in (2, 3) for b in bodies]
    through = [any(implicit[a] for a in _path(parent, b)) for b in range(len(bodies))]
    members = {}
    for i, b in enumerate(bodies):
        members.setdefault(b["cluster"], []).append(i)
    rotors = [mem[-1] for c, mem in members.items() if len(mem) >= 2 and not implicit[mem[0]] and mem[-1] not in parent]
    return parent, through, rotors


def expected_route(name, bodies):
    """0 the walk, 1 the expanded batch, from the model alone: the spanning-tree route, an implicit cluster on a root path, a walk past
    MAX_WALK bodies, frames and saved branch points past MAX_SLOTS"""
    plan = plan_at_gravity(name)
    parent, through, _ = tree(name)
    walk_len, saved, _ = plan.body_list_walk(bodies)
    return int(bool(plan.info().spanning_tree_route) or any(through[b] for b in bodies) or walk_len > MAX_WALK or len(bodies) + saved > MAX_SLOTS)


@functools.lru_cache(maxsize=None)
def lists(name):
    """kind -> (bodies, offsets)"""
    plan = plan_at_gravity(name)
    parent, through, rotors = tree(name)
    nb = len(parent)
    leaves = [b for b in range(nb) if b not in parent]
    depth = lambda b: (len(_path(parent, b)), b)
    leaf = max((b for b in leaves if b not in rotors), key=depth)
    shared = {b: len(set(_path(parent, b)) & set(_path(parent, leaf))) for b in leaves if b != leaf}
    other = min((b for b in shared if shared[b] >= 1), key=lambda b: (shared[b], b)) if any(shared.values()) else leaf
    longest = []
    for b in range(nb - 1, -1, -1):
        if len(longest) < 16 and plan.frame_jacobians_route(longest + [b])[0] == 0:
            longest.append(b)
    longest = longest or list(range(nb - 1, max(nb - 16, 0) - 1, -1))
    past = (list(range(nb - 1, max(nb - 16, 0) - 1, -1)) * 16)[:16]
    out = {
        "leaf": [leaf],
        "two_leaves": sorted({leaf, other}, reverse=True),
        "with_ancestor": [leaf, parent[leaf] if parent[leaf] >= 0 else leaf, _path(parent, leaf)[-1]],
        "repeated": [other, leaf, other, leaf],
        "first_body": [0],
        "rotor": [rotors[-1] if rotors else nb - 1],
        "longest": longest,
        "past_caps": past,
    }
    return {k: (v, None if k == "first_body" else _offsets(len(v))) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def every_body(name, rounded):
    """(q, qd, all_bodies(...)) of B_TOP states, read-only, computed once per process"""
    blob = EP._model(name)
    q, qd, _ = (TS.fp32_rounded(a) if rounded else a for a in EP._states(blob, B_TOP, SEED))
    at_g = plan_at_gravity(name).blob
    ref = FJ.all_bodies(at_g, q, qd, big=EP._big(blob))
    return tuple(TS._frozen(np.ascontiguousarray(a)) for a in (q, qd) + ref)


def reference(name, kind, frame, rounded):
    bodies, offsets = lists(name)[kind]
    return FJ.assemble(*every_body(name, rounded)[2:], bodies, offsets, frame)


def _held(got, ref, tol, what):
    err = EP._rel(got.reshape(len(got), -1), ref.reshape(len(ref), -1))
    print(f"{what}: {err:.2e}")
    assert np.isfinite(got).all() and err < tol, (what, err, tol)
    return err


def _tensors(name, B, dt, gpu, lo=0):
    import torch

    dtype = torch.float32 if dt == "f32" else torch.float64
    q, qd = every_body(name, dt == "f32")[:2]
    return tuple(torch.as_tensor(a[lo:lo + B], dtype=dtype, device=gpu) for a in (q, qd))


def _run(name, kind, frame, B, dt, gpu, stream=None):
    """(J, drift) of the first B states as float64 numpy"""
    bodies, offsets = lists(name)[kind]
    tq, tqd = _tensors(name, B, dt, gpu)
    J, d = plan_at_gravity(name).frame_jacobians(tq, bodies, offsets, frame, qd=tqd, drift=True, stream=stream)
    assert J.shape == (B, len(bodies), 6, plan_at_gravity(name).nv) and d.shape == (B, len(bodies), 6) and J.dtype == d.dtype == tq.dtype
    if stream is not None:
        stream.synchronize()
    return J.double().cpu().numpy(), d.double().cpu().numpy()


CASES = [(m, k) for m in MODELS for k in KINDS]


@pytest.mark.parametrize("name,kind", CASES, ids=[f"{m}-{k}" for m, k in CASES])
def test_jacobians_and_drift_match_the_reference(name, kind, gpu):
    bodies, offsets = lists(name)[kind]
    route = plan_at_gravity(name).frame_jacobians_route(bodies)
    print(f"{name} {kind} {bodies}: route {route}")
    assert route[0] == expected_route(name, bodies)
    if kind == "past_caps":
        assert route[0] == 1 and len(bodies) == 16
    for frame in FRAMES:
        for dt, tol in (("f64", EP.TOL64), ("f32", EP.TOL32)):
            J_ref, d_ref = reference(name, kind, frame, dt == "f32")
            assert np.abs(J_ref).max() > 0.1
            for B in BATCHES:
                J, d = _run(name, kind, frame, B, dt, gpu)
                _held(J, J_ref[:B], tol, f"{name} {kind} {frame} {dt} B={B} J")
                _held(d, d_ref[:B], tol, f"{name} {kind} {frame} {dt} B={B} drift")


def test_both_routes_occur():
    routes = {(m, k): plan_at_gravity(m).frame_jacobians_route(lists(m)[k][0])[0] for m, k in CASES}
    for m in ("urdf_mini_cheetah", "tello_with_arms", "tree_generic_float"):
        assert {routes[m, k] for k in KINDS} == {0, 1}, (m, routes)
    assert {routes["parallel_chain_exp_d10_l16", k] for k in KINDS} == {1}
    assert all(routes[m, "longest"] == 0 for m in MODELS if m != "parallel_chain_exp_d10_l16")
    # the walk's longest lists fill a cap: one more frame, or one more body, does not walk
    for m in ("urdf_mini_cheetah", "tree_generic_float"):
        bodies = lists(m)["longest"][0]
        r, walk_len, saved = plan_at_gravity(m).frame_jacobians_route(bodies)
        assert len(bodies) + saved == MAX_SLOTS or walk_len == MAX_WALK or len(bodies) == plan_at_gravity(m).n_bodies, (m, bodies, walk_len, saved)


def _columns_on_the_path(name, b):
    m = parse(EP._model(name))
    parent = [x["parent"] for x in m["bodies"]]
    cols = set()
    for a in _path(parent, b):
        cl = m["clusters"][m["bodies"][a]["cluster"]]
        cols |= set(range(cl[5], cl[5] + cl[6]))
    return cols


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "two_leaves"), ("tree_generic_float", "longest"), ("tello_with_arms", "two_leaves"),
                                       ("tello_with_arms", "longest"), ("parallel_chain_exp_d10_l16", "leaf")])
def test_structural_zeros_are_written(name, kind, gpu):
    """the outputs seeded with NaN at the C level: every entry finite, the columns off a frame's root path exactly 0.0"""
    import torch

    plan = plan_at_gravity(name)
    bodies, offsets = lists(name)[kind]
    n, nv = len(bodies), plan.nv
    arr = (ctypes.c_int * n)(*bodies)
    off = (ctypes.c_double * (3 * n))(*[x for o in offsets for x in o])
    for dt in ("f64", "f32"):
        tq, tqd = _tensors(name, B_TOP, dt, gpu)
        for fr, frame in enumerate(FRAMES):
            J = torch.full((B_TOP, n, 6, nv), float("nan"), dtype=tq.dtype, device=gpu)
            d = torch.full((B_TOP, n, 6), float("nan"), dtype=tq.dtype, device=gpu)
            torch.cuda.synchronize()
            plan._dispatch("frame_jacobians", tq.dtype, tq.data_ptr(), tqd.data_ptr(), n, arr, off, fr, J.data_ptr(), d.data_ptr(), B_TOP, 0, None)
            torch.cuda.synchronize()
            J, d = J.cpu().numpy(), d.cpu().numpy()
            assert np.isfinite(J).all() and np.isfinite(d).all()
            for i, b in enumerate(bodies):
                on = sorted(_columns_on_the_path(name, b))
                offp = [c for c in range(nv) if c not in on]
                assert (J[:, i][:, :, offp] == 0.0).all(), (name, kind, frame, dt, i)
                assert np.abs(J[:, i][:, :, on]).max() > 0.1
            J_ref, d_ref = reference(name, kind, frame, dt == "f32")
            _held(J.astype(np.float64), J_ref, EP.TOL64 if dt == "f64" else EP.TOL32, f"{name} {kind} {frame} {dt} seeded J")
            _held(d.astype(np.float64), d_ref, EP.TOL64 if dt == "f64" else EP.TOL32, f"{name} {kind} {frame} {dt} seeded drift")


@pytest.mark.parametrize("key", ["cheetah_feet", "tello_feet"])
def test_the_body_frame_jacobian_is_the_one_of_inv_osim(key, gpu):
    """urdf_mini_cheetah: inv_osim by force propagation; tello_with_arms: by unit wrenches"""
    name, bodies, offsets = C.contact_set(key)
    plan = plan_at_gravity(name)
    assert plan.frame_jacobians_route(bodies)[0] == (0 if key == "cheetah_feet" else 1)
    for dt, tol in (("f64", EP.TOL64), ("f32", EP.TOL32)):
        tq, _ = _tensors(name, B_TOP, dt, gpu)
        J = plan.frame_jacobians(tq, bodies, offsets).double().cpu().numpy()
        J_osim = plan.inv_osim(tq, bodies, offsets, with_jacobian=True)[1].double().cpu().numpy()
        _held(J.reshape(B_TOP, 6 * len(bodies), -1), J_osim, tol, f"{key} {dt} J against inv_osim")


@pytest.mark.parametrize("name", ["urdf_mini_cheetah", "tello_with_arms", "tree_generic_float"])
def test_the_jacobian_times_the_velocity_is_the_listed_twist_at_the_point(name, gpu):
    import torch

    plan = plan_at_gravity(name)
    for kind in ("two_leaves", "longest", "repeated"):
        bodies, offsets = lists(name)[kind]
        for dt, tol in (("f64", EP.TOL64), ("f32", EP.TOL32)):
            tq, tqd = _tensors(name, B_TOP, dt, gpu)
            J = plan.frame_jacobians(tq, bodies, offsets)
            v = torch.einsum("bcik,bk->bci", J, tqd)
            V = plan.body_twists_list(tq, tqd, torch.zeros_like(tqd), bodies)
            o = torch.as_tensor(offsets, dtype=tq.dtype, device=gpu)[None].expand(B_TOP, -1, -1)
            ref = torch.cat([V[:, :, 0:3], V[:, :, 3:6] + torch.linalg.cross(V[:, :, 0:3], o)], dim=2)
            _held(v.double().cpu().numpy(), ref.double().cpu().numpy(), tol, f"{name} {kind} {dt} J qd against body_twists_list")


def _both(plan, tq, tqd, bodies, offsets, frame, stream=None):
    return plan.frame_jacobians(tq, bodies, offsets, frame, qd=tqd, drift=True, stream=stream)


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "two_leaves"), ("tello_with_arms", "two_leaves")])
def test_capture_and_replay(name, kind, gpu):
    """one eager call of the same B and n on the stream, then the call captured; the replay reads new states from the same tensors and
    gives the bits of an eager call on them"""
    import graph_capture as GC

    B = 65
    plan = plan_at_gravity(name)
    bodies, offsets = lists(name)[kind]
    for frame in FRAMES:
        tq, tqd = _tensors(name, B, "f64", gpu)
        cap = GC.capture(lambda: _both(plan, tq, tqd, bodies, offsets, frame))
        try:
            print(f"captured nodes: {cap.nodes}")
            assert cap.nodes["memcpy"] == 0 and cap.nodes["kernel"] >= 3
            nq, nqd = _tensors(name, B, "f64", gpu, lo=B)
            tq.copy_(nq)
            tqd.copy_(nqd)
            J, d = (o.cpu().numpy() for o in cap.replay())
            J_e, d_e = (o.cpu().numpy() for o in _both(plan, nq, nqd, bodies, offsets, frame))
            assert EP.same_bits_np(J, J_e) and EP.same_bits_np(d, d_e)
            J_ref, d_ref = reference(name, kind, frame, False)
            _held(J, J_ref[B:2 * B], EP.TOL64, f"{name} {frame} replayed J")
            _held(d, d_ref[B:2 * B], EP.TOL64, f"{name} {frame} replayed drift")
        finally:
            cap.drop()


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "longest"), ("tello_with_arms", "two_leaves")])
def test_on_a_callers_stream(name, kind, gpu):
    import torch

    plan = plan_at_gravity(name)
    bodies, offsets = lists(name)[kind]
    tq, tqd = _tensors(name, B_TOP, "f64", gpu)
    J0, d0 = (o.cpu().numpy() for o in _both(plan, tq, tqd, bodies, offsets, "world"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    J, d = _both(plan, tq, tqd, bodies, offsets, "world", stream=s)
    s.synchronize()
    assert EP.same_bits_np(J.cpu().numpy(), J0) and EP.same_bits_np(d.cpu().numpy(), d0)


def test_route_one_in_three_chunks(gpu, monkeypatch):
    """tello_with_arms, two feet in the world frame, J and drift: per state nv rows of the expanded batch, so that the smallest budget,
    GRBDA_WORK_MAX_MB=1, holds less than two tiles and B = 130 goes through in three passes of 64, 64 and 2 states"""
    import torch

    import generalized_rbda_amd as G

    name, kind = "tello_with_arms", "two_leaves"
    plan = G.Plan(EP._model(name))
    plan.set_gravity(GRAVITY)
    bodies, offsets = lists(name)[kind]
    assert plan.frame_jacobians_route(bodies)[0] == 1 and plan.body_list_walk(bodies)[2] == 0
    n12, nq, nv, ns = 12 * len(bodies), plan.nq, plan.nv, plan.n_span_vel
    per_state = (n12 + nv * (nq + 2 * nv + n12 + 2 * ns) + (nv + n12 + 2 * ns)) * 8
    assert (1 << 20) // per_state < 128  # states per pass: one tile
    tq, tqd = _tensors(name, B_TOP, "f64", gpu)
    J0, d0 = (o.cpu().numpy() for o in _both(plan, tq, tqd, bodies, offsets, "world"))
    n = len(bodies)
    J = torch.full((B_TOP, n, 6, nv), float("nan"), dtype=torch.float64, device=gpu)
    d = torch.full((B_TOP, n, 6), float("nan"), dtype=torch.float64, device=gpu)
    arr = (ctypes.c_int * n)(*bodies)
    off = (ctypes.c_double * (3 * n))(*[x for o in offsets for x in o])
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", "1")
    plan.release_work()
    torch.cuda.synchronize()
    try:
        plan._dispatch("frame_jacobians", torch.float64, tq.data_ptr(), tqd.data_ptr(), n, arr, off, 1, J.data_ptr(), d.data_ptr(), B_TOP, 0, None)
        torch.cuda.synchronize()
    finally:
        plan.release_work()
    assert EP.same_bits_np(J.cpu().numpy(), J0) and EP.same_bits_np(d.cpu().numpy(), d0)


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "two_leaves"), ("tello_with_arms", "two_leaves"), ("parallel_chain_exp_d10_l16", "leaf")])
def test_either_output_alone_is_the_same(name, kind, gpu):
    plan = plan_at_gravity(name)
    bodies, offsets = lists(name)[kind]
    for frame in FRAMES:
        for dt in ("f64", "f32"):
            tq, tqd = _tensors(name, B_TOP, dt, gpu)
            J, d = (o.cpu().numpy() for o in _both(plan, tq, tqd, bodies, offsets, frame))
            assert EP.same_bits_np(plan.frame_jacobians(tq, bodies, offsets, frame).cpu().numpy(), J)
            assert EP.same_bits_np(plan.frame_drift(tq, tqd, bodies, offsets, frame).cpu().numpy(), d)


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "two_leaves"), ("tello_with_arms", "two_leaves")])
def test_the_host_variant_agrees(name, kind, gpu):
    plan = plan_at_gravity(name)
    bodies, offsets = lists(name)[kind]
    q, qd = every_body(name, False)[:2]
    tq, tqd = _tensors(name, B_TOP, "f64", gpu)
    for frame in FRAMES:
        J, d = (o.cpu().numpy() for o in _both(plan, tq, tqd, bodies, offsets, frame))
        J_h, d_h = plan.frame_jacobians_host(q, bodies, offsets, frame, qd=qd, drift=True)
        _held(J_h, J, 1e-12, f"{name} {frame} host J")
        _held(d_h, d, 1e-12, f"{name} {frame} host drift")
        _held(plan.frame_jacobians_host(q, bodies, offsets, frame), J, 1e-12, f"{name} {frame} host J alone")


def test_the_facade_agrees(gpu, tmp_path):
    """tests/cpp/frame_jacobians_facade_test.cpp with a device: frameJacobiansBatch against grbda_frame_jacobians_f64, 1e-12"""
    from test_frame_jacobians_args_cpu import run_facade_test

    run_facade_test(tmp_path)
