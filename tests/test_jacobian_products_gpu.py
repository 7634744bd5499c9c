"""J v and J^T f at a listed few body frames on the GPU (include/grbda_hip_jacobian_products.h; run with -m gpu on an MI355X).

Jv[B, n, 6] and JTf[B, nv] of Plan.frame_jacobian_products are held to jacobian_product_ref (test_jacobian_product_ref_cpu.py pins it to the
listed twists and to the oracle's inverse dynamics) over the models, the eight list kinds and the batches 1, 63, 64, 65, 130 of
test_frame_jacobians_gpu.py, in both frames, at the project's bounds, fp64 1e-9 and fp32 1e-3, as max |got - ref| / (1 + max |ref|) over the
batch.  v and f are dense and random (a fixed seed); fp32 runs on float32-rounded q, v and f, which the reference is then fed.  The plans
sit at an oblique gravity, which the products must not see.  The route of every list is asserted against expected_route().

Then, at B = 130: JTf seeded with NaN at the C level comes back finite with exact 0.0 in the columns off every listed root path, on both
routes; a body listed twice gives the sum; both products against Plan.frame_jacobians contracted by torch.einsum on the device (the worst
difference is printed, and held to the project's bound, not to the bit); J v at v = qd against the velocities of Plan.body_twists_list;
either product alone, the other's buffer untouched; graph capture and replay; a caller's stream; route 1 in three chunks under
GRBDA_WORK_MAX_MB; the host variant."""
import ctypes
import functools

import numpy as np
import pytest

import entry_points as EP
import jacobian_product_ref as JP
import term_states as TS
from deriv_recursion_numpy import parse
from test_frame_jacobians_gpu import B_TOP, BATCHES, FRAMES, GRAVITY, KINDS, MODELS, every_body, expected_route, lists, plan_at_gravity, reference

pytestmark = pytest.mark.gpu
SEED = 97
SENTINEL = 7.25


@functools.lru_cache(maxsize=None)
def directions(name, kind, rounded):
    """(v[B_TOP, nv], f[B_TOP, n, 6]) of a list, read-only"""
    n, nv = len(lists(name)[kind][0]), plan_at_gravity(name).nv
    rng = np.random.default_rng([SEED, MODELS.index(name), KINDS.index(kind)])
    v, f = rng.uniform(-2, 2, size=(B_TOP, nv)), rng.uniform(-3, 3, size=(B_TOP, n, 6))
    return tuple(TS._frozen(TS.fp32_rounded(a) if rounded else a) for a in (v, f))


@functools.lru_cache(maxsize=None)
def products_ref(name, kind, frame, rounded):
    """(Jv, JTf) of the B_TOP states from the J of frame_jacobian_ref"""
    J = reference(name, kind, frame, rounded)[0]
    v, f = directions(name, kind, rounded)
    return JP.jv_of(J, v), JP.jtf_of(J, f)


def _held(got, ref, tol, what):
    err = EP._rel(got.reshape(len(got), -1), ref.reshape(len(ref), -1))
    print(f"{what}: {err:.2e}")
    assert np.isfinite(got).all() and err < tol, (what, err, tol)
    return err


def _tensors(name, kind, B, dt, gpu, lo=0):
    """(q, v, f) of the states lo .. lo + B"""
    import torch

    dtype = torch.float32 if dt == "f32" else torch.float64
    q = every_body(name, dt == "f32")[0]
    v, f = directions(name, kind, dt == "f32")
    return tuple(torch.as_tensor(a[lo:lo + B], dtype=dtype, device=gpu) for a in (q, v, f))


def _both(name, kind, frame, tq, tv, tf, stream=None):
    bodies, offsets = lists(name)[kind]
    return plan_at_gravity(name).frame_jacobian_products(tq, bodies, v=tv, f=tf, offsets=offsets, frame=frame, stream=stream)


def _tol(dt):
    return EP.TOL64 if dt == "f64" else EP.TOL32


CASES = [(m, k) for m in MODELS for k in KINDS]


@pytest.mark.parametrize("name,kind", CASES, ids=[f"{m}-{k}" for m, k in CASES])
def test_the_products_match_the_reference(name, kind, gpu):
    bodies, offsets = lists(name)[kind]
    plan = plan_at_gravity(name)
    assert plan.get_gravity() == list(GRAVITY)
    route = plan.frame_jacobians_route(bodies)
    print(f"{name} {kind} {bodies}: route {route}")
    assert route[0] == expected_route(name, bodies)
    for frame in FRAMES:
        for dt in ("f64", "f32"):
            Jv_ref, JTf_ref = products_ref(name, kind, frame, dt == "f32")
            assert np.abs(Jv_ref).max() > 0.1 and np.abs(JTf_ref).max() > 0.1
            for B in BATCHES:
                tq, tv, tf = _tensors(name, kind, B, dt, gpu)
                Jv, JTf = _both(name, kind, frame, tq, tv, tf)
                assert Jv.shape == (B, len(bodies), 6) and JTf.shape == (B, plan.nv) and Jv.dtype == JTf.dtype == tq.dtype
                _held(Jv.double().cpu().numpy(), Jv_ref[:B], _tol(dt), f"{name} {kind} {frame} {dt} B={B} Jv")
                _held(JTf.double().cpu().numpy(), JTf_ref[:B], _tol(dt), f"{name} {kind} {frame} {dt} B={B} JTf")


def _columns_on_the_paths(name, bodies):
    m = parse(EP._model(name))
    cols = set()
    for b in bodies:
        while b >= 0:
            cl = m["clusters"][m["bodies"][b]["cluster"]]
            cols |= set(range(cl[5], cl[5] + cl[6]))
            b = m["bodies"][b]["parent"]
    return cols


def _c_list(name, kind):
    bodies, offsets = lists(name)[kind]
    n = len(bodies)
    return n, (ctypes.c_int * n)(*bodies), (ctypes.c_double * (3 * n))(*[x for o in offsets for x in o])


# route 0: the mini cheetah, tree_generic_float, tello's arms; route 1: tello's legs (implicit clusters), the spanning-tree route
@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "two_leaves"), ("rev_rotor_chain_3", "rotor"), ("tree_generic_float", "longest"),
                                       ("tello_with_arms", "longest"), ("tello_with_arms", "two_leaves"), ("parallel_chain_exp_d10_l16", "leaf")])
def test_every_column_is_written_and_the_columns_off_the_paths_are_zero(name, kind, gpu):
    """both outputs seeded with NaN at the C level: every entry finite, the columns of JTf on no listed frame's root path exactly 0.0"""
    import torch

    plan = plan_at_gravity(name)
    bodies, _ = lists(name)[kind]
    n, arr, off = _c_list(name, kind)
    on = sorted(_columns_on_the_paths(name, bodies))
    offp = [c for c in range(plan.nv) if c not in on]
    print(f"{name} {kind}: route {plan.frame_jacobians_route(bodies)[0]}, {len(on)} columns on the paths, {len(offp)} off")
    for dt in ("f64", "f32"):
        tq, tv, tf = _tensors(name, kind, B_TOP, dt, gpu)
        for fr, frame in enumerate(FRAMES):
            Jv = torch.full((B_TOP, n, 6), float("nan"), dtype=tq.dtype, device=gpu)
            JTf = torch.full((B_TOP, plan.nv), float("nan"), dtype=tq.dtype, device=gpu)
            torch.cuda.synchronize()
            plan._dispatch("frame_jacobian_products", tq.dtype, tq.data_ptr(), tv.data_ptr(), tf.data_ptr(), n, arr, off, fr, Jv.data_ptr(),
                           JTf.data_ptr(), B_TOP, 0, None)
            torch.cuda.synchronize()
            Jv, JTf = Jv.double().cpu().numpy(), JTf.double().cpu().numpy()
            assert np.isfinite(Jv).all() and np.isfinite(JTf).all()
            assert (JTf[:, offp] == 0.0).all(), (name, kind, frame, dt)
            assert np.abs(JTf[:, on]).max() > 0.1
            Jv_ref, JTf_ref = products_ref(name, kind, frame, dt == "f32")
            _held(Jv, Jv_ref, _tol(dt), f"{name} {kind} {frame} {dt} seeded Jv")
            _held(JTf, JTf_ref, _tol(dt), f"{name} {kind} {frame} {dt} seeded JTf")


def test_both_routes_are_seeded():
    routes = {(m, k): plan_at_gravity(m).frame_jacobians_route(lists(m)[k][0])[0] for m, k in CASES}
    assert routes["urdf_mini_cheetah", "two_leaves"] == routes["tree_generic_float", "longest"] == routes["tello_with_arms", "longest"] == 0
    assert routes["rev_rotor_chain_3", "rotor"] == 0
    assert routes["tello_with_arms", "two_leaves"] == routes["parallel_chain_exp_d10_l16", "leaf"] == 1
    assert off_path_columns_exist("urdf_mini_cheetah", "two_leaves") and off_path_columns_exist("tello_with_arms", "two_leaves")


def off_path_columns_exist(name, kind):
    return len(_columns_on_the_paths(name, lists(name)[kind][0])) < plan_at_gravity(name).nv


@pytest.mark.parametrize("name", ["urdf_mini_cheetah", "tello_with_arms", "rev_rotor_chain_3"])
def test_a_body_listed_twice_gives_the_sum(name, gpu):
    """the `repeated` list [a, b, a, b] with four offsets: JTf is the sum of the list's two halves, Jv holds the halves' rows"""
    plan = plan_at_gravity(name)
    bodies, offsets = lists(name)["repeated"]
    assert bodies[:2] == bodies[2:]
    for frame in FRAMES:
        for dt in ("f64", "f32"):
            tq, tv, tf = _tensors(name, "repeated", B_TOP, dt, gpu)
            Jv, JTf = _both(name, "repeated", frame, tq, tv, tf)
            halves = [plan.frame_jacobian_products(tq, bodies[s], v=tv, f=tf[:, s], offsets=offsets[s], frame=frame) for s in (slice(0, 2), slice(2, 4))]
            _held(JTf.double().cpu().numpy(), (halves[0][1] + halves[1][1]).double().cpu().numpy(), _tol(dt), f"{name} {frame} {dt} JTf, sum of the halves")
            _held(Jv.double().cpu().numpy(), np.concatenate([h[0].double().cpu().numpy() for h in halves], axis=1), _tol(dt),
                  f"{name} {frame} {dt} Jv, the halves' rows")


@pytest.mark.parametrize("name", ["urdf_mini_cheetah", "tello_with_arms", "tree_generic_float"])
def test_the_products_are_the_jacobian_contracted_on_the_device(name, gpu):
    """against Plan.frame_jacobians and torch.einsum: the same J by definition.  Not to the bit: the walk sums a root path's axes before it
    moves them to the frame, the einsum sums the moved columns"""
    import torch

    plan = plan_at_gravity(name)
    worst = {}
    for kind in ("two_leaves", "longest", "repeated", "past_caps"):
        bodies, offsets = lists(name)[kind]
        for frame in FRAMES:
            for dt in ("f64", "f32"):
                tq, tv, tf = _tensors(name, kind, B_TOP, dt, gpu)
                Jv, JTf = _both(name, kind, frame, tq, tv, tf)
                J = plan.frame_jacobians(tq, bodies, offsets, frame)
                e1 = _held(Jv.double().cpu().numpy(), torch.einsum("bcik,bk->bci", J, tv).double().cpu().numpy(), _tol(dt), f"{name} {kind} {frame} {dt} Jv against J")
                e2 = _held(JTf.double().cpu().numpy(), torch.einsum("bcik,bci->bk", J, tf).double().cpu().numpy(), _tol(dt), f"{name} {kind} {frame} {dt} JTf against J")
                worst[dt] = max(worst.get(dt, 0.0), e1, e2)
    print(f"{name}: worst difference device against device, fp64 {worst['f64']:.2e}, fp32 {worst['f32']:.2e}")


@pytest.mark.parametrize("name", ["urdf_mini_cheetah", "tello_with_arms", "tree_generic_float"])
def test_jv_at_the_velocity_is_the_listed_twist_at_the_point(name, gpu):
    import torch

    plan = plan_at_gravity(name)
    for kind in ("two_leaves", "longest", "repeated"):
        bodies, offsets = lists(name)[kind]
        for dt in ("f64", "f32"):
            tq = _tensors(name, kind, B_TOP, dt, gpu)[0]
            tqd = torch.as_tensor(every_body(name, dt == "f32")[1], dtype=tq.dtype, device=gpu)
            got = plan.frame_jv(tq, tqd, bodies, offsets)
            V = plan.body_twists_list(tq, tqd, torch.zeros_like(tqd), bodies)
            o = torch.as_tensor(offsets, dtype=tq.dtype, device=gpu)[None].expand(B_TOP, -1, -1)
            ref = torch.cat([V[:, :, 0:3], V[:, :, 3:6] + torch.linalg.cross(V[:, :, 0:3], o)], dim=2)
            _held(got.double().cpu().numpy(), ref.double().cpu().numpy(), _tol(dt), f"{name} {kind} {dt} J qd against body_twists_list")


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "two_leaves"), ("tello_with_arms", "two_leaves"), ("parallel_chain_exp_d10_l16", "leaf")])
def test_either_product_alone_leaves_the_other_buffer_untouched(name, kind, gpu):
    """one arena [Jv | JTf] filled with a sentinel, the call given one of the two: that one is the product, the other half keeps the
    sentinel; and the shorthands agree with it"""
    import torch

    plan = plan_at_gravity(name)
    bodies, offsets = lists(name)[kind]
    n, arr, off = _c_list(name, kind)
    n_jv, n_jtf = B_TOP * n * 6, B_TOP * plan.nv
    for fr, frame in enumerate(FRAMES):
        for dt in ("f64", "f32"):
            tq, tv, tf = _tensors(name, kind, B_TOP, dt, gpu)
            Jv_ref, JTf_ref = products_ref(name, kind, frame, dt == "f32")
            item = tq.element_size()
            for which in ("Jv", "JTf"):
                arena = torch.full((n_jv + n_jtf,), SENTINEL, dtype=tq.dtype, device=gpu)
                torch.cuda.synchronize()
                jv = which == "Jv"
                plan._dispatch("frame_jacobian_products", tq.dtype, tq.data_ptr(), tv.data_ptr() if jv else None, None if jv else tf.data_ptr(), n, arr,
                               off, fr, arena.data_ptr() if jv else None, None if jv else arena.data_ptr() + n_jv * item, B_TOP, 0, None)
                torch.cuda.synchronize()
                a = arena.double().cpu().numpy()
                if jv:
                    assert (a[n_jv:] == SENTINEL).all()
                    _held(a[:n_jv].reshape(B_TOP, n, 6), Jv_ref, _tol(dt), f"{name} {frame} {dt} Jv alone")
                    assert EP.same_bits_np(plan.frame_jv(tq, tv, bodies, offsets, frame).double().cpu().numpy(), a[:n_jv].reshape(B_TOP, n, 6))
                else:
                    assert (a[:n_jv] == SENTINEL).all()
                    _held(a[n_jv:].reshape(B_TOP, -1), JTf_ref, _tol(dt), f"{name} {frame} {dt} JTf alone")
                    assert EP.same_bits_np(plan.frame_jtf(tq, tf, bodies, offsets, frame).double().cpu().numpy(), a[n_jv:].reshape(B_TOP, -1))


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "two_leaves"), ("tello_with_arms", "two_leaves")])
def test_capture_and_replay(name, kind, gpu):
    """one eager call of the same B and n on the stream, then the call captured; the replay reads new states from the same tensors and
    gives the bits of an eager call on them"""
    import graph_capture as GC

    B = 65
    for frame in FRAMES:
        tq, tv, tf = _tensors(name, kind, B, "f64", gpu)
        cap = GC.capture(lambda: _both(name, kind, frame, tq, tv, tf))
        try:
            print(f"captured nodes: {cap.nodes}")
            assert cap.nodes["memcpy"] == 0 and cap.nodes["kernel"] >= 1
            new = _tensors(name, kind, B, "f64", gpu, lo=B)
            for t, s in zip((tq, tv, tf), new):
                t.copy_(s)
            Jv, JTf = (o.cpu().numpy() for o in cap.replay())
            Jv_e, JTf_e = (o.cpu().numpy() for o in _both(name, kind, frame, *new))
            assert EP.same_bits_np(Jv, Jv_e) and EP.same_bits_np(JTf, JTf_e)
            Jv_ref, JTf_ref = products_ref(name, kind, frame, False)
            _held(Jv, Jv_ref[B:2 * B], EP.TOL64, f"{name} {frame} replayed Jv")
            _held(JTf, JTf_ref[B:2 * B], EP.TOL64, f"{name} {frame} replayed JTf")
        finally:
            cap.drop()


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "longest"), ("tello_with_arms", "two_leaves")])
def test_on_a_callers_stream(name, kind, gpu):
    import torch

    tq, tv, tf = _tensors(name, kind, B_TOP, "f64", gpu)
    Jv0, JTf0 = (o.cpu().numpy() for o in _both(name, kind, "world", tq, tv, tf))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    Jv, JTf = _both(name, kind, "world", tq, tv, tf, stream=s)
    s.synchronize()
    assert EP.same_bits_np(Jv.cpu().numpy(), Jv0) and EP.same_bits_np(JTf.cpu().numpy(), JTf0)


def test_route_one_in_three_chunks(gpu, monkeypatch):
    """tello_with_arms, two feet in the world frame, both products: per state the chunk's J and the nv rows of the expanded batch, so that
    the smallest budget, GRBDA_WORK_MAX_MB=1, holds less than two tiles and B = 130 goes through in three passes of 64, 64 and 2 states"""
    import torch

    import generalized_rbda_amd as G

    name, kind = "tello_with_arms", "two_leaves"
    plan = G.Plan(EP._model(name))
    plan.set_gravity(GRAVITY)
    bodies, offsets = lists(name)[kind]
    assert plan.frame_jacobians_route(bodies)[0] == 1 and plan.body_list_walk(bodies)[2] == 0
    n, arr, off = _c_list(name, kind)
    n12, nq, nv, ns = 12 * n, plan.nq, plan.nv, plan.n_span_vel
    per_state = (n12 + (nv + n12 + 2 * ns) + (6 * n * nv + nv * (nq + 2 * nv + n12 + 2 * ns))) * 8
    assert (1 << 20) // per_state < 128  # states per pass: one tile
    tq, tv, tf = _tensors(name, kind, B_TOP, "f64", gpu)
    Jv0, JTf0 = (o.cpu().numpy() for o in plan.frame_jacobian_products(tq, bodies, v=tv, f=tf, offsets=offsets, frame="world"))
    Jv = torch.full((B_TOP, n, 6), float("nan"), dtype=torch.float64, device=gpu)
    JTf = torch.full((B_TOP, nv), float("nan"), dtype=torch.float64, device=gpu)
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", "1")
    plan.release_work()
    torch.cuda.synchronize()
    try:
        plan._dispatch("frame_jacobian_products", torch.float64, tq.data_ptr(), tv.data_ptr(), tf.data_ptr(), n, arr, off, 1, Jv.data_ptr(), JTf.data_ptr(),
                       B_TOP, 0, None)
        torch.cuda.synchronize()
    finally:
        plan.release_work()
    assert EP.same_bits_np(Jv.cpu().numpy(), Jv0) and EP.same_bits_np(JTf.cpu().numpy(), JTf0)
    Jv_ref, JTf_ref = products_ref(name, kind, "world", False)
    _held(Jv.cpu().numpy(), Jv_ref, EP.TOL64, "three chunks Jv")
    _held(JTf.cpu().numpy(), JTf_ref, EP.TOL64, "three chunks JTf")


@pytest.mark.parametrize("name,kind", [("urdf_mini_cheetah", "two_leaves"), ("tello_with_arms", "two_leaves")])
def test_the_host_variant_agrees(name, kind, gpu):
    plan = plan_at_gravity(name)
    bodies, offsets = lists(name)[kind]
    q = every_body(name, False)[0]
    v, f = directions(name, kind, False)
    tq, tv, tf = _tensors(name, kind, B_TOP, "f64", gpu)
    for frame in FRAMES:
        Jv, JTf = (o.cpu().numpy() for o in _both(name, kind, frame, tq, tv, tf))
        Jv_h, JTf_h = plan.frame_jacobian_products_host(q, bodies, v=v, f=f, offsets=offsets, frame=frame)
        _held(Jv_h, Jv, 1e-12, f"{name} {frame} host Jv")
        _held(JTf_h, JTf, 1e-12, f"{name} {frame} host JTf")
        only = plan.frame_jacobian_products_host(q, bodies, f=f, offsets=offsets, frame=frame)
        assert only[0] is None
        _held(only[1], JTf, 1e-12, f"{name} {frame} host JTf alone")
