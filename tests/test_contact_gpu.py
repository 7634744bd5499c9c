"""grbda_contact_points_* and grbda_contact_dynamics_* on the device against tests/contact_ref.py (held to the oracle by
test_contact_ref_cpu.py), every state on its own scale 1 + |ref|_inf, at B = 1, 65 and 130 (one state; one tile and one state; two tiles
and a ragged third).  Draws: entry_points._states, seed 61.

fp64 at TOL64: contact_points (pos / vel / acc apart) on a quaternion and a roll-pitch-yaw base, implicit clusters, a fixed base and the
two spanning-tree models; contact_dynamics (ydd, lambda, ydd_free) on the force-propagation and the unit-wrench route of the inverse
OSIM, implicit clusters, one and eight contacts (the latter redundant: damping 1e-3, with external forces), the spanning-tree route --
and on the device outputs alone p_ddot(ydd) + mu lambda = a_des at 1e-8.
fp32 at TOL32 on float32-rounded inputs against the fp64 reference (the two sets with cond(A) <= 2.4e2); the measured worst is printed.
Then: the singular solve is counted or finite (and counts exactly the states whose lambda is NaN, ydd_free finite), a chunked call equals the one-chunk call bit for bit, a captured call replays the eager
bits, and the host-array variant equals the device call bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import generalized_rbda_amd as G
import term_states as TS

pytestmark = pytest.mark.gpu
BATCHES = (1, 65, 130)
B_TOP = BATCHES[-1]
SEED = 61


def _last_link(blob):
    """the last body that is not a rotor"""
    import struct

    m = EP.K._parse(blob)
    n_ints, n_dbls, n_names = struct.unpack_from("<3i", blob, 28)
    off = 96 + 416 * m["nb"] + 64 * m["nc"] + 4 * ((n_ints + 1) & ~1) + 8 * n_dbls
    names = [n.decode() for n in blob[off: off + n_names].split(b"\0")[: m["nb"]]]
    links = [i for i, n in enumerate(names) if "rotor" not in n.lower()]
    return links[-1] if links else m["nb"] - 1


@functools.lru_cache(maxsize=None)
def points_of(name):
    """(bodies, offsets) of the contact_points case `name`"""
    blob = EP._model(name)
    if name == "urdf_mini_cheetah":
        return C.contact_set("cheetah_feet")[1:]
    if name == "tello_with_arms":
        return C.contact_set("tello_feet")[1:]
    if name == "urdf_mini_cheetah_rpy":
        return [C.body_index(blob, "FR_knee_link"), C.body_index(blob, "FL_knee_link")], [(0.0, 0.0, -0.2), (0.05, -0.02, 0.1)]
    return [_last_link(blob)], [(0.05, -0.02, 0.1)]


@functools.lru_cache(maxsize=None)
def draw(name, rounded=False):
    q, qd, x = EP._states(EP._model(name), B_TOP, SEED)
    return tuple(TS._frozen(TS.fp32_rounded(a) if rounded else a) for a in (q, qd, x))


def _dev(a, B, dtype, gpu):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a[:B]), dtype=dtype, device=gpu)


def _np(t):
    return t.detach().double().cpu().numpy()


POINT_MODELS = ["urdf_mini_cheetah", "tello_with_arms", "urdf_mini_cheetah_rpy", "rev_rotor_chain_4", "two_parent", "parallel_chain_exp_d10_l16"]


@pytest.mark.parametrize("name", POINT_MODELS)
def test_contact_points_fp64(name, gpu):
    import torch

    blob, plan = EP._model(name), EP.plan_for(name, ())
    bodies, offsets = points_of(name)
    q, qd, ydd = draw(name)
    ref = C.contact_points(blob, q, bodies, offsets, qd, ydd)
    for B in BATCHES:
        t = lambda a: _dev(a, B, torch.float64, gpu)
        tq, tqd, tydd = t(q), t(qd), t(ydd)
        got = plan.contact_points(tq, bodies, offsets, qd=tqd, ydd=tydd)
        for what, g, r in zip(("pos", "vel", "acc"), got, ref):
            err = C.rel_per_state(_np(g), r[:B])
            print(f"{name} B={B} {what}: {err.max():.2e}")
            assert err.max() < EP.TOL64, (what, B, int(err.argmax()), err.max())
        # acc alone, and pos alone (no rates given), give the same bits
        fn = G.lib().grbda_contact_points_f64
        acc = torch.empty_like(got[2])
        n = len(bodies)
        bod, off = (ctypes.c_int * n)(*bodies), (ctypes.c_double * (3 * n))(*[x for o in offsets for x in o])
        rc = fn(plan._h, tq.data_ptr(), tqd.data_ptr(), tydd.data_ptr(), n, bod, off, None, None, acc.data_ptr(), B, 0,
                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(acc, got[2])
        pos, vel, none = plan.contact_points(tq, bodies, offsets)
        assert vel is None and none is None and torch.equal(pos, got[0])
        _, vel, none = plan.contact_points(tq, bodies, offsets, qd=tqd)
        assert none is None and torch.equal(vel, got[1])


# (id, model, plan-time switches, contact set or None = one point on the last link, damping, external forces, random a_des)
DYNAMICS = [
    ("cheetah4", "urdf_mini_cheetah", (), "cheetah_feet", 0.0, False, True),
    ("cheetah4_unit_wrench", "urdf_mini_cheetah", (("GRBDA_NO_EFPA", "1"),), "cheetah_feet", 0.0, False, False),
    ("tello2", "tello_with_arms", (), "tello_feet", 0.0, False, True),
    ("cheetah1", "urdf_mini_cheetah", (), "cheetah_one", 0.0, False, False),
    ("humanoid8_damped_fext", "urdf_mit_humanoid", (), "humanoid_soles", 1e-3, True, True),
    ("two_parent1", "two_parent", (), None, 0.0, False, False),
]


@functools.lru_cache(maxsize=None)
def dynamics_case(cid, rounded=False):
    """inputs and the fp64 reference of B_TOP states, computed once per process and never written to"""
    _, name, env, key, mu, fext, rand = next(c for c in DYNAMICS if c[0] == cid)
    blob = EP._model(name)
    bodies, offsets = C.contact_set(key)[1:] if key else points_of(name)
    q, qd, tau = draw(name, rounded)
    rng = np.random.default_rng(SEED)
    rnd = lambda a: TS.fp32_rounded(a) if rounded else a
    fe = rnd(rng.uniform(-1, 1, (B_TOP, EP.K._parse(blob)["nb"], 6))) if fext else None
    ad = rnd(rng.uniform(-1, 1, (B_TOP, len(bodies), 3))) if rand else None
    ref = C.contact_dynamics(blob, q, qd, tau, bodies, offsets, ad, mu, fe)
    return blob, bodies, offsets, (q, qd, tau, fe, ad), ref


@pytest.mark.parametrize("case", DYNAMICS, ids=[c[0] for c in DYNAMICS])
def test_contact_dynamics_fp64(case, gpu):
    import torch

    cid, name, env, key, mu = case[:5]
    plan = EP.plan_for(name, env)
    blob, bodies, offsets, (q, qd, tau, fe, ad), ref = dynamics_case(cid)
    for B in BATCHES:
        t = lambda a: _dev(a, B, torch.float64, gpu)
        ydd, lam, free = plan.contact_dynamics(t(q), t(qd), t(tau), bodies, offsets, a_des=t(ad), damping=mu, f_ext=t(fe))
        for what, g, r in (("ydd", ydd, ref["ydd"]), ("lambda", lam, ref["lam"]), ("ydd_free", free, ref["ydd_free"])):
            err = C.rel_per_state(_np(g), r[:B])
            print(f"{cid} B={B} {what}: {err.max():.2e}")
            assert err.max() < EP.TOL64, (what, B, int(err.argmax()), err.max())
        # on the device outputs alone: the points have the acceleration asked for
        acc = plan.contact_points(t(q), bodies, offsets, qd=t(qd), ydd=ydd)[2]
        want = np.zeros((B, len(bodies), 3)) if ad is None else ad[:B]
        err = C.rel_per_state(_np(acc) + mu * _np(lam), want)
        print(f"{cid} B={B} constraint: {err.max():.2e}")
        assert err.max() < 1e-8, (B, int(err.argmax()), err.max())


# (case): (margin = twice the measured worst, measured worst, cause) for fp32 cases that miss TOL32 -- as test_kinematics_gpu.MARGINS
MARGINS32 = {}


@pytest.mark.parametrize("cid", ["cheetah4", "tello2"])
def test_contact_dynamics_fp32(cid, gpu):
    import torch

    _, name, env, key, mu = next(c for c in DYNAMICS if c[0] == cid)[:5]
    plan = EP.plan_for(name, env)
    blob, bodies, offsets, (q, qd, tau, fe, ad), ref = dynamics_case(cid, True)
    t = lambda a: _dev(a, B_TOP, torch.float32, gpu)
    ydd, lam, free = plan.contact_dynamics(t(q), t(qd), t(tau), bodies, offsets, a_des=t(ad), damping=mu, f_ext=t(fe))
    tol = MARGINS32.get(cid, (EP.TOL32,))[0]
    for what, g, r in (("ydd", ydd, ref["ydd"]), ("lambda", lam, ref["lam"]), ("ydd_free", free, ref["ydd_free"])):
        err = C.rel_per_state(_np(g), r)
        print(f"{cid} fp32 {what}: worst {err.max():.2e} (state {int(err.argmax())})")
        assert np.isfinite(_np(g)).all() and err.max() < tol, (what, int(err.argmax()), err.max())


def test_singular_solve_is_counted_or_finite(gpu):
    import torch

    plan = EP.plan_for("urdf_mit_humanoid", ())
    blob, bodies, offsets, (q, qd, tau, fe, ad), _ = dynamics_case("humanoid8_damped_fext")
    B = 65
    t = lambda a: _dev(a, B, torch.float64, gpu)
    G.spd_bad_pivots(0, reset=True)
    outs = plan.contact_dynamics(t(q), t(qd), t(tau), bodies, offsets, damping=0.0)
    bad = G.spd_bad_pivots(0, reset=True)
    finite = all(np.isfinite(_np(o)).all() for o in outs)
    print(f"rank-deficient contacts without damping: {bad} states counted, outputs finite: {finite}")
    assert bad > 0 or finite
    # the contract state by state: a counted state is a state whose lambda is NaN, and ydd_free is untouched by the solve
    nan_states = int(np.isnan(_np(outs[1])).reshape(B, -1).any(axis=1).sum())
    assert bad == nan_states, f"{bad} states counted, {nan_states} states with NaN in lambda"
    assert np.isfinite(_np(outs[2])).all(), "ydd_free is not finite"


def test_chunked_call_equals_the_one_chunk_call(gpu, monkeypatch):
    import torch

    from test_chunk_seams_gpu import CAP_MB

    plan = G.Plan(EP._model("urdf_mini_cheetah"))
    blob, bodies, offsets, (q, qd, tau, fe, ad), _ = dynamics_case("cheetah4")
    t = lambda a: _dev(a, B_TOP, torch.float64, gpu)
    call = lambda: plan.contact_dynamics(t(q), t(qd), t(tau), bodies, offsets, a_des=t(ad))
    whole = [_np(o) for o in call()]
    torch.cuda.synchronize()
    assert plan.release_work() > (CAP_MB << 20) + 256, "the batch fits the cap in one chunk: nothing is tested"
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", str(CAP_MB))
    chunked = [_np(o) for o in call()]
    torch.cuda.synchronize()
    assert 0 < plan.release_work() <= (CAP_MB << 20) + 256
    for a, b in zip(chunked, whole):
        assert np.array_equal(a, b), "the chunked call differs from the one-chunk call"


def test_graph_capture_replays_the_eager_bits(gpu):
    import torch

    from graph_capture import capture

    plan = G.Plan(EP._model("urdf_mini_cheetah"))
    blob, bodies, offsets, (q, qd, tau, fe, ad), _ = dynamics_case("cheetah4", True)
    B = 65
    x = [_dev(a, B, torch.float32, gpu) for a in (q, qd, tau, ad)]
    call = lambda: plan.contact_dynamics(x[0], x[1], x[2], bodies, offsets, a_des=x[3])
    cap = capture(call)
    try:
        assert cap.nodes["kernel"] >= 6
        got = [_np(o) for o in cap.replay()]
        with torch.cuda.stream(cap.stream):
            want = [_np(o) for o in call()]
        cap.stream.synchronize()
        for a, b in zip(got, want):
            assert np.isfinite(a).all() and np.array_equal(a, b)
    finally:
        cap.drop()


def test_host_variant_equals_the_device_call(gpu):
    import torch
    from ctypes import c_double, c_int, c_void_p

    plan = EP.plan_for("urdf_mini_cheetah", ())
    blob, bodies, offsets, (q, qd, tau, fe, ad), _ = dynamics_case("cheetah4")
    B, n, nv = 3, len(bodies), plan.nv
    t = lambda a: _dev(a, B, torch.float64, gpu)
    want = [_np(o) for o in plan.contact_dynamics(t(q), t(qd), t(tau), bodies, offsets, a_des=t(ad))]
    h = [np.ascontiguousarray(a[:B], dtype=np.float64) for a in (q, qd, tau, ad)]
    ydd, lam, free = np.empty((B, nv)), np.empty((B, n, 3)), np.empty((B, nv))
    p = lambda a: a.ctypes.data_as(c_void_p)
    fn = G.lib().grbda_contact_dynamics_host_f64
    rc = fn(plan._h, p(h[0]), p(h[1]), p(h[2]), None, n, (c_int * n)(*bodies), (c_double * (3 * n))(*[x for o in offsets for x in o]), p(h[3]),
            0.0, p(ydd), p(lam), p(free), B, 0)
    assert rc == 0
    for a, b in zip((ydd, lam, free), want):
        assert np.array_equal(a, b)
    # the points likewise
    pos, vel, acc = (np.empty((B, n, 3)) for _ in range(3))
    fp = G.lib().grbda_contact_points_host_f64
    rc = fp(plan._h, p(h[0]), p(h[1]), p(ydd), n, (c_int * n)(*bodies), (c_double * (3 * n))(*[x for o in offsets for x in o]), p(pos), p(vel),
            p(acc), B, 0)
    assert rc == 0
    dev = plan.contact_points(t(q), bodies, offsets, qd=t(qd), ydd=t(ydd))
    for a, b in zip((pos, vel, acc), dev):
        assert np.array_equal(a, _np(b))
