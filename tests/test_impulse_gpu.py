"""grbda_contact_impulse_* on the device against tests/impulse_ref.py (pinned by test_impulse_ref_cpu.py), every state on its own scale
1 + |ref|_inf, at B = 1, 65 and 130 (one state; one tile and one state; two tiles and a ragged third).  Draws: entry_points._states,
seed 73; the cases are impulse_ref.CASES.

fp64 at TOL64, qd_next and impulse: the force-propagation route of the inverse OSIM at 64 and 32 lanes (cheetah_n1 / n3 / n5, mu = 0), the
16-lane width with several contacts on one body (cheetah_n8, mu = 1e-3, v_des, e = 0.5), implicit clusters on the unit-wrench route
(tello_feet), a roll-pitch-yaw base, the spanning-tree route (two_parent), rank 12 of 24 (humanoid_soles, mu = 1e-3) -- and on the device
outputs alone J_w qd_next = v_des - e v- - mu impulse at 1e-8, through contact_points.
Energy on the device (grbda_energy_f64): e = 1, mu = 0 conserves the kinetic energy to TOL64; e = 0 never increases it.
fp32 at TOL32 on float32-rounded inputs against the fp64 reference (cheetah_feet, tello_feet); the measured worst is printed.
Then: qd_next == qd gives the bits of the out-of-place call; a chunked call (three chunks at least) equals the one-chunk call bit for bit; a
captured call replays the eager bits; the host-array variant equals the device call bit for bit; the singular set counts exactly the states
whose impulse is NaN, with qd_next NaN exactly there, and is finite with damping; qd_next and impulse keep to their buffers.

Measured on an MI355X: see DESIGN.md 7g'."""
import ctypes

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import generalized_rbda_amd as G
import impulse_ref as I

pytestmark = pytest.mark.gpu
BATCHES = (1, 65, 130)
B_TOP = I.B_TOP


def _dev(a, B, dtype, gpu):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a[:B]), dtype=dtype, device=gpu)


def _np(t):
    return t.detach().double().cpu().numpy()


def _plan(cid):
    return EP.plan_for(I.CASE[cid][1], I.CASE[cid][2])


FP64 = ["cheetah_n1", "cheetah_n3", "cheetah_n5", "cheetah_n8", "tello_feet", "cheetah_rpy2", "two_parent1", "humanoid_soles"]


@pytest.mark.parametrize("cid", FP64)
def test_contact_impulse_fp64(cid, gpu):
    import torch

    plan = _plan(cid)
    blob, bodies, offsets, (q, qd, vd), mu, e, ref = I.case(cid)
    for B in BATCHES:
        t = lambda a: _dev(a, B, torch.float64, gpu)
        G.spd_bad_pivots(0, reset=True)
        qn, imp = plan.contact_impulse(t(q), t(qd), bodies, offsets, v_des=t(vd), restitution=e, damping=mu)
        assert G.spd_bad_pivots(0, reset=True) == 0
        for what, g, r in (("qd_next", qn, ref["qd_next"]), ("impulse", imp, ref["impulse"])):
            err = C.rel_per_state(_np(g), r[:B])
            print(f"{cid} B={B} {what}: {err.max():.2e}")
            assert err.max() < EP.TOL64, (what, B, int(err.argmax()), err.max())
        # on the device outputs alone: the points leave with the velocity asked for
        before = _np(plan.contact_points(t(q), bodies, offsets, qd=t(qd))[1])
        after = _np(plan.contact_points(t(q), bodies, offsets, qd=qn)[1])
        want = (0.0 if vd is None else vd[:B]) - e * before - mu * _np(imp)
        err = C.rel_per_state(after, want)
        print(f"{cid} B={B} constraint: {err.max():.2e}")
        assert err.max() < 1e-8, (B, int(err.argmax()), err.max())


@pytest.mark.parametrize("cid", ["cheetah_feet", "tello_feet", "cheetah_n5"])
def test_energy_on_the_device(cid, gpu):
    """v_des = 0, mu = 0: e = 1 conserves 1/2 qd^T H qd, e = 0 never increases it (it drops by 1/2 v-^T A^-1 v- >= 0)"""
    import torch

    plan = _plan(cid)
    blob, bodies, offsets, (q, qd, _), _, _, _ = I.case(cid)
    tq, tqd = _dev(q, B_TOP, torch.float64, gpu), _dev(qd, B_TOP, torch.float64, gpu)
    before = _np(plan.energy(tq, tqd)[0])
    elastic = _np(plan.energy(tq, plan.contact_impulse(tq, tqd, bodies, offsets, restitution=1.0)[0])[0])
    plastic = _np(plan.energy(tq, plan.contact_impulse(tq, tqd, bodies, offsets, restitution=0.0)[0])[0])
    err = np.abs(elastic - before) / (1 + before)
    print(f"{cid}: e = 1 energy change {err.max():.2e}; e = 0 largest gain {(plastic - before).max():.2e} of {before.max():.2e}")
    assert err.max() < EP.TOL64, (int(err.argmax()), err.max())
    assert (plastic - before <= EP.TOL64 * (1 + before)).all(), "a plastic impact gained energy"
    assert (plastic < before).any()


# (case): (margin = twice the yardstick, measured worst, yardstick, cause) for fp32 cases that miss TOL32 -- as test_contact_gpu.MARGINS32
MARGINS32 = {}


@pytest.mark.parametrize("cid", ["cheetah_feet", "tello_feet"])
def test_contact_impulse_fp32(cid, gpu):
    import torch

    plan = _plan(cid)
    blob, bodies, offsets, (q, qd, vd), mu, e, ref = I.case(cid, True)
    t = lambda a: _dev(a, B_TOP, torch.float32, gpu)
    qn, imp = plan.contact_impulse(t(q), t(qd), bodies, offsets, v_des=t(vd), restitution=e, damping=mu)
    yard = I.contact_impulse_in(np.float32, ref, qd, vd, e, mu)
    tol = MARGINS32.get(cid, (EP.TOL32,))[0]
    for what, g, r, y in (("qd_next", qn, ref["qd_next"], yard[0]), ("impulse", imp, ref["impulse"], yard[1])):
        err = C.rel_per_state(_np(g), r)
        print(f"{cid} fp32 {what}: worst {err.max():.2e} (state {int(err.argmax())}); the closed form in float32: "
              f"{C.rel_per_state(y.astype(np.float64), r).max():.2e}")
        assert np.isfinite(_np(g)).all() and err.max() < tol, (what, int(err.argmax()), err.max())


def _raw_call(plan, tq, tqd, tvd, bodies, offsets, e, mu, qd_next, impulse, B):
    import torch

    n = len(bodies)
    bod, off = (ctypes.c_int * n)(*bodies), (ctypes.c_double * (3 * n))(*[x for o in offsets for x in o])
    fn = getattr(G.lib(), "grbda_contact_impulse_" + ("f32" if tq.dtype == torch.float32 else "f64"))
    rc = fn(plan._h, tq.data_ptr(), tqd.data_ptr(), n, bod, off, None if tvd is None else tvd.data_ptr(), e, mu, qd_next.data_ptr(),
            impulse.data_ptr(), B, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, G.lib().grbda_last_error()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_in_place_gives_the_bits_of_the_out_of_place_call(dtype, gpu):
    import torch

    cid, td = "cheetah_n3", (torch.float32 if dtype == "f32" else torch.float64)
    plan = _plan(cid)
    blob, bodies, offsets, (q, qd, vd), mu, e, _ = I.case(cid, dtype == "f32")
    tq, tqd, tvd = (_dev(a, B_TOP, td, gpu) for a in (q, qd, vd))
    qn, imp = plan.contact_impulse(tq, tqd, bodies, offsets, v_des=tvd, restitution=e, damping=mu)
    io, imp2 = tqd.clone(), torch.full_like(imp, float("nan"))
    _raw_call(plan, tq, io, tvd, bodies, offsets, e, mu, io, imp2, B_TOP)
    torch.cuda.synchronize()
    assert np.isfinite(_np(qn)).all() and not torch.equal(qn, tqd)
    assert torch.equal(io, qn) and torch.equal(imp2, imp)


def test_chunked_call_equals_the_one_chunk_call(gpu, monkeypatch):
    """in place too: a chunk reads its rows of qd before it writes them"""
    import torch

    from test_chunk_seams_gpu import CAP_MB

    cid = "cheetah_feet"
    plan = G.Plan(I.case(cid)[0])
    blob, bodies, offsets, (q, qd, vd), mu, e, _ = I.case(cid)
    tq, tqd, tvd = (_dev(a, B_TOP, torch.float64, gpu) for a in (q, qd, vd))
    call = lambda: plan.contact_impulse(tq, tqd, bodies, offsets, v_des=tvd, restitution=e, damping=mu)
    whole = [_np(o) for o in call()]
    torch.cuda.synchronize()
    held = plan.release_work()
    per_state = (held - 256) // ((B_TOP + 63) // 64 * 64)
    assert held > (CAP_MB << 20) + 256, "the batch fits the cap in one chunk: nothing is tested"
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", str(CAP_MB))
    chunked = [_np(o) for o in call()]
    io, imp = tqd.clone(), torch.empty((B_TOP, len(bodies), 3), dtype=torch.float64, device=gpu)
    _raw_call(plan, tq, io, tvd, bodies, offsets, e, mu, io, imp, B_TOP)
    torch.cuda.synchronize()
    capped = plan.release_work()
    assert 0 < capped < held
    chunk = (capped - 256) // per_state
    assert -(-B_TOP // chunk) >= 3, f"{B_TOP} states in chunks of {chunk}: fewer than three chunks"
    for a, b in zip(chunked, whole):
        assert np.array_equal(a, b), "the chunked call differs from the one-chunk call"
    assert np.array_equal(_np(io), whole[0]) and np.array_equal(_np(imp), whole[1]), "the chunked in-place call differs"


def test_graph_capture_replays_the_eager_bits(gpu):
    import torch

    from graph_capture import capture

    cid = "cheetah_feet"
    plan = G.Plan(I.case(cid)[0])
    blob, bodies, offsets, (q, qd, vd), mu, e, _ = I.case(cid, True)
    B = 65
    x = [_dev(a, B, torch.float32, gpu) for a in (q, qd, vd)]
    call = lambda: plan.contact_impulse(x[0], x[1], bodies, offsets, v_des=x[2], restitution=e, damping=mu)
    cap = capture(call)
    try:
        assert cap.nodes["kernel"] >= 7  # poses, spanning rates, twists, inverse OSIM, solve, two forward dynamics, finish
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

    cid = "cheetah_n3"
    plan = _plan(cid)
    blob, bodies, offsets, (q, qd, vd), mu, e, _ = I.case(cid)
    B, n, nv = 3, len(bodies), plan.nv
    t = lambda a: _dev(a, B, torch.float64, gpu)
    want = [_np(o) for o in plan.contact_impulse(t(q), t(qd), bodies, offsets, v_des=t(vd), restitution=e, damping=mu)]
    h = [np.ascontiguousarray(a[:B], dtype=np.float64) for a in (q, qd, vd)]
    qn, imp = np.empty((B, nv)), np.empty((B, n, 3))
    p = lambda a: a.ctypes.data_as(c_void_p)
    fn = G.lib().grbda_contact_impulse_host_f64
    bod, off = (c_int * n)(*bodies), (c_double * (3 * n))(*[x for o in offsets for x in o])
    assert fn(plan._h, p(h[0]), p(h[1]), n, bod, off, p(h[2]), e, mu, p(qn), p(imp), B, 0) == 0
    assert np.array_equal(qn, want[0]) and np.array_equal(imp, want[1])
    # in place on the host
    io = h[1].copy()
    assert fn(plan._h, p(h[0]), p(io), n, bod, off, p(h[2]), e, mu, p(io), p(imp), B, 0) == 0
    assert np.array_equal(io, want[0])


def test_singular_set_is_counted_state_by_state(gpu):
    """one contact on the last link of the fixed-base chain whose joint axes are all z (test_contact_solve_gpu.chain_case: row 2 of
    J_w H^-1 J_w^T is made of exact zeros): without damping every state has a pivot that is not positive"""
    import torch

    cid = "chain1_damped"
    plan = _plan(cid)
    blob, bodies, offsets, (q, qd, _), mu, e, ref = I.case(cid)
    A0 = ref["A"] - mu * np.eye(3)[None]
    assert (A0[:, 2, :] == 0).all()
    B = B_TOP
    t = lambda a: _dev(a, B, torch.float64, gpu)
    G.spd_bad_pivots(0, reset=True)
    qn, imp = plan.contact_impulse(t(q), t(qd), bodies, offsets, damping=0.0)
    bad = G.spd_bad_pivots(0, reset=True)
    nan_imp = np.isnan(_np(imp)).reshape(B, -1).any(axis=1)
    nan_qn = np.isnan(_np(qn)).reshape(B, -1).any(axis=1)
    print(f"{cid} mu = 0: {bad} of {B} states counted, {int(nan_imp.sum())} with NaN impulses")
    assert bad == int(nan_imp.sum()) and bad > 0
    assert np.array_equal(nan_qn, nan_imp), "qd_next is NaN in other states than impulse"
    assert np.isnan(_np(imp))[nan_imp].all() and np.isfinite(_np(qn))[~nan_qn].all()
    # the same set with damping is finite everywhere, and right
    qn, imp = plan.contact_impulse(t(q), t(qd), bodies, offsets, damping=mu)
    assert G.spd_bad_pivots(0, reset=True) == 0
    assert np.isfinite(_np(qn)).all() and np.isfinite(_np(imp)).all()
    for what, g, r in (("qd_next", qn, ref["qd_next"]), ("impulse", imp, ref["impulse"])):
        err = C.rel_per_state(_np(g), r)
        assert err.max() < EP.TOL64, (what, int(err.argmax()), err.max())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 65])
def test_outputs_keep_to_their_buffers(B, dtype, gpu):
    """qd_next and impulse in arenas of guarded.py with a misaligned lead: both bands intact, every element written, inputs untouched"""
    import torch

    import guarded

    cid, td = "cheetah_n3", (torch.float32 if dtype == "f32" else torch.float64)
    plan = _plan(cid)
    blob, bodies, offsets, (q, qd, vd), mu, e, ref = I.case(cid, dtype == "f32")
    lead = 1
    x = [guarded.place(a[:B], td, gpu, lead) for a in (q, qd, vd)]
    before = [guarded.snapshot(v) for v in x]
    with guarded.guarded_outputs(lead) as made:
        qn, imp = plan.contact_impulse(x[0], x[1], bodies, offsets, v_des=x[2], restitution=e, damping=mu)
    torch.cuda.synchronize()
    assert len(made) == 2
    for a in made:
        assert guarded.check(a) == 0, f"{tuple(a.shape)}: elements never written"
    for v, b in zip(x, before):
        assert guarded.same_bits(v, b), "an input changed"
    tol = EP.TOL32 if dtype == "f32" else EP.TOL64
    for what, g, r in (("qd_next", qn, ref["qd_next"]), ("impulse", imp, ref["impulse"])):
        err = C.rel_per_state(_np(g), r[:B])
        assert err.max() < tol, (what, int(err.argmax()), err.max())
    # in place, qd itself in an arena: the bands around it stay
    io = guarded.place(qd[:B], td, gpu, lead)
    imp2 = guarded.arena((B, len(bodies), 3), td, gpu, lead)
    _raw_call(plan, x[0], io, x[2], bodies, offsets, e, mu, io, imp2, B)
    torch.cuda.synchronize()
    assert guarded.check(io) == 0 and guarded.check(imp2) == 0
    assert torch.equal(io, qn) and torch.equal(imp2, imp)
