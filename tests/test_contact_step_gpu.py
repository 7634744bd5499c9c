"""The scheduled contacts (include/grbda_hip_contact_step.h) on the device against tests/contact_step_ref.py (held to the pinned
references by test_contact_step_ref_cpu.py), every state on its own scale 1 + |ref|_inf, at B = 1, 65 and 130: one state; a wavefront
plus one; and, at the 16 lanes of fp64 with 8 contacts, more than eight workgroups with a ragged last one.  State b carries the mask
b mod 2^n, shuffled with a fixed seed, so every wavefront mixes empty, partial and full sets.  Draws: entry_points._states, seed 67.

fp64 at TOL64: contact_dynamics_active (random a_des, at kd = 0 and at kd = 1 / dt), contact_impulse_active (random v_des, e = 0.25) and contact_step
(kd = 1 / dt, a previous mask drawn with another seed, e = 0.25) on the Mini Cheetah's four feet, Tello's two feet (implicit clusters: a
fallback route of the sparse-wrench call), one point on a fixed-base chain, the eight sole corners of the MIT Humanoid (redundant, damping
1e-3), and a list with a rotor contact (unit-wrench OSIM route, dense wrench route).
fp32 at TOL32 on float32-rounded inputs against the fp64 helper, the two well-conditioned sets; the measured worst is printed.
Exact properties on NaN-seeded outputs; the full mask against Plan.contact_dynamics; the step against its three calls and the rollout
against its steps, bit for bit; a NULL prev_active enqueues no impulse stage (kernel nodes of a captured graph); three chunks equal one;
a captured call replays the eager bits; a caller's stream; in-place q_next / qd_next; the host variant."""
import ctypes
import functools

import numpy as np
import pytest

import contact_ref as C
import contact_step_ref as S
import entry_points as EP
import generalized_rbda_amd as G
import term_states as TS

pytestmark = pytest.mark.gpu
BATCHES = (1, 65, 130)
B_TOP = BATCHES[-1]
SEED = 67
RESTITUTION = 0.25


def _rotor_list(blob):
    """the last link of the chain and its first rotor, a point on each"""
    import struct

    from test_contact_gpu import _last_link

    m = EP.K._parse(blob)
    n_ints, n_dbls, n_names = struct.unpack_from("<3i", blob, 28)
    off = 96 + 416 * m["nb"] + 64 * m["nc"] + 4 * ((n_ints + 1) & ~1) + 8 * n_dbls
    names = [n.decode() for n in blob[off: off + n_names].split(b"\0")[: m["nb"]]]
    rotor = next(i for i, n in enumerate(names) if "rotor" in n.lower())
    return [_last_link(blob), rotor], [(0.05, -0.02, 0.1), (0.01, 0.02, -0.03)]


# (id, model, contact set of contact_ref.SETS / "point" = test_contact_gpu.points_of / "rotor", damping)
CASES = [
    ("cheetah_feet", "urdf_mini_cheetah", "cheetah_feet", 0.0),
    ("tello_feet", "tello_with_arms", "tello_feet", 0.0),
    ("chain_point", "rev_rotor_chain_4", "point", 1e-3),
    ("humanoid_soles", "urdf_mit_humanoid", "humanoid_soles", 1e-3),
    ("chain_rotor", "rev_rotor_chain_4", "rotor", 1e-3),
]
CASE = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def inputs(cid, rounded=False):
    """(blob, bodies, offsets, damping, dt, dict of the arrays of B_TOP states), drawn once per process and never written to"""
    from test_contact_gpu import points_of

    _, name, key, mu = CASE[cid]
    blob = EP._model(name)
    bodies, offsets = points_of(name) if key == "point" else _rotor_list(blob) if key == "rotor" else C.contact_set(key)[1:]
    bodies, offsets, n = list(bodies), [tuple(o) for o in offsets], len(bodies)
    rnd = TS.fp32_rounded if rounded else (lambda a: a)
    q, qd, tau = (TS._frozen(rnd(a)) for a in EP._states(blob, B_TOP, SEED))
    rng = np.random.default_rng(SEED)
    x = dict(q=q, qd=qd, tau=tau, a_des=TS._frozen(rnd(rng.uniform(-1, 1, (B_TOP, n, 3)))), v_des=TS._frozen(rnd(rng.uniform(-1, 1, (B_TOP, n, 3)))),
             active=S.shuffled_masks(B_TOP, n, 0), prev=S.shuffled_masks(B_TOP, n, 1))
    return blob, bodies, offsets, mu, EP._dt(blob), x


@functools.lru_cache(maxsize=None)
def reference(cid, rounded=False):
    """(dynamics with a_des at kd = 0 and at kd = 1 / dt, impulse with v_des, step with kd = 1 / dt) of the helper, computed once per process"""
    blob, bodies, offsets, mu, dt, x = inputs(cid, rounded)
    dyn = tuple(S.contact_dynamics_active(blob, x["q"], x["qd"], x["tau"], bodies, offsets, x["active"], x["a_des"], kd, mu) for kd in (0.0, 1.0 / dt))
    imp = S.contact_impulse_active(blob, x["q"], x["qd"], bodies, offsets, x["active"], x["v_des"], RESTITUTION, mu)
    step = S.contact_step(blob, x["q"], x["qd"], x["tau"], bodies, offsets, x["active"], x["prev"], 1.0 / dt, RESTITUTION, mu, dt)
    return dyn, imp, step


def _dev(a, B, dtype, gpu):
    import torch

    if a is None:
        return None
    return torch.as_tensor(np.ascontiguousarray(a[:B]), dtype=torch.int32 if a.dtype.kind == "i" else dtype, device=gpu)


def _np(t):
    return t.detach().double().cpu().numpy()


def _hold(cid, what, got, ref, tol, rows=None):
    err = C.rel_per_state(_np(got) if hasattr(got, "detach") else got, ref)
    if rows is not None:
        err = err[rows]
    print(f"{cid} {what}: worst {err.max():.2e} (state {int(err.argmax())})")
    assert err.max() < tol, (cid, what, int(err.argmax()), err.max())


def _hold_all(cid, B, dtype, gpu, tol):
    import integrate_ref as R
    import test_integrate_gpu as TI

    blob, bodies, offsets, mu, dt, x = inputs(cid, tol > 1e-6)
    dyn, imp, step = reference(cid, tol > 1e-6)
    plan = EP.plan_for(CASE[cid][1], ())
    t = lambda k: _dev(x[k], B, dtype, gpu)
    for kd, ref in zip((0.0, 1.0 / dt), dyn):
        ydd, lam, free = plan.contact_dynamics_active(t("q"), t("qd"), t("tau"), bodies, offsets, t("active"), a_des=t("a_des"), kd=kd, damping=mu)
        for what, g, r in (("ydd", ydd, ref["ydd"]), ("lambda", lam, ref["lam"]), ("ydd_free", free, ref["ydd_free"])):
            _hold(cid, f"B={B} dynamics kd={kd:g} {what}", g, r[:B], tol)
    vn, impulse = plan.contact_impulse_active(t("q"), t("qd"), bodies, offsets, t("active"), v_des=t("v_des"), restitution=RESTITUTION, damping=mu)
    _hold(cid, f"B={B} impulse qd_next", vn, imp["qd_next"][:B], tol)
    _hold(cid, f"B={B} impulse", impulse, imp["impulse"][:B], tol)
    qn, vn, ydd, lam, impulse, ok = plan.contact_step(t("q"), t("qd"), t("tau"), bodies, offsets, t("active"), dt, prev_active=t("prev"), kd=1.0 / dt,
                                                      restitution=RESTITUTION, damping=mu)
    rok = step["ok"][:B]
    assert rok.any()
    qn = TI.quat_sign_aligned(_np(qn), step["q_next"][:B], R.column_kinds(blob))
    for what, g, r in (("ydd", ydd, step["ydd"]), ("lambda", lam, step["lam"]), ("impulse", impulse, step["impulse"]), ("qd_next", vn, step["qd_next"]),
                       ("q_next", qn, step["q_next"])):
        _hold(cid, f"B={B} step {what}", g, r[:B], tol, rows=None if what != "q_next" else rok)
    if tol < 1e-6:
        TI.check_flags(_np(ok) != 0, rok, step["phi"][:B], R.TOL, f"{cid} step")


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_fp64_against_the_helper(cid, gpu):
    import torch

    for B in BATCHES:
        _hold_all(cid, B, torch.float64, gpu, EP.TOL64)


# (case): (margin = twice the measured worst, measured worst, cause) for fp32 cases that miss TOL32 -- as test_contact_gpu.MARGINS32
MARGINS32 = {}


@pytest.mark.parametrize("cid", ["cheetah_feet", "tello_feet"])
def test_fp32_against_the_helper(cid, gpu):
    import torch

    _hold_all(cid, B_TOP, torch.float32, gpu, MARGINS32.get(cid, (EP.TOL32,))[0])


def _raw(plan, stem, dtype, args, B):
    """grbda_<stem>_<precision>(plan, args..., B, 0, the current stream) on tensors the test allocated itself"""
    import torch

    fn = getattr(G.lib(), f"grbda_{stem}_{'f32' if dtype == torch.float32 else 'f64'}")
    rc = fn(plan._h, *[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args], B, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, G.lib().grbda_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_exact_properties_on_nan_seeded_outputs(precision, gpu):
    import torch

    dtype = torch.float32 if precision == "f32" else torch.float64
    blob, bodies, offsets, mu, dt, x = inputs("cheetah_feet", precision == "f32")
    plan = EP.plan_for("urdf_mini_cheetah", ())
    B, n, nv = B_TOP, len(bodies), plan.nv
    t = lambda k: _dev(x[k], B, dtype, gpu)
    c = plan._contacts(bodies, offsets)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=dtype, device=gpu)
    on = ((x["active"][:, None] >> np.arange(n)[None]) & 1).astype(bool)  # [B, n]
    empty = x["active"] == 0
    assert empty.any() and on.all(axis=1).any() and (on.any(axis=1) & ~on.all(axis=1)).any()
    G.spd_bad_pivots(0, reset=True)
    ydd, lam, free = nan(B, nv), nan(B, n, 3), nan(B, nv)
    q, qd, tau, act = t("q"), t("qd"), t("tau"), t("active")
    _raw(plan, "contact_dynamics_active", dtype, (q, qd, tau, *c, act, t("a_des"), 1.0 / dt, mu, ydd, lam, free), B)
    assert torch.isfinite(ydd).all() and torch.isfinite(lam).all() and torch.isfinite(free).all()
    assert (lam.cpu().numpy()[~on] == 0).all() and (lam.cpu().numpy()[on] != 0).all()
    assert torch.equal(ydd[torch.as_tensor(empty)], free[torch.as_tensor(empty)])
    assert not torch.equal(ydd[torch.as_tensor(~empty)], free[torch.as_tensor(~empty)])
    vn, imp = nan(B, nv), nan(B, n, 3)
    _raw(plan, "contact_impulse_active", dtype, (q, qd, *c, act, t("v_des"), RESTITUTION, mu, vn, imp), B)
    assert torch.isfinite(vn).all() and (imp.cpu().numpy()[~on] == 0).all() and (imp.cpu().numpy()[on] != 0).all()
    assert EP.same_bits_np(vn.cpu().numpy()[empty], qd.cpu().numpy()[empty])
    assert G.spd_bad_pivots(0, reset=True) == 0


def test_bad_pivots_count_the_nan_states_and_never_an_empty_set(gpu):
    import torch

    blob, bodies, offsets, mu, dt, x = inputs("humanoid_soles")
    plan = EP.plan_for("urdf_mit_humanoid", ())
    B = B_TOP
    t = lambda k: _dev(x[k], B, torch.float64, gpu)
    G.spd_bad_pivots(0, reset=True)
    ydd, lam, free = plan.contact_dynamics_active(t("q"), t("qd"), t("tau"), bodies, offsets, t("active"), damping=0.0)  # rank-deficient, undamped
    torch.cuda.synchronize()
    bad = G.spd_bad_pivots(0, reset=True)
    nan_states = np.isnan(_np(lam)).reshape(B, -1).any(axis=1)
    print(f"undamped sole corners: {bad} states counted, {int(nan_states.sum())} with NaN in lambda")
    assert bad == int(nan_states.sum())
    empty = (x["active"] & 0xFF) == 0
    assert empty.any() and not nan_states[empty].any() and np.isfinite(_np(ydd)[empty]).all() and np.isfinite(_np(free)).all()
    on = ((x["active"][:, None] >> np.arange(len(bodies))[None]) & 1).astype(bool)
    assert (_np(lam)[~on] == 0).all()  # (exactly zero off the set in a counted state too)
    # the impulse entry with an all-empty schedule: nothing can be counted
    vn, imp = plan.contact_impulse_active(t("q"), t("qd"), bodies, offsets, torch.zeros(B, dtype=torch.int32, device=gpu), damping=0.0)
    torch.cuda.synchronize()
    assert G.spd_bad_pivots(0, reset=True) == 0 and EP.same_bits_np(_np(vn), _np(t("qd"))) and not _np(imp).any()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_full_mask_agrees_with_contact_dynamics(precision, gpu):
    import torch

    dtype, tol = (torch.float32, EP.TOL32) if precision == "f32" else (torch.float64, EP.TOL64)
    blob, bodies, offsets, mu, dt, x = inputs("cheetah_feet", precision == "f32")
    plan = EP.plan_for("urdf_mini_cheetah", ())
    t = lambda k: _dev(x[k], B_TOP, dtype, gpu)
    full = torch.full((B_TOP,), 0xF, dtype=torch.int32, device=gpu)
    got = plan.contact_dynamics_active(t("q"), t("qd"), t("tau"), bodies, offsets, full, a_des=t("a_des"))
    want = plan.contact_dynamics(t("q"), t("qd"), t("tau"), bodies, offsets, a_des=t("a_des"))
    for what, g, w in zip(("ydd", "lambda", "ydd_free"), got, want):
        _hold("cheetah_feet", f"{precision} full mask {what}", g, _np(w), tol)


def _step_args(cid, B, dtype, gpu):
    blob, bodies, offsets, mu, dt, x = inputs(cid, dtype is not None and "32" in str(dtype))
    plan = G.Plan(blob)  # (a plan of its own: the work pools of these tests are released and capped)
    return plan, bodies, offsets, mu, dt, {k: _dev(v, B, dtype, gpu) for k, v in x.items()}


def test_step_equals_its_three_calls_bit_for_bit(gpu):
    import torch

    for cid, dtype in (("cheetah_feet", torch.float64), ("tello_feet", torch.float32)):
        plan, bodies, offsets, mu, dt, t = _step_args(cid, B_TOP, dtype, gpu)
        kd = 1.0 / dt
        qn, vn, ydd, lam, imp, ok = plan.contact_step(t["q"], t["qd"], t["tau"], bodies, offsets, t["active"], dt, prev_active=t["prev"], kd=kd,
                                                      restitution=RESTITUTION, damping=mu)
        n = len(bodies)
        impact = torch.as_tensor(S.impact_masks(t["active"].cpu().numpy(), t["prev"].cpu().numpy(), n).astype(np.int32), device=gpu)
        v1, i1 = plan.contact_impulse_active(t["q"], t["qd"], bodies, offsets, impact, restitution=RESTITUTION, damping=mu)
        y1, l1, _ = plan.contact_dynamics_active(t["q"], v1, t["tau"], bodies, offsets, t["active"], kd=kd, damping=mu)
        q2, v2, ok2 = plan.integrate(t["q"], v1, y1, dt)
        for what, a, b in (("impulse", imp, i1), ("ydd", ydd, y1), ("lambda", lam, l1), ("q_next", qn, q2), ("qd_next", vn, v2), ("ok", ok, ok2)):
            assert torch.equal(a, b), (cid, what)
        # without a previous mask: no impulse, the dynamics at qd itself
        qn, vn, ydd, lam, imp, ok = plan.contact_step(t["q"], t["qd"], t["tau"], bodies, offsets, t["active"], dt, kd=kd, damping=mu)
        y1, l1, _ = plan.contact_dynamics_active(t["q"], t["qd"], t["tau"], bodies, offsets, t["active"], kd=kd, damping=mu)
        q2, v2, ok2 = plan.integrate(t["q"], t["qd"], y1, dt)
        assert imp is None and torch.equal(ydd, y1) and torch.equal(lam, l1) and torch.equal(qn, q2) and torch.equal(vn, v2)


@pytest.mark.parametrize("tau_per_step", [False, True], ids=["tau_held", "tau_per_step"])
@pytest.mark.parametrize("per_step", [False, True], ids=["held", "per_step"])
@pytest.mark.parametrize("with_impulses", [False, True], ids=["no_impulses", "impulses"])
def test_rollout_equals_its_steps_bit_for_bit(per_step, with_impulses, tau_per_step, gpu):
    import torch

    T = 3
    plan, bodies, offsets, mu, dt, t = _step_args("cheetah_feet", B_TOP, torch.float64, gpu)
    dt, kd, n = 1e-2, 100.0, len(bodies)
    # feet open and close along the sequence
    seq = torch.stack([t["active"], t["prev"], t["active"] ^ 0x5]) if per_step else t["active"]
    taus = torch.stack([t["tau"], 0.5 * t["tau"], -t["tau"]]) if tau_per_step else t["tau"].expand(T, -1, -1)  # (the steps' view of it)
    tau = taus if tau_per_step else t["tau"]
    first_prev = t["prev"]
    qT, vT, ok, qt, vt, lt = plan.contact_rollout(t["q"], t["qd"], tau, bodies, offsets, seq, dt, T, active_prev=first_prev, with_impulses=with_impulses,
                                                  kd=kd, restitution=RESTITUTION, damping=mu, record=True)
    q, qd, oks = t["q"], t["qd"], torch.ones(B_TOP, dtype=torch.bool, device=gpu)
    for s in range(T):
        act = seq[s] if per_step else seq
        prev = None if not with_impulses else first_prev if s == 0 else (seq[s - 1] if per_step else seq)
        q, qd, ydd, lam, imp, ok_s = plan.contact_step(q, qd, taus[s], bodies, offsets, act, dt, prev_active=prev, kd=kd, restitution=RESTITUTION,
                                                       damping=mu)
        oks &= ok_s
        assert torch.equal(qt[s], q) and torch.equal(vt[s], qd) and torch.equal(lt[s], lam), s
    assert torch.equal(qT, q) and torch.equal(vT, qd) and torch.equal(ok, oks)
    if with_impulses:  # a NULL active_prev stands for active[0]: nothing closes in step 0
        a0 = seq[0] if per_step else seq
        got = plan.contact_rollout(t["q"], t["qd"], tau, bodies, offsets, seq, dt, T, kd=kd, restitution=RESTITUTION, damping=mu)
        want = plan.contact_rollout(t["q"], t["qd"], tau, bodies, offsets, seq, dt, T, active_prev=a0, kd=kd, restitution=RESTITUTION, damping=mu)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_a_null_prev_active_enqueues_no_impulse_stage(gpu):
    import torch

    from graph_capture import capture

    plan, bodies, offsets, mu, dt, t = _step_args("cheetah_feet", 65, torch.float64, gpu)
    step = lambda prev: plan.contact_step(t["q"], t["qd"], t["tau"], bodies, offsets, t["active"], dt, prev_active=prev, damping=mu)
    without = capture(lambda: step(None))
    n0 = without.nodes["kernel"]
    without.drop()
    with_prev = capture(lambda: step(t["prev"]))
    n1 = with_prev.nodes["kernel"]
    with_prev.drop()
    print(f"contact_step kernel nodes: {n0} without prev_active, {n1} with it")
    # the impulse stage: the impact masks, the twists (two kernels on the walk route), the solve, two forward dynamics, the finish
    assert n1 >= n0 + 6


def test_three_chunks_equal_one_chunk(gpu, monkeypatch):
    import torch

    from test_chunk_seams_gpu import CAP_MB

    plan, bodies, offsets, mu, dt, t = _step_args("humanoid_soles", B_TOP, torch.float64, gpu)
    call = lambda: [_np(o) for o in plan.contact_step(t["q"], t["qd"], t["tau"], bodies, offsets, t["active"], dt, prev_active=t["prev"], kd=1.0 / dt,
                                                      restitution=RESTITUTION, damping=mu)]
    whole = call()
    torch.cuda.synchronize()
    held = plan.release_work()
    assert held > 3 * (CAP_MB << 20), "the batch does not fill three chunks of the cap: nothing is tested"
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", str(CAP_MB))
    chunked = call()
    torch.cuda.synchronize()
    assert plan.release_work() > 0
    for a, b in zip(chunked, whole):
        assert EP.same_bits_np(a, b), "the chunked call differs from the one-chunk call"


def test_graph_capture_replays_the_eager_bits(gpu):
    import torch

    from graph_capture import capture

    plan, bodies, offsets, mu, dt, t = _step_args("cheetah_feet", 65, torch.float32, gpu)
    T = 3
    call = lambda: plan.contact_rollout(t["q"], t["qd"], t["tau"], bodies, offsets, t["active"], dt, T, active_prev=t["prev"], kd=1.0 / dt,
                                        restitution=RESTITUTION, damping=mu, record=True)
    cap = capture(call)
    try:
        got = [_np(o) for o in cap.replay()]
        with torch.cuda.stream(cap.stream):
            want = [_np(o) for o in call()]
        cap.stream.synchronize()
        for a, b in zip(got, want):
            assert np.isfinite(a).all() and np.array_equal(a, b)
    finally:
        cap.drop()


def test_a_callers_stream_and_in_place_outputs(gpu):
    import torch

    plan, bodies, offsets, mu, dt, t = _step_args("cheetah_feet", B_TOP, torch.float64, gpu)
    kw = dict(prev_active=t["prev"], kd=1.0 / dt, restitution=RESTITUTION, damping=mu)
    want = plan.contact_step(t["q"], t["qd"], t["tau"], bodies, offsets, t["active"], dt, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = plan.contact_step(t["q"], t["qd"], t["tau"], bodies, offsets, t["active"], dt, stream=side, **kw)
    side.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    q, qd = t["q"].clone(), t["qd"].clone()
    got = plan.contact_step(q, qd, t["tau"], bodies, offsets, t["active"], dt, out=(q, qd), **kw)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == q.data_ptr() and got[1].data_ptr() == qd.data_ptr()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    v = t["qd"].clone()
    vn, imp = plan.contact_impulse_active(t["q"], v, bodies, offsets, t["active"], restitution=RESTITUTION, damping=mu, out=v)
    vw, iw = plan.contact_impulse_active(t["q"], t["qd"], bodies, offsets, t["active"], restitution=RESTITUTION, damping=mu)
    assert vn.data_ptr() == v.data_ptr() and torch.equal(vn, vw) and torch.equal(imp, iw)


def test_host_variant_equals_the_device_call(gpu):
    import torch

    blob, bodies, offsets, mu, dt, x = inputs("cheetah_feet")
    plan = EP.plan_for("urdf_mini_cheetah", ())
    B = 5
    t = lambda k: _dev(x[k], B, torch.float64, gpu)
    kw = dict(kd=1.0 / dt, restitution=RESTITUTION, damping=mu)
    want = plan.contact_step(t("q"), t("qd"), t("tau"), bodies, offsets, t("active"), dt, prev_active=t("prev"), **kw)
    got = plan.contact_step_host(x["q"][:B], x["qd"][:B], x["tau"][:B], bodies, offsets, x["active"][:B], dt, prev_active=x["prev"][:B], **kw)
    for a, b in zip(got[:5], want[:5]):
        assert np.array_equal(a, _np(b))
    assert np.array_equal(got[5], want[5].cpu().numpy())
