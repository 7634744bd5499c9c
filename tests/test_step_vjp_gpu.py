"""The vector-Jacobian products of integrate, step and rollout on the GPU (run with -m gpu on an MI355X): Plan.integrate_vjp / step_vjp /
rollout_vjp (grbda_integrate_vjp_* / grbda_step_vjp_* / grbda_rollout_vjp_*), tangent_cotangent and step_ad / rollout_ad.

The yardstick of integrate_vjp is the numpy closed form of tests/step_vjp_ref.py, which tests/test_step_vjp_ref_cpu.py holds to central
differences of the reference step.  step_vjp and rollout_vjp are DEFINED as compositions (include/grbda_hip_step_vjp.h), so they are held
to the bits of those compositions made from the Python methods, and to the oracle's forward-dynamics columns and to central differences
of Plan.rollout besides.  The cotangents (g_q, g_qd) of a state are drawn from a seeded generator and scaled to unit 1-norm together, as
test_vjp_gpu.unit_cotangent scales its own.  Every call compared with a reference goes through entry_points.run_guarded.

Measured on an MI355X: integrate_vjp fp64 at most 5.9e-17 of 1 + max |reference| (bound 1e-9); fp32 at most 1.9e-8 against a float32
reference at 6.9e-9 .. 2.3e-8 (bound max(1e-5, twice that)); step_vjp against the oracle "q" 5.8e-13, "qd" 3.1e-17, "tau" 1.7e-18 (bounds
2e-5, 1e-8, 1e-8); the directional check of the rollout 3.9e-11 (rev_rotor_chain_3) and 2.9e-10 (Mini Cheetah) against 2e-5."""
import functools
import itertools

import numpy as np
import pytest

import generalized_rbda_amd as G
import integrate_ref as R
import step_vjp_ref as S
from entry_points import TOL64, _dq_oracle, _fd_columns, _host, _states, run_guarded, same_bits_np
from graph_capture import capture
from id_derivative_refs import blob_of
from test_vjp_gpu import DQ_STATES, FD_BOUND

pytestmark = pytest.mark.gpu
ANGLES = (0.0, 1e-9, 1e-4, 1e-2, 3.0)  # |omega'| dt of the special rows
I_NAMES, S_NAMES = ("q", "qd", "ydd"), ("q", "qd", "tau")
STEP_MODELS = ("pair_rotor_chain_4", "mini_cheetah")  # a fixed base (nq == nv) and a quaternion base


def _dtype(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def _round(a, dt):
    return a if dt == "f64" else a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _plan(blob):
    return G.Plan(blob)


def cotangents(shape, seed, dt="f64"):
    """(g_q, g_qd) of `shape` [..., nv]: the 2 nv entries of a state of unit 1-norm together (then rounded to the type)"""
    g = np.random.default_rng([seed, 1789]).uniform(-1, 1, (2,) + tuple(shape))
    g /= np.abs(g).sum(axis=(0, -1), keepdims=True)
    return _round(g[0], dt), _round(g[1], dt)


@functools.lru_cache(maxsize=None)
def integrate_inputs(model, B, dt="f64"):
    """{"q_start", "qd_next", "g_q", "g_qd"} of B states: the stepped velocities of integrate_ref's states with the special angles at
    the first states (as many as fit) and, from ten states on, mirrored at the last ones -- B = 1 takes its angle from `B` itself"""
    blob = R.blob_of(model)
    q, qd, ydd = R.states_of(model, B)
    v = qd + R.dt_of(model) * ydd
    base = S.layout(blob)[2]
    if base is not None:
        axes = np.random.default_rng(B).normal(size=(len(ANGLES), 3))
        axes /= np.linalg.norm(axes, axis=1, keepdims=True)
        rows = {b: b for b in range(min(B, len(ANGLES)))}
        if B >= 2 * len(ANGLES):
            rows.update({B - 1 - a: a for a in range(len(ANGLES))})
        for b, a in rows.items():
            v[b, base[1]:base[1] + 3] = axes[a] * (ANGLES[a] / R.dt_of(model))
    g_q, g_qd = cotangents(v.shape, B, dt)
    return {"q_start": q.copy(), "qd_next": _round(v, dt), "g_q": g_q, "g_qd": g_qd}


def _integrate_call(dt_step, want=I_NAMES, g_q="g_q", g_qd="g_qd"):
    return lambda plan, x: tuple(plan.integrate_vjp(x["qd_next"], dt_step, x.get(g_q), x.get(g_qd), want=want).values())


def _rel(got, ref):
    return max(float(np.abs(a - b).max() / (1.0 + np.abs(b).max())) for a, b in zip(got, ref))


@pytest.mark.parametrize("model", R.EXPLICIT_MODELS)
def test_integrate_vjp_matches_the_closed_form_at_every_batch_size(model, gpu):
    blob, h = R.blob_of(model), R.dt_of(model)
    plan = _plan(blob)
    for B in R.BATCHES + (257,):
        s = integrate_inputs(model, B)
        got = run_guarded(plan, _integrate_call(h), s, _dtype("f64"), gpu, 0)
        err = _rel(got, S.integrate_vjp(blob, s["qd_next"], h, s["g_q"], s["g_qd"]))
        print(f"{model} integrate_vjp f64 B={B}: {err:.2e}")
        assert all(o.shape == (B, plan.nv) for o in got) and err < TOL64


def test_integrate_vjp_on_one_state_at_every_special_angle(gpu):
    blob, h = R.blob_of("urdf_mini_cheetah"), R.DT_EXPLICIT
    vi = S.layout(blob)[2][1]
    for a, angle in enumerate(ANGLES):
        s = {k: v[:1].copy() for k, v in integrate_inputs("urdf_mini_cheetah", 63).items()}
        s["qd_next"][0, vi:vi + 3] = np.array([0.6, -0.48, 0.64]) * (angle / h)
        got = run_guarded(_plan(blob), _integrate_call(h), s, _dtype("f64"), gpu, 0)
        err = _rel(got, S.integrate_vjp(blob, s["qd_next"], h, s["g_q"], s["g_qd"]))
        print(f"B=1, |omega'| dt = {angle}: {err:.2e}")
        assert err < TOL64


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("model", ["rev_rotor_chain_3", "urdf_mini_cheetah"])
def test_every_subset_of_want_and_a_null_cotangent(model, dt, gpu):
    blob, h, B = R.blob_of(model), R.dt_of(model), 65
    plan, s = _plan(blob), integrate_inputs(model, 65, dt)
    full = dict(zip(I_NAMES, run_guarded(plan, _integrate_call(h), s, _dtype(dt), gpu, 0)))
    for n in (1, 2):
        for want in itertools.combinations(I_NAMES, n):
            got = run_guarded(plan, _integrate_call(h, want), s, _dtype(dt), gpu, 0)
            assert len(got) == n and all(np.array_equal(o, full[k]) for o, k in zip(got, want)), want
    for null in ("g_q", "g_qd"):  # a NULL cotangent is a zero array
        zeroed = dict(s, **{null: np.zeros_like(s[null])})
        want = run_guarded(plan, _integrate_call(h), zeroed, _dtype(dt), gpu, 0)
        got = run_guarded(plan, _integrate_call(h, **{null: "none"}), s, _dtype(dt), gpu, 0)
        assert same_bits_np(got, want), null
    assert B == len(s["qd_next"])


@pytest.mark.parametrize("model", R.EXPLICIT_MODELS)
def test_integrate_vjp_fp32_is_as_good_as_the_float32_reference(model, gpu):
    """against the fp64 result of the same entry point on the rounded inputs; the bound is max(1e-5, twice the error of the numpy
    reference run in float32 on the same inputs): the yardstick is the reference, the factor covers the other operation order"""
    blob, h = R.blob_of(model), R.dt_of(model)
    plan = _plan(blob)
    for B in R.BATCHES + (257,):
        s = integrate_inputs(model, B, "f32")
        got = run_guarded(plan, _integrate_call(h), s, _dtype("f32"), gpu, 0)
        want = run_guarded(plan, _integrate_call(h), s, _dtype("f64"), gpu, 0)
        ref32 = [a.astype(np.float64) for a in S.integrate_vjp(blob, s["qd_next"], h, s["g_q"], s["g_qd"], dtype=np.float32)]
        err, by_ref = _rel(got, want), _rel(ref32, want)
        print(f"{model} integrate_vjp f32 B={B}: {err:.2e}; the float32 reference: {by_ref:.2e}")
        assert err < max(1e-5, 2 * by_ref)


# ---- step ---------------------------------------------------------------------------------------------------------------------------
H_STEP_DT = 0.05


@functools.lru_cache(maxsize=None)
def step_inputs(name, B, dt="f64"):
    """{"q", "qd", "tau", "g_q", "g_qd", "q_start"} of B random states, rounded to the type"""
    q, qd, tau = (_round(a, dt) for a in _states(blob_of(name), B, 41))
    g_q, g_qd = cotangents(qd.shape, 7 * B, dt)
    return {"q": q, "qd": qd, "tau": tau, "g_q": g_q, "g_qd": g_qd, "q_start": q}


def _with_step(plan, x, h=H_STEP_DT):
    """x with the library's own stepped velocities"""
    return dict(x, qd_next=plan.step(x["q"], x["qd"], x["tau"], h)[1])


def _step_call(want=S_NAMES, h=H_STEP_DT):
    def call(plan, x):
        x = _with_step(plan, x, h)
        return tuple(plan.step_vjp(x["q"], x["qd"], x["tau"], x["qd_next"], h, x["g_q"], x["g_qd"], want=want).values())

    return call


def _composed_step(plan, x, h=H_STEP_DT, want=S_NAMES):
    """the three stages from the Python methods and torch adds"""
    i = plan.integrate_vjp(x["qd_next"], h, x["g_q"], x["g_qd"], want=tuple(k for k in ("q", "qd") if k in want) + ("ydd",))
    a = plan.fd_vjp(x["q"], x["qd"], x["tau"], i["ydd"], want=want)
    return tuple(a[k] if k == "tau" else i[k] + a[k] for k in want)


def _bits(t):
    import torch

    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(got, want):
    import torch

    return len(got) == len(want) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", STEP_MODELS)
def test_step_vjp_has_the_bits_of_its_three_stages(name, dt, gpu):
    import torch

    plan = _plan(blob_of(name))
    for B in (1, 65, 130):
        s = step_inputs(name, B, dt)
        host = run_guarded(plan, _step_call(), s, _dtype(dt), gpu, 0)
        x = _with_step(plan, {k: torch.as_tensor(v, dtype=_dtype(dt), device=gpu) for k, v in s.items()})
        want = _composed_step(plan, x)
        assert same_bits_np(host, _host(want)), f"B={B}: step_vjp differs from integrate_vjp + fd_vjp + add"
        for sub in (("tau",), ("q",), ("qd", "tau")):
            got = plan.step_vjp(x["q"], x["qd"], x["tau"], x["qd_next"], H_STEP_DT, x["g_q"], x["g_qd"], want=sub)
            assert list(got) == list(sub) and _same(list(got.values()), [want[S_NAMES.index(k)] for k in sub]), (B, sub)


def test_step_vjp_matches_the_oracle_on_the_quaternion_base(gpu):
    """the numpy integrate VJP plus g_ydd^T of the oracle's forward-dynamics columns; test_vjp_gpu's bounds -- "q" 2e-5, "qd" and "tau"
    1e-8 -- relative to (1 + max |oracle matrix|) max(1, |g_ydd|_1)"""
    import torch

    name, B, h = "mini_cheetah", DQ_STATES, H_STEP_DT
    blob, plan = blob_of(name), _plan(blob_of(name))
    s = {k: v[:B] for k, v in step_inputs(name, 65).items()}
    got = dict(zip(S_NAMES, run_guarded(plan, _step_call(), s, _dtype("f64"), gpu, 0)))
    x = {k: torch.as_tensor(v, dtype=torch.float64, device=gpu) for k, v in s.items()}
    qd_next = plan.step(x["q"], x["qd"], x["tau"], h)[1].cpu().numpy()
    i_q, i_qd, g_ydd = S.integrate_vjp(blob, qd_next, h, s["g_q"], s["g_qd"])
    mats = {"tau": _fd_columns(blob, s["q"], s["qd"], s["tau"], "dtau"), "qd": _fd_columns(blob, s["q"], s["qd"], s["tau"], "dqd"),
            "q": _dq_oracle(blob, s["q"], s["qd"], s["tau"])}
    norm = max(1.0, float(np.abs(g_ydd).sum(axis=1).max()))
    for k, plus in (("q", i_q), ("qd", i_qd), ("tau", 0.0)):
        ref = plus + np.einsum("bi,bij->bj", g_ydd, mats[k])
        err = float(np.abs(got[k] - ref).max() / ((1.0 + np.abs(mats[k]).max()) * norm))
        print(f"step_vjp f64 {k}: {err:.2e} (|g_ydd|_1 at most {norm:.3g})")
        assert err < FD_BOUND[k], (k, err)


def test_the_host_variant_has_the_bits_of_the_device_call(gpu):
    import torch

    for name in STEP_MODELS:
        plan, B = _plan(blob_of(name)), 5
        s = {k: np.ascontiguousarray(v[:B]) for k, v in step_inputs(name, 65).items()}
        x = _with_step(plan, {k: torch.as_tensor(v, dtype=torch.float64, device=gpu) for k, v in s.items()})
        want = _host(plan.step_vjp(x["q"], x["qd"], x["tau"], x["qd_next"], H_STEP_DT, x["g_q"], x["g_qd"]).values())
        qd_next = np.ascontiguousarray(x["qd_next"].cpu().numpy())
        out = np.full((3, B, plan.nv), np.nan)
        ptr = lambda a: a.ctypes.data
        rc = G.lib().grbda_step_vjp_host_f64(plan._h, ptr(s["q"]), ptr(s["qd"]), ptr(s["tau"]), ptr(qd_next), H_STEP_DT, ptr(s["g_q"]), ptr(s["g_qd"]),
                                             1e-6, *[ptr(o) for o in out], B, gpu.index or 0)
        assert rc == 0, G.lib().grbda_last_error()
        assert same_bits_np(list(out), want), name


# ---- rollout ------------------------------------------------------------------------------------------------------------------------
def rollout_case(plan, name, B, T, tau_T, g_T, dt, gpu, h=H_STEP_DT):
    """device tensors of one rollout: states, torques ([T, B, nv] or [B, nv]), the recorded trajectory and cotangents ([T, B, nv] or
    [B, nv])"""
    import torch

    s = step_inputs(name, B, dt)
    x = {k: torch.as_tensor(s[k], dtype=_dtype(dt), device=gpu) for k in ("q", "qd", "tau")}
    if tau_T:
        scale = torch.as_tensor(np.linspace(1.0, 0.4, T), dtype=_dtype(dt), device=gpu)
        x["tau"] = x["tau"][None] * scale[:, None, None]
    x["q_traj"], x["qd_traj"] = plan.rollout(x["q"], x["qd"], x["tau"], h, T, record=True)[3:]
    g_q, g_qd = cotangents((T, B, plan.nv) if g_T else (B, plan.nv), 100 * T + B, dt)
    x["g_q"], x["g_qd"] = (torch.as_tensor(g, dtype=_dtype(dt), device=gpu) for g in (g_q, g_qd))
    return x


def python_loop(plan, x, h=H_STEP_DT, g_q="g_q", g_qd="g_qd"):
    """the loop of include/grbda_hip_step_vjp.h from Plan.step_vjp and torch adds (step_vjp_ref.rollout_vjp over device tensors)"""
    step = lambda q, qd, tau, qd_next, a, b: plan.step_vjp(q, qd, tau, qd_next, h, a, b)
    got = S.rollout_vjp(step, x["q"], x["qd"], x["q_traj"], x["qd_traj"], x["tau"], x.get(g_q), x.get(g_qd))
    import torch

    return got["q"], got["qd"], torch.stack(got["tau"]) if isinstance(got["tau"], list) else got["tau"]


def _rollout_call(plan, x, h=H_STEP_DT, **kw):
    return tuple(plan.rollout_vjp(x["q"], x["qd"], x["tau"], h, x["q_traj"], x["qd_traj"], x.get("g_q"), x.get("g_qd"), **kw).values())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("g_T", [False, True], ids=["g_last", "g_every"])
@pytest.mark.parametrize("tau_T", [False, True], ids=["tau_held", "tau_every"])
@pytest.mark.parametrize("name", STEP_MODELS)
def test_rollout_vjp_has_the_bits_of_the_loop_of_step_vjp(name, tau_T, g_T, dt, gpu):
    plan = _plan(blob_of(name))
    for B, T in ((70, 3), (1, 1)):
        x = rollout_case(plan, name, B, T, tau_T, g_T, dt, gpu)
        got, want = _rollout_call(plan, x), python_loop(plan, x)
        assert got[2].shape == x["tau"].shape and _same(got, want), (B, T)
        assert all(bool(t.isfinite().all()) for t in got)
    # every subset of want, and one cotangent alone, at the last case
    for sub in (("q",), ("tau",), ("qd", "tau")):
        part = _rollout_call(plan, x, want=sub)
        assert _same(part, [got[S_NAMES.index(k)] for k in sub]), sub
    alone = dict(x, g_q=None)
    assert _same(_rollout_call(plan, alone), python_loop(plan, alone))


def test_a_rollout_of_no_steps_writes_nothing(gpu):
    import torch

    plan, B = _plan(blob_of("mini_cheetah")), 3
    s = step_inputs("mini_cheetah", 65)
    x = {k: torch.as_tensor(s[k][:B], dtype=torch.float64, device=gpu) for k in ("q", "qd", "tau", "g_q", "g_qd")}
    out = torch.full((3, B, plan.nv), float("nan"), dtype=torch.float64, device=gpu)
    none = torch.empty((0, B, plan.nq), dtype=torch.float64, device=gpu)
    rc = G.lib().grbda_rollout_vjp_f64(plan._h, x["q"].data_ptr(), x["qd"].data_ptr(), none.data_ptr() or x["q"].data_ptr(), none.data_ptr() or x["qd"].data_ptr(),
                                       x["tau"].data_ptr(), 1, H_STEP_DT, 0, x["g_q"].data_ptr(), x["g_qd"].data_ptr(), 1, 1e-6, out[0].data_ptr(),
                                       out[1].data_ptr(), out[2].data_ptr(), B, gpu.index or 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool(out.isnan().all())


@pytest.mark.parametrize("name,model", [("rev_rotor_chain_3", "rev_rotor_chain_3"), ("mini_cheetah", "urdf_mini_cheetah")])
def test_the_gradient_of_a_rollout_along_a_direction(name, model, gpu):
    """fp64, T = 4, dt = 0.05, B = 5: <grad, u> for a unit tangent direction u in (q0, qd0, tau) against the central difference
    (h = 1e-6) of L = sum_k <g_k, tangent_minus(state_k(+-h u), state_k)> taken with Plan.rollout; 2e-5 (1 + |<grad, u>|), the
    project's central-difference bound.  tests/test_step_vjp_ref_cpu.py holds the closed form at dt = 0.25."""
    import torch

    blob, B, T, h, eps = R.blob_of(model), 5, 4, 0.05, 1e-6
    plan = _plan(blob)
    q, qd, tau = _states(blob, B, 23)
    g_q, g_qd = cotangents((T, B, plan.nv), 99)
    rng = np.random.default_rng(17)
    u = rng.uniform(-1, 1, (3, B, plan.nv))
    u /= np.sqrt((u * u).sum(axis=(0, 2), keepdims=True))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gpu)

    def trajectory(q, qd, tau):
        out = plan.rollout(t(q), t(qd), t(tau), h, T, record=True)
        return out[3], out[4]

    qt, vt = trajectory(q, qd, tau)
    s = {"q": q, "qd": qd, "tau": tau, "q_start": q, "q_traj": qt.cpu().numpy(), "qd_traj": vt.cpu().numpy(), "g_q": g_q, "g_qd": g_qd}
    grad = run_guarded(plan, lambda plan, x: _rollout_call(plan, x, h), s, torch.float64, gpu, 0)
    analytic = sum((a * b).sum(axis=1) for a, b in zip(grad, u))
    side = []
    for sign in (+eps, -eps):
        qs, vs = trajectory(S.tangent_plus(blob, q, sign * u[0]), qd + sign * u[1], tau + sign * u[2])
        qs, vs = qs.cpu().numpy(), vs.cpu().numpy()
        side.append(sum((g_q[k] * S.tangent_minus(blob, qs[k], s["q_traj"][k])).sum(axis=1) + (g_qd[k] * (vs[k] - s["qd_traj"][k])).sum(axis=1)
                        for k in range(T)))
    numeric = (side[0] - side[1]) / (2 * eps)
    err = np.abs(analytic - numeric) / (1.0 + np.abs(analytic))
    print(f"{name}: <grad, u> {analytic}, central difference {numeric}, relative {err.max():.2e}")
    assert err.max() < 2e-5


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("which", ["step_vjp", "rollout_vjp"])
def test_a_captured_call_replays_the_bits_of_the_eager_call(which, dt, gpu):
    import torch

    name, B, T = "mini_cheetah", 70, 3
    plan = _plan(blob_of(name))
    x = rollout_case(plan, name, B, T, True, True, dt, gpu)
    if which == "step_vjp":
        x = dict(x, tau=x["tau"][0].clone(), qd_next=x["qd_traj"][0].clone(), g_q=x["g_q"][0].clone(), g_qd=x["g_qd"][0].clone())
        call = lambda: tuple(plan.step_vjp(x["q"], x["qd"], x["tau"], x["qd_next"], H_STEP_DT, x["g_q"], x["g_qd"]).values())
    else:
        call = lambda: _rollout_call(plan, x)
    cap = capture(call)
    try:
        assert cap.nodes["kernel"] >= 3
        for k in x:  # (new inputs in place: the states in reverse order)
            x[k].copy_(x[k].flip(-2))
        got = _host(cap.replay())
        with torch.cuda.stream(cap.stream):
            want = _host(call())
        cap.stream.synchronize()
        assert same_bits_np(got, want) and all(np.isfinite(a).all() for a in got)
    finally:
        cap.drop()


@pytest.mark.parametrize("method", ["integrate_vjp", "step_vjp", "rollout_vjp"])
def test_the_tensor_arguments_follow_the_rules_of_the_binding(method, gpu):
    """what test_python_args_gpu.py holds every tensor method of Plan to, at B = 3: strided inputs and a side stream give the bits of the
    plain call; a CPU tensor is GrbdaError(-3), one float32 among float64 TypeError, a row short by one column ValueError"""
    import torch

    name, B, T = "pair_rotor_chain_4", 3, 2
    plan = _plan(blob_of(name))
    x = rollout_case(plan, name, B, T, True, True, "f64", gpu)
    if method == "rollout_vjp":
        keys = ("q", "qd", "tau", "q_traj", "qd_traj", "g_q", "g_qd")
        call = lambda a, stream=None: list(plan.rollout_vjp(a["q"], a["qd"], a["tau"], H_STEP_DT, a["q_traj"], a["qd_traj"], a["g_q"], a["g_qd"], stream=stream).values())
    else:
        x = dict(x, tau=x["tau"][0], qd_next=x["qd_traj"][0], g_q=x["g_q"][0], g_qd=x["g_qd"][0])
        if method == "step_vjp":
            keys = ("q", "qd", "tau", "qd_next", "g_q", "g_qd")
            call = lambda a, stream=None: list(plan.step_vjp(a["q"], a["qd"], a["tau"], a["qd_next"], H_STEP_DT, a["g_q"], a["g_qd"], stream=stream).values())
        else:
            keys = ("qd_next", "g_q", "g_qd")
            call = lambda a, stream=None: list(plan.integrate_vjp(a["qd_next"], H_STEP_DT, a["g_q"], a["g_qd"], stream=stream).values())
    plain = {k: x[k].contiguous() for k in keys}
    want = [t.clone() for t in call(plain)]

    def strided():
        big = {k: torch.full(v.shape[:-1] + (2 * v.shape[-1],), float("nan"), dtype=torch.float64, device=gpu) for k, v in plain.items()}
        for k, v in plain.items():
            big[k][..., ::2] = v
        views = {k: v[..., ::2] for k, v in big.items()}
        assert not any(v.is_contiguous() for v in views.values())
        return views

    assert _same(call(strided()), want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = call(strided(), side)
    side.synchronize()
    assert _same(got, want)
    for k in keys:
        with pytest.raises(G.GrbdaError) as e:
            call({**plain, k: plain[k].cpu()})
        assert e.value.code == -3
        with pytest.raises(TypeError):
            call({**plain, k: plain[k].float()})
        with pytest.raises(ValueError):
            call({**plain, k: plain[k][..., :-1]})


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def _leaves(x, grads):
    return [x[k].clone().requires_grad_(k in grads) for k in ("q", "qd", "tau")]


@pytest.mark.parametrize("rollout", [False, True], ids=["step_ad", "rollout_ad"])
@pytest.mark.parametrize("name", STEP_MODELS)
def test_autograd_gives_the_bits_of_the_vjp(name, rollout, gpu):
    import torch

    plan, B, T, h = _plan(blob_of(name)), 5, 3, H_STEP_DT
    x = rollout_case(plan, name, B, T, False, True, "f64", gpu)
    quaternion = plan.nq != plan.nv
    grads = ("qd", "tau") if quaternion else ("q", "qd", "tau")
    # weights of the outputs: an ambient cotangent of the positions, and g_qd
    w_q = torch.as_tensor(np.random.default_rng(3).uniform(-1, 1, (T, B, plan.nq)), dtype=torch.float64, device=gpu)
    w_qd = x["g_qd"]
    if not rollout:
        w_q, w_qd = w_q[0], w_qd[0]
    q, qd, tau = _leaves(x, grads)
    out = plan.rollout_ad(q, qd, tau, h, T) if rollout else plan.step_ad(q, qd, tau, h)
    plain = plan.rollout(x["q"], x["qd"], x["tau"], h, T, record=True)[3:] if rollout else plan.step(x["q"], x["qd"], x["tau"], h)[:2]
    assert _same([o.detach() for o in out], list(plain)), "the forward values have other bits"
    ((out[0] * w_q).sum() + (out[1] * w_qd).sum()).backward()
    g_q = plan.tangent_cotangent(plain[0], w_q)
    if rollout:
        want = plan.rollout_vjp(x["q"], x["qd"], x["tau"], h, plain[0], plain[1], g_q, w_qd, want=grads)
    else:
        want = plan.step_vjp(x["q"], x["qd"], x["tau"], plain[1], h, g_q, w_qd, want=grads)
    for leaf, k in zip((q, qd, tau), S_NAMES):
        if k in grads:
            assert leaf.grad is not None and torch.equal(_bits(leaf.grad), _bits(want[k])), k
        else:
            assert leaf.grad is None
    # only tau requires grad: the others get none
    q, qd, tau = _leaves(x, ("tau",))
    out = plan.rollout_ad(q, qd, tau, h, T) if rollout else plan.step_ad(q, qd, tau, h)
    ((out[0] * w_q).sum() + (out[1] * w_qd).sum()).backward()
    assert q.grad is None and qd.grad is None and torch.equal(_bits(tau.grad), _bits(want["tau"]))
    if quaternion:
        q, qd, tau = _leaves(x, ("q", "qd", "tau"))
        with pytest.raises(ValueError, match="rollout_vjp" if rollout else "step_vjp"):
            plan.rollout_ad(q, qd, tau, h, T) if rollout else plan.step_ad(q, qd, tau, h)
