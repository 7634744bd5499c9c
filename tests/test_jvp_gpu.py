"""The Jacobian-vector products on the GPU (run with -m gpu on an MI355X): Plan.id_jvp / fd_jvp / integrate_jvp / step_jvp
(grbda_rnea_jvp_* / grbda_aba_jvp_* / grbda_integrate_jvp_* / grbda_step_jvp_*).

A tangent u is drawn per state from a seeded generator and scaled to unit 1-norm (jvp_ref.unit_tangent), so that the matrix bounds of the
project carry over unchanged: |sum_j (M - M_ref)_ij u_j| <= max |M - M_ref|.  Every error below is relative to 1 + max |reference MATRIX| of
the states compared, as test_vjp_gpu.py states its own.

id_jvp, fp64: each term alone against einsum("bij,bj->bi", ref, u) of id_derivative_refs.refs_of -- "q" 2e-5, "qd" 1e-8, "ydd" 1e-9 -- and
all three together at the sum of the three absolute bounds, on every batch size of id_derivative_refs.BATCHES and every model of
test_vjp_gpu.ID_MODELS (nv = 4: sixteen states per unit and partial packs; 18: three and idle lanes; 31 / 32: two per unit; 44 / 45, 64: one
per unit, 64 every lane a row; 65: two row blocks, the second with one live row and two column tiles, the second with one live column; the
four-bar and GRBDA_NO_ANALYTIC: difference routes).  fd_jvp, fp64: each term alone against the oracle's exact difference columns ("tau", "qd":
1e-8) and its central differences ("q": 2e-5, the first five states on the larger models); ydd has the bits of forward_dynamics.

The adjoint identity <g, jvp(u)> = <vjp(g), u> holds both products to one another on the device: 1e-9 on the analytic route (the same slab
matrices, another summation order), the "q" bound on difference routes.

fp32, explicit models: against the same entry point's fp64 result on the rounded inputs; id_jvp at 1e-3 of 1 + max |fp64 result|, fd_jvp at
max(1e-3, twice the error of (the fp32 matrices of fd_derivatives) u against that fp64 result), both printed: test_vjp_gpu.py's construction.

Chunk seams: a chunk of the work slab is never less than one tile of 64 states (the chunk rule every slab shares), so B = 70 cannot take
more than two passes whatever GRBDA_WORK_MAX_MB says; three passes are had from the 70 states taken twice, B = 140.

Every call that is compared with a reference goes through entry_points.run_guarded (NaN-canary arenas around inputs and outputs).

Measured on an MI355X (tree64_floating, B = 70 under a 1 MB slab): id_jvp "q" 1.6e-11, "qd" 9.4e-17, "ydd" 4.1e-16; fd_jvp "q" 1.3e-11,
"qd" and "tau" 5.0e-17; fp32 fd_jvp at most 4.6e-7 where the fp32 matrices times the tangent are at 1.4e-6; integrate_jvp fp64 at most
3.6e-17, fp32 at most 2.5e-8 against a float32 reference at 1.5e-8; step_jvp against the central difference at most 6.5e-10."""
import functools

import numpy as np
import pytest

import generalized_rbda_amd as G
import integrate_ref as R
import jvp_ref as J
import oracle_py as O
import step_vjp_ref as S
from entry_points import TOL32, _host, _states, edge_states, run_guarded, same_bits_np
from graph_capture import capture
from id_derivative_refs import BATCHES, B_MAX, MODELS, blob_of, is_explicit, oracle_refs, refs_of, states_of
from test_vjp_gpu import FD_BOUND, FD_MODELS, ID_BOUND, ID_MODELS, ID_REF, _dtype, _plan, fd_refs_of, unit_cotangent

pytestmark = pytest.mark.gpu
ID_NAMES, FD_NAMES = ("q", "qd", "ydd"), ("q", "qd", "tau")
TANGENT = {"q": "u_q", "qd": "u_qd", "ydd": "u_x", "tau": "u_x"}  # the tangent of a term among the inputs
ADJOINT_BOUND, LINEAR_BOUND = 1e-9, 1e-12


def _round(a, dt):
    return a if dt == "f64" else a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs_of(name, dt="f64"):
    """the model's B_MAX states with three tangents and a cotangent; shared, never written to (the forward side takes "ydd" as its tau)"""
    s = dict(states_of(name, dt))
    nv = s["qd"].shape[1]
    for k, key in enumerate(("u_q", "u_qd", "u_x")):
        s[key] = J.unit_tangent(B_MAX, nv, 10 * len(name) + k, dt)
    s["g"] = unit_cotangent(B_MAX, nv, len(name), dt)
    return s


def _jvp_call(forward, terms, with_ydd=False):
    """call(plan, x) for the tangents of `terms` (names of ID_NAMES / FD_NAMES), the others None"""
    names = FD_NAMES if forward else ID_NAMES

    def call(plan, x):
        t = [x[TANGENT[k]] if k in terms else None for k in names]
        if not forward:
            return (plan.id_jvp(x["q"], x["qd"], x["ydd"], *t),)
        got = plan.fd_jvp(x["q"], x["qd"], x["ydd"], *t, with_ydd=with_ydd)
        return got if with_ydd else (got,)

    return call


def run(forward, name, dt, B, gpu, terms, plan=None, with_ydd=False, s=None):
    s = {k: v[:B] for k, v in (s or inputs_of(name, dt)).items()}
    got = run_guarded(plan or _plan(name), _jvp_call(forward, terms, with_ydd), s, _dtype(dt), gpu, 0)
    return got if with_ydd else got[0]


def product(M, u):
    return np.einsum("bij,bj->bi", M, u)


def hold_id_f64(name, B, gpu, plan=None, what="", s=None, ref=None):
    s, ref = s or inputs_of(name), ref or refs_of(name)
    total, budget = 0.0, 0.0
    for k in ID_NAMES:
        M, u = ref[ID_REF[k]][:B], s[TANGENT[k]][:B]
        got = run(False, name, "f64", B, gpu, (k,), plan, s=s)
        assert got.shape == u.shape
        err = float(np.abs(got - product(M, u)).max() / (1.0 + np.abs(M).max()))
        print(f"{name} id_jvp f64 B={B}{what} {k}: {err:.2e}")
        assert err < ID_BOUND[k], (k, err)
        total = total + product(M, u)
        budget += ID_BOUND[k] * (1.0 + np.abs(M).max())
    got = run(False, name, "f64", B, gpu, ID_NAMES, plan, s=s)
    err = float(np.abs(got - total).max())
    print(f"{name} id_jvp f64 B={B}{what} all three: {err:.2e} absolute, bound {budget:.2e}")
    assert err < budget
    return got


def hold_fd_f64(name, B, gpu, plan=None, what=""):
    s, ref = inputs_of(name), fd_refs_of(name)
    for k in FD_NAMES:
        n = min(B, len(ref[k]))
        M, u = ref[k][:n], s[TANGENT[k]][:n]
        got = run(True, name, "f64", B, gpu, (k,), plan)
        assert got.shape == (B, u.shape[1])
        err = float(np.abs(got[:n] - product(M, u)).max() / (1.0 + np.abs(M).max()))
        print(f"{name} fd_jvp f64 B={B}{what} {k}: {err:.2e} ({n} states)")
        assert err < FD_BOUND[k], (k, err)


@pytest.mark.parametrize("name", ID_MODELS)
def test_id_jvp_matches_the_oracle_matrices_times_the_tangent_at_every_batch_size(name, gpu):
    for B in BATCHES:
        hold_id_f64(name, B, gpu)


@pytest.mark.parametrize("name", FD_MODELS)
def test_fd_jvp_matches_the_oracle_columns_times_the_tangent_at_every_batch_size(name, gpu):
    import torch

    plan, s = _plan(name), inputs_of(name)
    for B in BATCHES:
        hold_fd_f64(name, B, gpu)
        dydd, ydd = run(True, name, "f64", B, gpu, FD_NAMES, with_ydd=True)
        q, qd, tau = (torch.as_tensor(s[k][:B], dtype=torch.float64, device=gpu) for k in ("q", "qd", "ydd"))
        assert np.array_equal(ydd, plan.forward_dynamics(q, qd, tau).cpu().numpy()), "ydd has other bits than forward_dynamics"
        assert np.array_equal(dydd, run(True, name, "f64", B, gpu, FD_NAMES)), "with_ydd changes the bits of the product"


def _scale(name, forward, k):
    M = fd_refs_of(name)[k] if forward else refs_of(name)[ID_REF[k]]
    return 1.0 + float(np.abs(M).max())


@pytest.mark.parametrize("name,forward", [(n, False) for n in ID_MODELS] + [(n, True) for n in FD_MODELS],
                         ids=[f"id-{n}" for n in ID_MODELS] + [f"fd-{n}" for n in FD_MODELS])
def test_the_adjoint_identity_pairs_the_jvp_with_the_vjp(name, forward, gpu):
    """<g, jvp(u)> = <vjp(g), u>, term by term and state by state, relative to 1 + max |reference matrix of the term|"""
    import torch

    plan, B = _plan(name), 5
    s = inputs_of(name)
    x = {k: torch.as_tensor(v[:B], dtype=torch.float64, device=gpu) for k, v in s.items()}
    names = FD_NAMES if forward else ID_NAMES
    pulled = (plan.fd_vjp if forward else plan.id_vjp)(x["q"], x["qd"], x["ydd"], x["g"])
    for k in names:
        pushed = _jvp_call(forward, (k,))(plan, x)[0]
        lhs, rhs = (x["g"] * pushed).sum(dim=1), (pulled[k] * x[TANGENT[k]]).sum(dim=1)
        err = float((lhs - rhs).abs().max()) / _scale(name, forward, k)
        bound = ADJOINT_BOUND if MODELS[name][2] else ID_BOUND["q"]
        print(f"{name} {'fd' if forward else 'id'} {k}: <g, jvp(u)> - <vjp(g), u> = {err:.2e} (bound {bound:.0e})")
        assert err < bound, (k, err)


@pytest.mark.parametrize("forward", [False, True], ids=["id", "fd"])
@pytest.mark.parametrize("name", ["mini_cheetah", "tree65_fixed", "pair_rotor_chain_4"])
def test_the_three_single_tangent_calls_add_up_to_the_call_with_all_three(name, forward, gpu):
    B, names = 5, FD_NAMES if forward else ID_NAMES
    whole = run(forward, name, "f64", B, gpu, names)
    parts = sum(run(forward, name, "f64", B, gpu, (k,)) for k in names)
    err = float(np.abs(whole - parts).max() / (1.0 + np.abs(whole).max()))
    print(f"{name} {'fd' if forward else 'id'}: all three against the sum of the three: {err:.2e}")
    assert err < LINEAR_BOUND


@pytest.mark.parametrize("name", [n for n in ID_MODELS if is_explicit(blob_of(n))])
def test_id_jvp_fp32_follows_its_fp64_result(name, gpu):
    for B in BATCHES:
        got = run(False, name, "f32", B, gpu, ID_NAMES)
        want = run_guarded(_plan(name), _jvp_call(False, ID_NAMES), {k: v[:B] for k, v in inputs_of(name, "f32").items()}, _dtype("f64"), gpu, 0)[0]
        err = float(np.abs(got - want).max() / (1.0 + np.abs(want).max()))
        print(f"{name} id_jvp f32 B={B}: {err:.2e}")
        assert err < TOL32, err


@pytest.mark.parametrize("name", [n for n in FD_MODELS if is_explicit(blob_of(n))])
def test_fd_jvp_fp32_is_as_good_as_the_fp32_matrices_times_the_tangent(name, gpu):
    import torch

    plan = _plan(name)
    for B in BATCHES:
        s = {k: v[:B] for k, v in inputs_of(name, "f32").items()}
        q, qd, tau = (torch.as_tensor(s[k], dtype=torch.float32, device=gpu) for k in ("q", "qd", "ydd"))
        mats = {k: v.double().cpu().numpy() for k, v in plan.fd_derivatives(q, qd, tau).items()}
        for k, m in zip(FD_NAMES, ("dq", "dqd", "dtau")):
            got = run(True, name, "f32", B, gpu, (k,))
            want = run_guarded(plan, _jvp_call(True, (k,)), s, _dtype("f64"), gpu, 0)[0]
            scale = 1.0 + np.abs(want).max()
            by_matrices = float(np.abs(product(mats[m], s[TANGENT[k]]) - want).max() / scale)
            err = float(np.abs(got - want).max() / scale)
            print(f"{name} fd_jvp f32 B={B} {k}: {err:.2e}; fd_derivatives u: {by_matrices:.2e}")
            assert err < max(TOL32, 2 * by_matrices), (k, err, by_matrices)


def test_chunk_seams_inside_the_batch(gpu, monkeypatch):
    """tree64_floating under GRBDA_WORK_MAX_MB=1: the slab holds one tile of 64 states (2 x 64 x 64 + O(64) doubles each; a chunk is never
    less than a tile), so B = 70 goes through in passes of 64 and 6 states and the 70 states taken twice, B = 140, in three passes of 64,
    64 and 12 with seams inside both copies"""
    name = "tree64_floating"
    plan = G.Plan(blob_of(name))  # (a plan of its own: its slabs are measured)
    nn = plan.nv * plan.nv
    twice = {k: np.concatenate([v, v]) for k, v in inputs_of(name).items()}
    ref_twice = {k: np.concatenate([v, v]) for k, v in refs_of(name).items()}
    for B, s, ref in ((70, None, None), (140, twice, ref_twice)):
        monkeypatch.setenv("GRBDA_WORK_MAX_MB", "1")
        try:
            hold_id_f64(name, B, gpu, plan, " under a 1 MB slab", s, ref)
            if B == 70:
                hold_fd_f64(name, B, gpu, plan, " under a 1 MB slab")
        finally:
            monkeypatch.delenv("GRBDA_WORK_MAX_MB")
        held = plan.release_work()
        chunk = 64  # states: what 1 MB holds of 2 nn + O(nv) doubles is less than a tile, and a tile is the least
        assert (1 << 20) // ((2 * nn + 5 * plan.nv) * 8) < chunk
        passes = -(-B // chunk)
        print(f"B={B}: work slabs held {held} bytes, {passes} passes; the matrices of the whole batch would take {B * 2 * nn * 8}")
        assert passes == (2 if B == 70 else 3)
        assert chunk * 2 * nn * 8 <= held < (chunk + 1) * 2 * nn * 8 + chunk * 16 * plan.nv * 8  # one tile of states, not the batch


def test_the_contraction_kernel_past_one_trip_of_its_grid(gpu):
    """pair_rotor_chain_4 at the smallest batch for which a workgroup of the contraction kernel takes a second unit (the launch rule:
    G.jvp_contract_launch; at nv = 4 the fp32 launch has the fp64 grid): one call per precision, the fp64 one against the oracle's matrices
    on the first, the last and a handful of states, the fp32 one against the fp64 one on all"""
    import torch

    name = "pair_rotor_chain_4"
    plan, blob = _plan(name), blob_of(name)
    n_cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    cap = G.jvp_contract_launch(plan.nv, 1 << 40, n_cu)[1]  # the grid when there is no end of units
    B = cap * (64 // plan.nv) + 1
    assert G.jvp_contract_launch(plan.nv, B - 1, n_cu) == (cap, cap) and G.jvp_contract_launch(plan.nv, B, n_cu) == (cap + 1, cap)
    q, qd, ydd = _states(blob, B, 31)
    r32 = lambda a: _round(a, "f32")
    s = {"q": r32(q), "qd": r32(qd), "ydd": r32(ydd), "q_start": r32(q)}
    for k, key in enumerate(("u_q", "u_qd", "u_x")):
        s[key] = J.unit_tangent(B, plan.nv, 50 + k, "f32")
    got = run_guarded(plan, _jvp_call(False, ID_NAMES), s, _dtype("f64"), gpu, 0)[0]
    idx = np.unique(np.concatenate([edge_states(B), np.arange(0, B, B // 7)]))
    at = {k: v[idx] for k, v in s.items()}
    ref = oracle_refs(blob, at)
    want = sum(product(ref[ID_REF[k]], at[TANGENT[k]]) for k in ID_NAMES)
    budget = sum(ID_BOUND[k] * (1.0 + np.abs(ref[ID_REF[k]]).max()) for k in ID_NAMES)
    err = float(np.abs(got[idx] - want).max())
    print(f"B={B} ({cap + 1} units on {cap} workgroups) f64 on states {idx.tolist()}: {err:.2e} absolute, bound {budget:.2e}")
    assert err < budget
    got32 = run_guarded(plan, _jvp_call(False, ID_NAMES), s, _dtype("f32"), gpu, 0)[0]
    err32 = float(np.abs(got32 - got).max() / (1.0 + np.abs(got).max()))
    print(f"B={B} f32 against f64 on every state: {err32:.2e}")
    assert err32 < TOL32


# ---- integrate and step ---------------------------------------------------------------------------------------------------------------
ANGLES = (0.0, 1e-9, 1e-4, 1e-2, 3.0)  # |omega'| dt of the special rows
STEP_MODELS = ("pair_rotor_chain_4", "mini_cheetah")  # a fixed base (nq == nv) and a quaternion base
DT_INTEGRATE, DT_STEP, B_STEP = 0.25, 0.05, 5


@functools.lru_cache(maxsize=None)
def integrate_inputs(name, B, dt="f64"):
    """{"q_start", "qd_next", "u_q", "u_qd", "u_x"} of B states: stepped velocities with the special angles at the first states (as many
    as fit) and, from ten states on, mirrored at the last ones"""
    blob = blob_of(name)
    q, qd, ydd = _states(blob, B, 53)
    v = qd + DT_INTEGRATE * ydd
    base = S.layout(blob)[2]
    if base is not None:
        axes = np.random.default_rng(B).normal(size=(len(ANGLES), 3))
        axes /= np.linalg.norm(axes, axis=1, keepdims=True)
        rows = {b: b for b in range(min(B, len(ANGLES)))}
        if B >= 2 * len(ANGLES):
            rows.update({B - 1 - a: a for a in range(len(ANGLES))})
        for b, a in rows.items():
            v[b, base[1]:base[1] + 3] = axes[a] * (ANGLES[a] / DT_INTEGRATE)
    s = {"q_start": q.copy(), "qd_next": _round(v, dt)}
    for k, key in enumerate(("u_q", "u_qd", "u_x")):
        s[key] = J.unit_tangent(B, v.shape[1], 70 + k, dt)
    return s


def _integrate_call(keys=("u_q", "u_qd", "u_x")):
    return lambda plan, x: plan.integrate_jvp(x["qd_next"], DT_INTEGRATE, *[x[k] if k in keys else None for k in ("u_q", "u_qd", "u_x")])


def _rel(got, ref):
    return max(float(np.abs(a - b).max() / (1.0 + np.abs(b).max())) for a, b in zip(got, ref))


@pytest.mark.parametrize("name", STEP_MODELS)
def test_integrate_jvp_matches_the_closed_form(name, gpu):
    blob, plan = blob_of(name), _plan(name)
    for B in (1, 5, 70, 257):
        s = integrate_inputs(name, B)
        if S.layout(blob)[2] is not None and B >= 5:
            vi = S.layout(blob)[2][1]
            assert np.allclose(np.linalg.norm(s["qd_next"][:5, vi:vi + 3], axis=1) * DT_INTEGRATE, ANGLES, rtol=1e-12, atol=0)
        got = run_guarded(plan, _integrate_call(), s, _dtype("f64"), gpu, 0)
        err = _rel(got, J.integrate_jvp(blob, s["qd_next"], DT_INTEGRATE, s["u_q"], s["u_qd"], s["u_x"]))
        print(f"{name} integrate_jvp f64 B={B}: {err:.2e}")
        assert all(o.shape == (B, plan.nv) for o in got) and err < 1e-12
    for keys in (("u_q",), ("u_qd",), ("u_x",), ("u_q", "u_x")):  # a tangent that is None is a zero array
        got = run_guarded(plan, _integrate_call(keys), s, _dtype("f64"), gpu, 0)
        want = run_guarded(plan, _integrate_call(), {k: v if k in keys or not k.startswith("u_") else np.zeros_like(v) for k, v in s.items()},
                           _dtype("f64"), gpu, 0)
        assert same_bits_np(got, want), keys


@pytest.mark.parametrize("name", STEP_MODELS)
def test_integrate_jvp_fp32_is_as_good_as_the_float32_reference(name, gpu):
    """against the fp64 result of the same entry point on the rounded inputs; the bound is test_step_vjp_gpu.py's for the transposed
    kernel, max(1e-5, twice the error of the numpy reference run in float32 on the same inputs)"""
    blob, plan = blob_of(name), _plan(name)
    for B in (1, 5, 70, 257):
        s = integrate_inputs(name, B, "f32")
        got = run_guarded(plan, _integrate_call(), s, _dtype("f32"), gpu, 0)
        want = run_guarded(plan, _integrate_call(), s, _dtype("f64"), gpu, 0)
        ref32 = [a.astype(np.float64) for a in J.integrate_jvp(blob, s["qd_next"], DT_INTEGRATE, s["u_q"], s["u_qd"], s["u_x"], dtype=np.float32)]
        err, by_ref = _rel(got, want), _rel(ref32, want)
        print(f"{name} integrate_jvp f32 B={B}: {err:.2e}; the float32 reference: {by_ref:.2e}")
        assert err < max(1e-5, 2 * by_ref)


@functools.lru_cache(maxsize=None)
def step_inputs(name, B=B_STEP, dt="f64"):
    q, qd, tau = (_round(a, dt) for a in _states(blob_of(name), B, 41))
    s = {"q": q, "qd": qd, "tau": tau, "q_start": q}
    for k, key in enumerate(("u_q", "u_qd", "u_x")):
        s[key] = J.unit_tangent(B, qd.shape[1], 90 + k, dt)
    return s


def _step_call(plan, x):
    qd_next = plan.step(x["q"], x["qd"], x["tau"], DT_STEP)[1]
    return plan.step_jvp(x["q"], x["qd"], x["tau"], qd_next, DT_STEP, x["u_q"], x["u_qd"], x["u_x"])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", STEP_MODELS)
def test_step_jvp_has_the_bits_of_fd_jvp_followed_by_integrate_jvp(name, dt, gpu):
    import torch

    plan = _plan(name)
    for B in (1, 5, 70):
        s = step_inputs(name, B, dt)
        got = run_guarded(plan, _step_call, s, _dtype(dt), gpu, 0)
        x = {k: torch.as_tensor(v, dtype=_dtype(dt), device=gpu) for k, v in s.items()}
        qd_next = plan.step(x["q"], x["qd"], x["tau"], DT_STEP)[1]
        dydd = plan.fd_jvp(x["q"], x["qd"], x["tau"], x["u_q"], x["u_qd"], x["u_x"])
        want = plan.integrate_jvp(qd_next, DT_STEP, x["u_q"], x["u_qd"], dydd)
        assert same_bits_np(got, _host(want)), f"B={B}: step_jvp differs from fd_jvp + integrate_jvp"
        alone = plan.step_jvp(x["q"], x["qd"], x["tau"], qd_next, DT_STEP, dtau=x["u_x"])  # (no recursion: dtau alone)
        dydd = plan.fd_jvp(x["q"], x["qd"], x["tau"], dtau=x["u_x"])
        assert same_bits_np(_host(alone), _host(plan.integrate_jvp(qd_next, DT_STEP, dydd=dydd)))


@pytest.mark.parametrize("name", STEP_MODELS)
def test_step_jvp_matches_a_central_difference_of_the_reference_step(name, gpu):
    """fp64, B = 5, dt = 0.05: the step built from the oracle's forward dynamics and integrate_ref.reference_step, differenced (h = 1e-6)
    along the direction (u_q, u_qd, u_tau) through tangent_plus and read back with tangent_minus; 2e-5 of 1 + max |difference quotient|,
    the project's central-difference bound"""
    blob, plan, h = blob_of(name), _plan(name), 1e-6
    s = step_inputs(name)
    got = run_guarded(plan, _step_call, s, _dtype("f64"), gpu, 0)

    def stepped(q, qd, tau):
        return R.reference_step(blob, q, qd, O.forward_dynamics(blob, q, qd, tau), DT_STEP)[:2]

    q0, v0 = stepped(s["q"], s["qd"], s["tau"])
    side = [stepped(S.tangent_plus(blob, s["q"], e * s["u_q"]), s["qd"] + e * s["u_qd"], s["tau"] + e * s["u_x"]) for e in (+h, -h)]
    ref = [(S.tangent_minus(blob, side[0][0], q0) - S.tangent_minus(blob, side[1][0], q0)) / (2 * h), (side[0][1] - side[1][1]) / (2 * h)]
    for what, a, b in zip(("dq_next", "dqd_next"), got, ref):
        err = float(np.abs(a - b).max() / (1.0 + np.abs(b).max()))
        print(f"{name} step_jvp f64 {what}: {err:.2e} (max |reference| {np.abs(b).max():.3g})")
        assert err < 2e-5, (what, err)


@pytest.mark.parametrize("which", ["id_jvp", "fd_jvp", "step_jvp"])
def test_a_captured_call_replays_the_bits_of_the_eager_call(which, gpu):
    import torch

    name, B = "mini_cheetah", 5
    plan = _plan(name)
    s = step_inputs(name)
    x = {k: torch.as_tensor(v[:B], dtype=torch.float64, device=gpu) for k, v in s.items()}
    x["qd_next"] = plan.step(x["q"], x["qd"], x["tau"], DT_STEP)[1].clone()
    t = ("u_q", "u_qd", "u_x")
    if which == "id_jvp":
        call = lambda: (plan.id_jvp(x["q"], x["qd"], x["tau"], *[x[k] for k in t]),)
    elif which == "fd_jvp":
        call = lambda: plan.fd_jvp(x["q"], x["qd"], x["tau"], *[x[k] for k in t], with_ydd=True)
    else:
        call = lambda: plan.step_jvp(x["q"], x["qd"], x["tau"], x["qd_next"], DT_STEP, *[x[k] for k in t])
    cap = capture(call)
    try:
        assert cap.nodes["kernel"] >= 3
        for k in x:  # (new inputs in place: the states in reverse order)
            x[k].copy_(x[k].flip(0))
        got = _host(cap.replay())
        with torch.cuda.stream(cap.stream):
            want = _host(call())
        cap.stream.synchronize()
        assert same_bits_np(got, want) and all(np.isfinite(a).all() for a in got)
    finally:
        cap.drop()


def test_the_host_array_variants_give_the_bits_of_the_device_calls(gpu):
    import torch

    name, B = "mini_cheetah", 5
    plan = _plan(name)
    s = {k: np.ascontiguousarray(v[:B]) for k, v in step_inputs(name).items()}
    x = {k: torch.as_tensor(v, dtype=torch.float64, device=gpu) for k, v in s.items()}
    ptr = lambda a: a.ctypes.data
    dev = gpu.index or 0
    out = np.full((2, B, plan.nv), np.nan)
    args = [ptr(s[k]) for k in ("q", "qd", "tau", "u_q", "u_qd", "u_x")]
    assert G.lib().grbda_rnea_jvp_host_f64(plan._h, *args, 1e-6, ptr(out[0]), B, dev) == 0, G.lib().grbda_last_error()
    assert np.array_equal(out[0], plan.id_jvp(x["q"], x["qd"], x["tau"], x["u_q"], x["u_qd"], x["u_x"]).cpu().numpy())
    assert G.lib().grbda_aba_jvp_host_f64(plan._h, *args, 1e-6, ptr(out[0]), ptr(out[1]), B, dev) == 0, G.lib().grbda_last_error()
    assert same_bits_np(list(out), _host(plan.fd_jvp(x["q"], x["qd"], x["tau"], x["u_q"], x["u_qd"], x["u_x"], with_ydd=True)))
    qd_next = plan.step(x["q"], x["qd"], x["tau"], DT_STEP)[1]
    vn = np.ascontiguousarray(qd_next.cpu().numpy())
    rc = G.lib().grbda_step_jvp_host_f64(plan._h, ptr(s["q"]), ptr(s["qd"]), ptr(s["tau"]), ptr(vn), DT_STEP, ptr(s["u_q"]), ptr(s["u_qd"]), ptr(s["u_x"]),
                                         1e-6, ptr(out[0]), ptr(out[1]), B, dev)
    assert rc == 0, G.lib().grbda_last_error()
    assert same_bits_np(list(out), _host(plan.step_jvp(x["q"], x["qd"], x["tau"], qd_next, DT_STEP, x["u_q"], x["u_qd"], x["u_x"])))
