"""Chunk seams of the pipelines that split a batch (capi.cpp): every chunked site of the single-device entry points runs a batch through
at least three chunks and a ragged tail.

Sites whose chunk comes from work_budget() (analytic derivatives on each of their routes, derivatives on the constraint manifold, the
spanning-tree dynamics, the spanning recovery of big clusters) are forced into chunks with GRBDA_WORK_MAX_MB, which is read per call.
Then, without restating any chunk formula:
  * chunking is proved by the captured call's kernel nodes: at least three times those of a 64-state batch;
  * the slab release_work() reports stays within the cap (or at the one-tile minimum: the slab of a 64-state batch);
  * the capped call equals the uncapped (one-chunk) call at the same batch bit for bit -- both launch the same per-lane kernels, so a
    seam off by one row or one group is a mismatch;
  * every state within 2 of a multiple of 64 (chunks are whole tiles: a superset of the seams), the tail and a seeded sample agree with
    the oracle at the tolerances of test_gpu_parity.py.
The slab check can only catch an overrun of the budget where the whole-batch ydd is a sizeable part of the cap: the *_ydd_per_chunk rows.
Sites with a fixed chunk (derived()'s difference batches, applyTestForce and the inverse OSIM on the unit-wrench route, the fp32 position
derivative through fp64 differences, fp32 spanning-tree forward dynamics through fp64) get a batch of three chunks of that documented size
and a ragged tail, the same node proof, the oracle at the seams, and -- where no one-chunk call of the whole batch exists -- bitwise
equality with separate calls on the batch's chunk-sized slices (the same launches, state for state)."""
import numpy as np
import pytest

import oracle_py as O
import generalized_rbda_amd as G
from generalized_rbda_amd.states import random_states
from graph_capture import capture
from entry_points import _dq_oracle, _fd_columns, _mass_oracle, _model, _rel, _states

pytestmark = pytest.mark.gpu
TOL64 = 1e-9
TOL32 = 1e-3
CAP_MB = 1


def _near_seams(B, step, seed):
    idx = {i for s in range(step, B, step) for i in range(s - 2, s + 3) if 0 <= i < B}
    idx |= set(range(max(0, B - 3), B))
    idx |= set(np.random.default_rng(seed).choice(B, min(B, 64), replace=False).tolist())
    return np.array(sorted(idx))


def _derivs(plan, x):
    d = plan.fd_derivatives(x["q"], x["qd"], x["tau"])
    return d["dq"], d["dqd"], d["dtau"]


def _chk_derivs(blob, s, o, tol, big=False):
    assert _rel(o[2], _fd_columns(blob, s["q"], s["qd"], s["tau"], "dtau")) < max(tol, 1e-8)
    assert _rel(o[1], _fd_columns(blob, s["q"], s["qd"], s["tau"], "dqd")) < max(tol, 1e-8)
    # (d / dq: central differences along the tangent step, a few states at the first seams and the last ones at the tail)
    k = np.unique(np.r_[np.arange(min(4, len(s["q"]))), np.arange(max(0, len(s["q"]) - 4), len(s["q"]))])
    assert _rel(o[0][k], _dq_oracle(blob, s["q"][k], s["qd"][k], s["tau"][k])) < max(tol, 2e-5)


def _chk_aba(blob, s, o, tol, big=False):
    assert _rel(o[0], O.forward_dynamics(blob, s["q"], s["qd"], s["tau"], big=big)) < tol


def _chk_spanning(blob, s, o, tol, big=False):
    assert _rel(o[0], O.spanning_state(blob, s["q"], s["qd"], big=big)[1]) < max(tol, 1e-10)


CALLS = {
    "fd_derivatives": (_derivs, _chk_derivs),
    "aba": (lambda p, x: (p.forward_dynamics(x["q"], x["qd"], x["tau"]),), _chk_aba),
    "spanning": (lambda p, x: p.spanning(x["q"], x["qd"], x["tau"]), _chk_spanning),
}

# (id, model, plan-time switches, dtype, B, entry point): B mod 64 != 0 and B mod 4 in {1, 2, 3} (the interleaved groups of kDerivGroup = 4)
BUDGET_SITES = [
    ("analytic_minv_f32", "urdf_mini_cheetah", {}, "f32", 1001, "fd_derivatives"),
    ("analytic_minv_f64", "urdf_mini_cheetah", {}, "f64", 1001, "fd_derivatives"),
    ("analytic_dense_f64", "urdf_mini_cheetah", {"GRBDA_NO_MINV": "1"}, "f64", 1001, "fd_derivatives"),
    ("analytic_dense_f32", "urdf_mini_cheetah", {"GRBDA_NO_MINV": "1"}, "f32", 1002, "fd_derivatives"),
    ("analytic_solve_f64", "urdf_mini_cheetah", {"GRBDA_SOLVE_F64": "1"}, "f32", 1003, "fd_derivatives"),
    # B nv scalars of ydd exceed the cap less one tile: the forward dynamics run per chunk (no whole-batch ydd), and the slab check holds
    # the budget arithmetic to the cap (the whole-batch ydd used to be added on top of a chunk sized for the full budget)
    ("analytic_ydd_per_chunk_f32", "urdf_mini_cheetah", {}, "f32", 20001, "fd_derivatives"),
    ("analytic_ydd_per_chunk_f64", "urdf_mini_cheetah", {}, "f64", 20002, "fd_derivatives"),
    ("manifold_tello", "tello", {}, "f64", 1001, "fd_derivatives"),
    ("manifold_four_bar", "urdf_four_bar", {}, "f64", 50001, "fd_derivatives"),
    ("projection_two_parent", "two_parent", {}, "f64", 20001, "aba"),
    ("projection_big_cluster", "parallel_chain_exp_d10_l16", {}, "f64", 1001, "aba"),
    ("spanning_big_cluster", "parallel_chain_exp_d10_l16", {}, "f64", 60001, "spanning"),
]


def _inputs(blob, B, seed, dtype, gpu, big=False):
    import torch

    if big:
        from models import valid_states

        q, qd, tau = valid_states(blob, B, config_index=seed, big=True, scale=0.5, max_cond=50)
    else:
        q, qd, tau = _states(blob, B, seed)
    c = lambda a: np.asarray(torch.as_tensor(a, dtype=dtype).double())
    s = {"q": c(q), "qd": c(qd), "tau": c(tau)}
    return s, {k: torch.as_tensor(np.ascontiguousarray(v), dtype=dtype, device=gpu) for k, v in s.items()}


def _host(outs):
    return [o.detach().cpu().double().numpy() for o in outs]


@pytest.mark.parametrize("site,model,env,dtype_name,B,entry", BUDGET_SITES, ids=[s[0] for s in BUDGET_SITES])
def test_work_budget_chunk_seams(site, model, env, dtype_name, B, entry, gpu, monkeypatch):
    import torch

    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob = _model(model)
    big = model.startswith("parallel_chain")
    plan = G.Plan(blob)
    call, check = CALLS[entry]
    s, x = _inputs(blob, B, 5, dtype, gpu, big)
    _, x64 = _inputs(blob, 64, 6, dtype, gpu, big)
    # uncapped: one chunk
    whole = _host(call(plan, x))
    torch.cuda.synchronize()
    plan.release_work()
    # the one-tile slab (64 states, uncapped)
    call(plan, x64)
    torch.cuda.synchronize()
    one_tile = plan.release_work()
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", str(CAP_MB))
    chunked = _host(call(plan, x))
    torch.cuda.synchronize()
    held = plan.release_work()
    assert 0 < held <= max((CAP_MB << 20) + 256, one_tile), f"slab of {held} B against a cap of {CAP_MB} MiB"
    for a, b in zip(chunked, whole):
        assert np.array_equal(a, b), "the chunked call differs from the one-chunk call"
    # at least three chunks: kernel nodes of the captured call against a 64-state batch (both under the cap)
    cap_B = capture(lambda: call(plan, x))
    n_B = cap_B.nodes["kernel"]
    cap_B.drop()
    cap_64 = capture(lambda: call(plan, x64))
    n_64 = cap_64.nodes["kernel"]
    cap_64.drop()
    assert n_B >= 3 * n_64, f"{n_B} kernel nodes at B = {B}, {n_64} at 64: fewer than three chunks"
    plan.release_work()
    idx = _near_seams(B, 64, 7)
    check(blob, {k: v[idx] for k, v in s.items()}, [a[idx] for a in chunked], TOL64 if dtype == torch.float64 else TOL32, big=big)


# derived(): the difference batches of the mass matrix (nv + 1 inverse dynamics per state) and of the bias force (one), GRBDA_NO_CRBA=1;
# chunks of 256 MiB of expanded rows (q, qd, x, result per row)
@pytest.mark.parametrize("mode", ["mass_matrix", "bias"])
def test_difference_batch_chunk_seams(mode, gpu, monkeypatch):
    import torch

    monkeypatch.setenv("GRBDA_NO_CRBA", "1")
    blob = _model("urdf_mini_cheetah")
    plan = G.Plan(blob)
    nq, nv = plan.nq, plan.nv
    R = nv + 1 if mode == "mass_matrix" else 1
    chunk = (256 << 20) // ((nq + 3 * nv) * 8 * R)
    B = 3 * chunk + 45
    B += B % 4 == 0  # (a ragged tail: B mod 4 in {1, 2, 3}, B mod 64 != 0)
    assert B % 4 in (1, 2, 3) and B % 64
    q, qd, _ = random_states(blob, B, config_index=8)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gpu)
    tq, tqd = t(q), t(qd)
    call = (lambda b: (plan.mass_matrix(tq[:b]),)) if mode == "mass_matrix" else (lambda b: (plan.bias_force(tq[:b], tqd[:b]),))
    cap_B = capture(lambda: call(B))
    n_B = cap_B.nodes["kernel"]
    got = _host(cap_B.replay())[0]
    cap_B.drop()
    cap_64 = capture(lambda: call(64))
    n_64 = cap_64.nodes["kernel"]
    cap_64.drop()
    assert n_B >= 3 * n_64, f"{n_B} kernel nodes at B = {B}, {n_64} at 64"
    eager = _host(call(B))[0]
    torch.cuda.synchronize()
    assert np.array_equal(got, eager)
    idx = _near_seams(B, chunk, 9)
    if mode == "mass_matrix":
        assert _rel(got[idx], _mass_oracle(blob, q[idx])) < TOL64
    else:
        ref = O.inverse_dynamics(blob, q[idx], qd[idx], np.zeros_like(qd[idx]))
        assert _rel(got[idx], ref) < TOL64


# ---- fixed chunk sizes: (id, model, switches, dtype, entry, scalars per state of the documented chunk, chunk bytes, scalar size) ---------
FORCE_BODY, OFFSET = "FL_knee_link", (0.05, -0.02, 0.1)  # (a link: a frame on a rotor is fine too on these routes)


def _fixed_call(entry, plan):
    from test_gpu_parity import _body_index

    b = _body_index(plan.blob, FORCE_BODY) if entry in ("apply_test_force", "inv_osim") else None
    if entry == "apply_test_force":
        return lambda x: plan.apply_test_force(x["q"], b, OFFSET, x["force"])
    if entry == "inv_osim":
        return lambda x: plan.inv_osim(x["q"], [b], [OFFSET], with_jacobian=True)
    if entry == "fd_dq":
        return lambda x: (plan.fd_dq(x["q"], x["qd"], x["tau"]),)
    return lambda x: (plan.forward_dynamics(x["q"], x["qd"], x["tau"]),)


def _fixed_per_state(entry, plan):
    nq, nv, nb = plan.nq, plan.nv, plan.n_bodies
    return {"apply_test_force": (nb * 18 + 5 * nv, 256 << 20, 8),  # poses, wrenches, zeros, four results (fp64)
            "inv_osim": (nb * 12 + 7 * (nq + nb * 6 + 3 * nv), 256 << 20, 8),  # one frame: 7 rows of q, wrenches, zeros, results
            "fd_dq": (nq + 2 * nv + nv * nv, 64 << 20, 8),  # fp64 copies of q, qd, tau and the matrix
            "aba": (nq + 3 * nv, 256 << 20, 8)}[entry]  # fp64 copies of q, qd, tau and ydd


def _fixed_check(entry, blob, s, o, big):
    from entry_points import _chk_osim

    tol32 = lambda a: max(a, TOL32) if s["dtype"] == "f32" else a
    if entry == "apply_test_force":
        from test_gpu_parity import _body_index

        nb, B, body = s["nb"], len(s["q"]), _body_index(blob, FORCE_BODY)
        lam, ds = o
        Xa = O.body_poses(blob, s["q"], nb)[:, body]
        E, r = Xa[:, :9].reshape(B, 3, 3), Xa[:, 9:]
        fe = np.zeros((B, nb, 6))
        fe[:, body, :3] = np.cross(r + np.einsum("bji,j->bi", E, OFFSET), s["force"])
        fe[:, body, 3:] = s["force"]
        z = np.zeros_like(s["qd"])
        ds_ref = O.forward_dynamics(blob, s["q"], z, z, fe) - O.forward_dynamics(blob, s["q"], z, z)
        jtf = O.inverse_dynamics(blob, s["q"], z, z) - O.inverse_dynamics(blob, s["q"], z, z, fe)
        assert _rel(ds, ds_ref) < 1e-8
        assert np.abs(lam.reshape(-1) - np.einsum("bi,bi->b", jtf, ds_ref)).max() / (1 + np.abs(lam).max()) < 1e-8
    elif entry == "inv_osim":
        from test_gpu_parity import _body_index

        _chk_osim(blob, s, o, TOL64, frames=([_body_index(blob, FORCE_BODY)], [OFFSET]))  # (the one frame of _fixed_call)
    elif entry == "fd_dq":
        # (fp32 in and out, the differences in fp64: the tolerance of the fp64 differences and fp32 rounding of the result)
        assert _rel(o[0], _dq_oracle(blob, s["q"], s["qd"], s["tau"])) < 2e-5
    else:
        assert _rel(o[0], O.forward_dynamics(blob, s["q"], s["qd"], s["tau"], big=big)) < tol32(TOL64)


FIXED_SITES = [
    ("apply_test_force_unit_wrench", "urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, "f64", "apply_test_force"),
    ("inv_osim_unit_wrench", "urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, "f64", "inv_osim"),
    ("fd_dq_f32_differences", "urdf_mini_cheetah", {"GRBDA_NO_ANALYTIC": "1"}, "f32", "fd_dq"),
    ("aba_f32_through_f64_big_cluster", "parallel_chain_exp_d10_l16", {}, "f32", "aba"),
]


@pytest.mark.parametrize("site,model,env,dtype_name,entry", FIXED_SITES, ids=[s[0] for s in FIXED_SITES])
def test_fixed_chunk_seams(site, model, env, dtype_name, entry, gpu, monkeypatch):
    import torch

    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob = _model(model)
    big = model.startswith("parallel_chain")
    plan = G.Plan(blob)
    per_state, chunk_bytes, size = _fixed_per_state(entry, plan)
    chunk = chunk_bytes // (per_state * size)
    B = 3 * chunk + 45
    B += B % 4 == 0
    assert B % 4 in (1, 2, 3) and B % 64 and B > 3 * chunk
    # (2 048 seeded states, tiled: every index still has its own state for the oracle)
    s0, _ = _inputs(blob, 2048, 11, dtype, gpu, big)
    rep = lambda a: np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:]))
    s = {k: rep(v) for k, v in s0.items()}
    s["force"] = np.asarray(torch.as_tensor(np.random.default_rng(12).uniform(-1, 1, (B, 3)), dtype=dtype).double())
    x = {k: torch.as_tensor(v, dtype=dtype, device=gpu) for k, v in s.items()}
    call = _fixed_call(entry, plan)
    sl = lambda a, b: {k: v[a:b].contiguous() for k, v in x.items()}
    cap_B = capture(lambda: call(x))
    n_B = cap_B.nodes["kernel"]
    got = _host(cap_B.replay())
    cap_B.drop()
    cap_64 = capture(lambda: call(sl(0, 64)))
    n_64 = cap_64.nodes["kernel"]
    cap_64.drop()
    assert n_B >= 3 * n_64, f"{n_B} kernel nodes at B = {B}, {n_64} at 64: fewer than three chunks"
    # each chunk-sized slice through its own call: one chunk each, the same launches as that chunk of the whole batch
    for b0 in range(0, B, chunk):
        part = _host(call(sl(b0, min(B, b0 + chunk))))
        torch.cuda.synchronize()
        for a, p in zip(got, part):
            assert np.array_equal(a[b0:b0 + len(p)], p), f"chunk at {b0} differs from its own call"
    idx = _near_seams(B, chunk, 13)
    if entry == "fd_dq":  # (central differences of the oracle per state and column: the seams, the tail and a few more)
        idx = np.unique(np.r_[idx[np.isin(idx, [c * chunk + d for c in (1, 2, 3) for d in range(-2, 3)])], np.arange(B - 3, B), idx[:6]])
    sub = {k: v[idx] for k, v in s.items()}
    sub["nb"], sub["dtype"] = plan.n_bodies, dtype_name
    _fixed_check(entry, blob, sub, [a[idx] for a in got], big)
