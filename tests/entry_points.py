"""The table of device entry points the GPU tests share: ENTRY (name -> (call, oracle checker)), CASES (route x model x plan-time switches
x batch x entry point), and what makes their models, states and inputs.  A plain module, not a test file: test_graph_capture_gpu.py,
test_buffer_edges_gpu.py and test_batch_ladder_gpu.py all go through it, so an entry point added to the library is covered by every one
of them with one more row here.

call(plan, x) returns a tuple of output tensors, x holding the device tensors "q", "qd", "tau", "fext", "force", "q_start", "q_proj";
check(blob, s, outs, tol) compares the numpy outputs `outs` of the states `s` (a dict of numpy inputs) with the oracle."""
import functools
import os

import numpy as np

import kinematics_ref as K
import oracle_py as O
import generalized_rbda_amd as G
from generalized_rbda_amd.states import parse_clusters, random_states
from models import ROBOT_MODELS, valid_states, zoo

TOL64 = 1e-9
TOL32 = 1e-3
B_CHAIN = 65536 + 37  # beyond four tiles per SIMD of 256 CUs: the chain kernels, not latency mode


_BIG = set()  # blobs of plans with clusters beyond the structured limits: the oracle built with room for them (big=True)


def _big(blob):
    return blob in _BIG


_zoo = functools.lru_cache(maxsize=None)(zoo)  # (the descriptions are immutable bytes: built once per process)


@functools.lru_cache(maxsize=None)
def _model(name):
    if name == "two_parent":
        from test_capi_cpu import two_parent_model

        return two_parent_model().serialize()
    if name.startswith("parallel_chain"):
        blob = G.urdf_to_blob(os.path.join(ROBOT_MODELS, name + ".urdf"))
        _BIG.add(blob)
        return blob
    return _zoo()[name]


def _states(blob, B, seed, max_cond=None):
    if _big(blob):
        return valid_states(blob, B, config_index=seed, big=True, scale=0.5, max_cond=50)
    if any(c[9] in (2, 3) for c in parse_clusters(blob)["clusters"]):  # implicit loops: states on the constraint manifold
        return valid_states(blob, B, config_index=seed, max_cond=max_cond)
    return random_states(blob, B, config_index=seed)


def _rel(a, b):
    return float(np.abs(a - b).max() / (1.0 + np.abs(b).max()))


def _fd_columns(blob, q, qd, tau, wrt):
    """d ydd / d tau (exact: linear) and d ydd / d qd (exact central difference: quadratic) of the oracle's forward dynamics"""
    B, nv = qd.shape
    out = np.empty((B, nv, nv))
    for k in range(nv):
        e = np.zeros((B, nv))
        e[:, k] = 1.0
        if wrt == "dtau":
            out[:, :, k] = O.forward_dynamics(blob, q, qd, tau + e) - O.forward_dynamics(blob, q, qd, tau)
        else:
            out[:, :, k] = (O.forward_dynamics(blob, q, qd + e, tau) - O.forward_dynamics(blob, q, qd - e, tau)) / 2
    return out


def _mass_oracle(blob, q):
    B, nv = q.shape[0], parse_clusters(blob)["nv"]
    z = np.zeros((B, nv))
    C = O.inverse_dynamics(blob, q, z, z, big=_big(blob))
    H = np.empty((B, nv, nv))
    for k in range(nv):
        e = np.zeros((B, nv))
        e[:, k] = 1.0
        H[:, :, k] = O.inverse_dynamics(blob, q, z, e, big=_big(blob)) - C
    return H


def _dq_oracle(blob, q, qd, tau):
    from test_gpu_parity import _reference_plus_on_manifold

    m = parse_clusters(blob)
    B, nv, h = q.shape[0], qd.shape[1], 1e-6
    out = np.empty((B, nv, nv))
    for b in range(B):
        for k in range(nv):
            qp = _reference_plus_on_manifold(blob, m, q[b], k, +h)[None]
            qm = _reference_plus_on_manifold(blob, m, q[b], k, -h)[None]
            out[b, :, k] = (O.forward_dynamics(blob, qp, qd[b:b + 1], tau[b:b + 1])[0] - O.forward_dynamics(blob, qm, qd[b:b + 1], tau[b:b + 1])[0]) / (2 * h)
    return out


# ---- the cases: (id, model, plan-time switches, B, entry point) -------------------------------------------------------------------
# Entry point: call(plan, x) -> tuple of output tensors, where x holds device tensors "q", "qd", "tau", "fext", "force";
# check(blob, s, outs, tol) compares the numpy outputs `outs` of the states `s` (a dict of numpy inputs) with the oracle.
def _aba(plan, x):
    return (plan.forward_dynamics(x["q"], x["qd"], x["tau"]),)


def _aba_fext(plan, x):
    return (plan.forward_dynamics(x["q"], x["qd"], x["tau"], f_ext=x["fext"]),)


def _rnea(plan, x):
    return (plan.inverse_dynamics(x["q"], x["qd"], x["tau"]),)


def _rnea_fext(plan, x):
    return (plan.inverse_dynamics(x["q"], x["qd"], x["tau"], f_ext=x["fext"]),)


def _chk_aba(blob, s, o, tol, fext=False):
    assert _rel(o[0], O.forward_dynamics(blob, s["q"], s["qd"], s["tau"], s["fext"] if fext else None, big=_big(blob))) < tol


def _chk_rnea(blob, s, o, tol, fext=False):
    assert _rel(o[0], O.inverse_dynamics(blob, s["q"], s["qd"], s["tau"], s["fext"] if fext else None, big=_big(blob))) < tol


def _chk_bias(blob, s, o, tol):
    assert _rel(o[0], O.inverse_dynamics(blob, s["q"], s["qd"], np.zeros_like(s["qd"]))) < tol


def _chk_mass(blob, s, o, tol):
    assert _rel(o[0], _mass_oracle(blob, s["q"])) < tol


def _chk_dtau(blob, s, o, tol):
    assert _rel(o[0], _fd_columns(blob, s["q"], s["qd"], s["tau"], "dtau")) < max(tol, 1e-8)


def _chk_dqd(blob, s, o, tol):
    assert _rel(o[0], _fd_columns(blob, s["q"], s["qd"], s["tau"], "dqd")) < max(tol, 1e-8)


def _chk_dq(blob, s, o, tol):
    assert _rel(o[0], _dq_oracle(blob, s["q"], s["qd"], s["tau"])) < max(tol, 2e-5)


def _chk_derivs(blob, s, o, tol):
    _chk_dq(blob, s, o[0:1], tol)
    _chk_dqd(blob, s, o[1:2], tol)
    _chk_dtau(blob, s, o[2:3], tol)


def _chk_poses(blob, s, o, tol):
    nb = o[0].shape[1]
    assert _rel(o[0].reshape(len(s["q"]), -1), O.body_poses(blob, s["q"], nb).reshape(len(s["q"]), -1)) < tol


def _chk_force(blob, s, o, tol):
    # applyTestForce at OFFSET on FORCE_BODY: dstate = FD with the force applied - FD without (zero velocity and torque)
    nb, B, body = s["fext"].shape[1], len(s["q"]), _body_index(blob, FORCE_BODY)
    lam, ds = o
    Xa = O.body_poses(blob, s["q"], nb)[:, body]
    E, r = Xa[:, :9].reshape(B, 3, 3), Xa[:, 9:]
    fe = np.zeros((B, nb, 6))
    fe[:, body, :3] = np.cross(r + np.einsum("bji,j->bi", E, OFFSET), s["force"])
    fe[:, body, 3:] = s["force"]
    z = np.zeros_like(s["qd"])
    ds_ref = O.forward_dynamics(blob, s["q"], z, z, fe) - O.forward_dynamics(blob, s["q"], z, z)
    jtf = O.inverse_dynamics(blob, s["q"], z, z) - O.inverse_dynamics(blob, s["q"], z, z, fe)
    assert _rel(ds, ds_ref) < max(tol, 1e-8)
    assert np.abs(lam.reshape(-1) - np.einsum("bi,bi->b", jtf, ds_ref)).max() / (1 + np.abs(lam).max()) < max(tol, 1e-8)


def _chk_twists(blob, s, o, tol):
    # v and a apart, every state on its own scale: a wrong state, or a term that is small next to the batch's largest |a|, cannot hide.
    # The call feeds x["tau"] as ydd, so the reference does.
    err = K.block_errors(o[0], K.body_twists(blob, s["q"], s["qd"], s["tau"], big=_big(blob)))
    assert err.max() < tol, f"state {int(err.max(axis=1).argmax())}: v {err[:, 0].max():.2e}, a {err[:, 1].max():.2e} against {tol:.0e}"


def _osim_frames(blob):
    return [_body_index(blob, b) for b in OSIM_BODIES], [OFFSET, (0.0, 0.0, 0.0)]


def _chk_osim(blob, s, o, tol, frames=None):
    # frames: (bodies, offsets) of the call, the table's when None.  J against the numpy recursion's frame Jacobians: the identity below
    # has the kernel's own J on both sides, and passes a frame on the wrong body or a dropped offset
    Linv, J = o
    J_ref = K.frame_jacobians(blob, s["q"], *(frames or _osim_frames(blob)), big=_big(blob))
    assert _rel(J, J_ref) < max(tol, 1e-9)
    # Linv = J H^-1 J^T, H^-1 from the oracle's forward dynamics (columns of d ydd / d tau)
    Hinv = _fd_columns(blob, s["q"], np.zeros_like(s["qd"]), np.zeros_like(s["qd"]), "dtau")
    assert _rel(Linv, np.einsum("bij,bjk,blk->bil", J, Hinv, J)) < max(tol, 1e-8)


def _chk_project(blob, s, o, tol):
    q_ref, ok_ref = O.project_positions(blob, s["q_start"])
    got, ok = o
    both = ok.astype(bool) & ok_ref
    assert both.any()
    assert np.abs(got[both] - q_ref[both]).max() < (1e-7 if tol < 1e-6 else 1e-3)


def _chk_spanning(blob, s, o, tol):
    assert _rel(o[0], O.spanning_state(blob, s["q"], s["qd"])[1]) < max(tol, 1e-10)
    # qdd_span = G ydd + g (the call feeds x["tau"] as ydd), at the bound test_spanning_recovery_matches_oracle holds the implicit bias to
    ref = K.spanning_rates(blob, s["q"], s["qd"], s["tau"], big=_big(blob))[1]
    g = ref - K.spanning_rates(blob, s["q"], np.zeros_like(s["qd"]), s["tau"], big=_big(blob))[1]
    assert np.abs(o[1] - ref).max() < max(tol, 1e-8) * (1 + np.abs(g).max())


def _chk_indep(blob, s, o, tol):
    # engine coordinates in, engine coordinates out: valid states come back unchanged
    q, qd, status = o
    assert (status == 0).all()
    assert np.abs(q - s["q"]).max() < (1e-12 if tol < 1e-6 else 1e-6) and np.abs(qd - s["qd"]).max() < (1e-12 if tol < 1e-6 else 1e-6)


OFFSET = (0.05, -0.02, 0.1)
# contact frames on links, not rotors: a frame on a rotor sends the inverse OSIM and applyTestForce from the force-propagation kernel
# (capi.cpp, choose_osim) to the unit-wrench route (Mini Cheetah)
FORCE_BODY = "FL_knee_link"
OSIM_BODIES = ("FR_knee_link", "FL_knee_link")


def _body_index(blob, name):
    from test_gpu_parity import _body_index as index

    return index(blob, name)


def _test_force(plan, x):
    return plan.apply_test_force(x["q"], _body_index(plan.blob, FORCE_BODY), OFFSET, x["force"])


def _inv_osim(plan, x):
    return plan.inv_osim(x["q"], *_osim_frames(plan.blob), with_jacobian=True)


def _project(plan, x):
    # (in place: the input is refilled from q_start inside the captured call, so every replay starts from the same positions)
    x["q_proj"].copy_(x["q_start"])
    return x["q_proj"], plan.project_positions(x["q_proj"])

ENTRY = {
    "aba": (_aba, _chk_aba),
    "aba_fext": (_aba_fext, lambda b, s, o, t: _chk_aba(b, s, o, t, True)),
    "rnea": (_rnea, _chk_rnea),
    "rnea_fext": (_rnea_fext, lambda b, s, o, t: _chk_rnea(b, s, o, t, True)),
    "bias": (lambda p, x: (p.bias_force(x["q"], x["qd"]),), _chk_bias),
    "mass_matrix": (lambda p, x: (p.mass_matrix(x["q"]),), _chk_mass),
    "fd_dtau": (lambda p, x: (p.fd_dtau(x["q"]),), _chk_dtau),
    "fd_dqd": (lambda p, x: (p.fd_dqd(x["q"], x["qd"], x["tau"]),), _chk_dqd),
    "fd_dq": (lambda p, x: (p.fd_dq(x["q"], x["qd"], x["tau"]),), _chk_dq),
    "fd_derivatives": (lambda p, x: tuple(p.fd_derivatives(x["q"], x["qd"], x["tau"]).values()), _chk_derivs),
    "body_poses": (lambda p, x: (p.body_poses(x["q"]),), _chk_poses),
    # (twists: no oracle entry point; the numpy recursion of kinematics_ref.py, pinned to the oracle's inverse dynamics on the CPU)
    "body_twists": (lambda p, x: (p.body_twists(x["q"], x["qd"], x["tau"]),), _chk_twists),
    "apply_test_force": (_test_force, _chk_force),
    "inv_osim": (_inv_osim, _chk_osim),
    "project_positions": (lambda p, x: _project(p, x), _chk_project),
    # (fp32 states sit within rounding of the manifold, not within 1e-8)
    "state_to_independent": (lambda p, x: p.state_to_independent(x["q"], x["qd"], tol=1e-8 if x["q"].dtype.itemsize == 8 else 1e-3), _chk_indep),
    "spanning": (lambda p, x: p.spanning(x["q"], x["qd"], x["tau"]), _chk_spanning),
}

CASES = []
for _ep in ("aba", "aba_fext", "rnea", "rnea_fext"):
    CASES += [("chain", "urdf_mini_cheetah", {}, B_CHAIN, _ep), ("latency", "urdf_mini_cheetah", {}, 300, _ep),
              ("interpreter", "urdf_mit_humanoid", {"GRBDA_NO_CHAIN": "1"}, 1000, _ep), ("gen1", "urdf_four_bar", {}, 1000, _ep),
              ("spanning_tree", "parallel_chain_exp_d10_l16", {}, 300, _ep), ("two_parent", "two_parent", {}, 300, _ep)]
CASES += [("crba", "urdf_mini_cheetah", {}, B_CHAIN, "mass_matrix"), ("no_crba", "urdf_mini_cheetah", {"GRBDA_NO_CRBA": "1"}, 1000, "mass_matrix"),
          ("chain", "urdf_mini_cheetah", {}, B_CHAIN, "bias"), ("chain", "urdf_mini_cheetah", {}, 1000, "fd_dtau"),
          ("chain", "urdf_mini_cheetah", {}, 1000, "fd_dqd"), ("chain", "urdf_mini_cheetah", {}, 1000, "fd_dq"),
          ("minv", "urdf_mini_cheetah", {}, 1001, "fd_derivatives"), ("dense", "urdf_mini_cheetah", {"GRBDA_NO_MINV": "1"}, 1001, "fd_derivatives"),
          ("manifold", "tello", {}, 301, "fd_derivatives"), ("manifold", "urdf_four_bar", {}, 301, "fd_dq"),
          ("chain", "urdf_mini_cheetah", {}, B_CHAIN, "body_poses"), ("chain", "urdf_mini_cheetah", {}, B_CHAIN, "body_twists"),
          ("chain", "urdf_mini_cheetah", {}, 1000, "apply_test_force"), ("chain", "urdf_mini_cheetah", {}, 1000, "inv_osim"),
          ("no_efpa", "urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, 300, "inv_osim"),
          ("implicit", "urdf_four_bar", {}, 1000, "project_positions"), ("implicit", "urdf_four_bar", {}, 1000, "state_to_independent"),
          ("implicit", "urdf_four_bar", {}, 1000, "spanning"), ("spanning_tree", "parallel_chain_exp_d10_l16", {}, 300, "mass_matrix")]
# twists on the routes the Mini Cheetah row does not reach: implicit differentials, a loop cluster, big clusters, a roll-pitch-yaw base
CASES += [("implicit", "tello_with_arms", {}, 300, "body_twists"), ("implicit", "urdf_four_bar", {}, 300, "body_twists"),
          ("spanning_tree", "parallel_chain_exp_d10_l16", {}, 300, "body_twists"), ("chain", "urdf_mini_cheetah_rpy", {}, 300, "body_twists")]
IDS = [f"{ep}-{route}-{model}-B{B}" for route, model, env, B, ep in CASES]


@functools.lru_cache(maxsize=8)
def _host_inputs(blob, n_bodies, B, seed, dtype, max_cond=None):
    """the numpy inputs of B states, rounded to `dtype` (the fp32 oracle inputs are the rounded ones); shared, so never written to"""
    import torch

    q, qd, tau = _states(blob, B, seed, max_cond)
    rng = np.random.default_rng(seed)
    s = {"q": q, "qd": qd, "tau": tau, "fext": rng.uniform(-1, 1, (B, n_bodies, 6)), "force": rng.uniform(-1, 1, (B, 3))}
    # projection input: the states moved off the manifold by a little (Newton has something to do)
    s["q_start"] = q + rng.uniform(-0.05, 0.05, q.shape)
    s = {k: np.asarray(torch.as_tensor(v, dtype=dtype).double()) for k, v in s.items()}
    return s


def _inputs(blob, plan, B, seed, dtype, gpu, max_cond=None):
    import torch

    s = dict(_host_inputs(blob, plan.n_bodies, B, seed, dtype, max_cond))
    x = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=dtype, device=gpu) for k, v in s.items()}
    x["q_proj"] = x["q_start"].clone()
    return s, x


def _host(outs):
    return [o.detach().cpu().double().numpy() if o.is_floating_point() else o.detach().cpu().numpy() for o in outs]


# ---- guarded calls: what test_buffer_edges_gpu.py and test_batch_ladder_gpu.py share ---------------------------------------------------
# Entry points whose checker differentiates the oracle along the constraint manifold.  When EVERY state of a draw is held to the
# reference's 2e-5, the draw bounds cond(K_d) of the implicit loops as the derivative tests of test_gpu_parity.py do (models.py,
# valid_states: a state that satisfies phi to 1e-12 sits 1e-12 / sigma_min off the manifold, and the difference quotient along the
# manifold then differs from the exact derivative at the state; measured on the four-bar, fp64: 1.2e-4 at cond 422, 8e-6 at 325,
# 1.5e-6 at 150 and below).  Explicit models are not affected by the bound.
DIFFERENTIATES = ("fd_dq", "fd_derivatives")


def draw_bound(entry):
    return 100.0 if entry in DIFFERENTIATES else None


TILE = 64  # states per tile of the tiled kernels (one wavefront); the derivative pipeline packs groups of 4 states


def edge_states(B, n_random=4, seed=0):
    """sorted states to hold against the oracle: 0, B - 1, the first and the last state of the last tile and of the last group of four,
    and a seeded few"""
    idx = {0, B - 1, ((B - 1) // TILE) * TILE, ((B - 1) // 4) * 4}
    idx |= set(np.random.default_rng(seed).choice(B, min(B, n_random), replace=False).tolist())
    return np.array(sorted(idx))


def _owned_by_projection(blob):
    """columns of q that project_positions may change: the dependent positions of the implicit clusters"""
    m = parse_clusters(blob)
    own = np.zeros(m["nq"], dtype=bool)
    for c in m["clusters"]:
        qi, nsv, ctype, io = c[3], c[8], c[9], c[11]
        if ctype in (2, 3):
            flags = m["ints"][io + 1: io + 1 + nsv] if ctype == 2 else m["ints"][io: io + nsv]
            for j in range(nsv):
                own[qi + j] = not flags[j]
    return own


def run_guarded(plan, call, s, dtype, gpu, lead, out_arena=None):
    """call(plan, x) with every input and every output in an arena of guarded.py (alignment `lead`).  Asserts: every output arena has
    both bands intact and no element left unwritten; every input arena, bands included, is bit for bit what it was (project_positions'
    q: its bands and the columns it does not own); every floating-point output is finite.  Returns the outputs as numpy arrays.
    out_arena: "aba" / "rnea" -- forward / inverse dynamics again with a caller-supplied out= arena, which must give the same bits."""
    import torch

    import guarded

    x = {k: guarded.place(v, dtype, gpu, lead) for k, v in s.items()}
    x["q_proj"] = guarded.place(s["q_start"], dtype, gpu, lead)
    before = {k: guarded.snapshot(v) for k, v in x.items()}
    with guarded.guarded_outputs(lead) as made:
        outs = call(plan, x)
    torch.cuda.synchronize()
    assert made, "the call allocated no output through torch.empty"
    for i, a in enumerate(made):
        left = guarded.check(a)
        assert left == 0, f"output arena {i} {tuple(a.shape)} {a.dtype}: {left} of {a.numel()} elements never written"
    for k, v in x.items():
        if k == "q_proj":
            assert guarded.same_bits(v, before[k], 0, v.numel()), "bands of the projected q changed"
            keep = torch.as_tensor(~_owned_by_projection(plan.blob), device=gpu)
            assert torch.equal(v[:, keep].view(torch.uint8), x["q_start"][:, keep].view(torch.uint8)), "project_positions changed a column it does not own"
        else:
            assert guarded.same_bits(v, before[k]), f"input {k} changed"
    host = _host(outs)
    for i, o in enumerate(host):
        assert np.isfinite(o).all(), f"output {i}: {int((~np.isfinite(o)).sum())} non-finite values, first at {np.argwhere(~np.isfinite(o))[0]}"
    if out_arena is not None:
        out = guarded.arena(outs[0].shape, dtype, gpu, lead)
        fn = plan.forward_dynamics if out_arena == "aba" else plan.inverse_dynamics
        with guarded.guarded_outputs(lead) as none_made:
            back = fn(x["q"], x["qd"], x["tau"], out=out)
        torch.cuda.synchronize()
        assert back is out and not none_made and guarded.check(out) == 0
        assert np.array_equal(_host([out])[0], host[0]), "out= gives other bits than the allocated output"
        for k in ("q", "qd", "tau"):
            assert guarded.same_bits(x[k], before[k]), f"input {k} changed"
    return host


def same_bits_np(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)) and len(a) == len(b)


@functools.lru_cache(maxsize=None)
def plan_for(model, env):
    """the plan of `model` compiled under the plan-time switches `env` (a tuple of (name, value) pairs); the switches are read once, at
    compilation, so the environment is put back before this returns"""
    old = {k: os.environ.get(k) for k, _ in env}
    os.environ.update(dict(env))
    try:
        return G.Plan(_model(model))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
