"""Graph capture of every stream-taking device entry point ("Graph capture"), fp32 and fp64, on each route a plan can take.

For every case: (a) capture succeeds after one eager call of the same batch on the capturing stream; (b) two replays with fresh inputs
(written in place) equal, bit for bit, eager calls on those inputs; (c) a seeded sample agrees with the oracle at the tolerances of
test_gpu_parity.py; (d) the graph has the same nodes as a capture of the same call taken after an eager call of TWICE the batch on a
fresh stream -- the launch sequence a graph records does not depend on what the stream held before.  Then the refusals of the
contract: a capture that would have to grow a slab, and release_work while a stream captures, raise GRBDA_EINVAL before any launch.
graph_capture.py gives the capture helper and the lifetime rules these tests follow."""
import os

import numpy as np
import pytest

import oracle_py as O
import generalized_rbda_amd as G
from generalized_rbda_amd.states import parse_clusters, random_states
from graph_capture import capture
from models import ROBOT_MODELS, valid_states, zoo

pytestmark = pytest.mark.gpu
TOL64 = 1e-9
TOL32 = 1e-3
B_CHAIN = 65536 + 37  # beyond four tiles per SIMD of 256 CUs: the chain kernels, not latency mode
N_ORACLE = 6         # states of each replay checked against the oracle


_BIG = set()  # blobs of plans with clusters beyond the structured limits: the oracle built with room for them (big=True)


def _big(blob):
    return blob in _BIG


def _model(name):
    if name == "two_parent":
        from test_capi_cpu import two_parent_model

        return two_parent_model().serialize()
    if name.startswith("parallel_chain"):
        blob = G.urdf_to_blob(os.path.join(ROBOT_MODELS, name + ".urdf"))
        _BIG.add(blob)
        return blob
    return zoo()[name]


def _states(blob, B, seed):
    if _big(blob):
        return valid_states(blob, B, config_index=seed, big=True, scale=0.5, max_cond=50)
    if any(c[9] in (2, 3) for c in parse_clusters(blob)["clusters"]):  # implicit loops: states on the constraint manifold
        return valid_states(blob, B, config_index=seed)
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


def _chk_osim(blob, s, o, tol):
    # Linv = J H^-1 J^T, H^-1 from the oracle's forward dynamics (columns of d ydd / d tau)
    Linv, J = o
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


def _chk_indep(blob, s, o, tol):
    # engine coordinates in, engine coordinates out: valid states come back unchanged
    q, qd, status = o
    assert (status == 0).all()
    assert np.abs(q - s["q"]).max() < (1e-12 if tol < 1e-6 else 1e-6) and np.abs(qd - s["qd"]).max() < (1e-12 if tol < 1e-6 else 1e-6)


OFFSET = (0.05, -0.02, 0.1)
# contact frames on links, not rotors: a frame on a rotor sends the inverse OSIM and applyTestForce from the force-propagation kernel
# (inv_osim_chain) to the unit-wrench route (Mini Cheetah)
FORCE_BODY = "FL_knee_link"
OSIM_BODIES = ("FR_knee_link", "FL_knee_link")


def _body_index(blob, name):
    from test_gpu_parity import _body_index as index

    return index(blob, name)


def _test_force(plan, x):
    return plan.apply_test_force(x["q"], _body_index(plan.blob, FORCE_BODY), OFFSET, x["force"])


def _inv_osim(plan, x):
    return plan.inv_osim(x["q"], [_body_index(plan.blob, b) for b in OSIM_BODIES], [OFFSET, (0.0, 0.0, 0.0)], with_jacobian=True)


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
    # (twists: no oracle entry point; test_gpu_parity.py holds them against the motion -- here (a), (b) and (d))
    "body_twists": (lambda p, x: (p.body_twists(x["q"], x["qd"], x["tau"]),), None),
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
IDS = [f"{ep}-{route}-{model}-B{B}" for route, model, env, B, ep in CASES]


def _inputs(blob, plan, B, seed, dtype, gpu):
    import torch

    q, qd, tau = _states(blob, B, seed)
    rng = np.random.default_rng(seed)
    s = {"q": q, "qd": qd, "tau": tau, "fext": rng.uniform(-1, 1, (B, plan.n_bodies, 6)), "force": rng.uniform(-1, 1, (B, 3))}
    # projection input: the states moved off the manifold by a little (Newton has something to do)
    s["q_start"] = q + rng.uniform(-0.05, 0.05, q.shape)
    c = lambda a: np.asarray(torch.as_tensor(a, dtype=dtype).double())  # (the fp32 oracle inputs are the rounded ones)
    s = {k: c(v) for k, v in s.items()}
    x = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=dtype, device=gpu) for k, v in s.items()}
    x["q_proj"] = x["q_start"].clone()
    return s, x


def _host(outs):
    return [o.detach().cpu().double().numpy() if o.is_floating_point() else o.detach().cpu().numpy() for o in outs]


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("route,model,env,B,entry", CASES, ids=IDS)
def test_capture_replay_matches_eager_and_oracle(route, model, env, B, entry, dtype_name, gpu, monkeypatch):
    import torch

    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob = _model(model)
    plan = G.Plan(blob)
    if entry in ("aba", "rnea"):
        name = plan.kernel_name(entry, dtype_name, B)
        assert {"chain": "_chain_kernel<", "latency": "_chain_lm_kernel<", "interpreter": f"{entry}_kernel<", "gen1": "_gen1_kernel<"}.get(
            route, "") in name, name
    if route in ("spanning_tree", "two_parent"):
        assert plan.info().spanning_tree_route == 1
    call, check = ENTRY[entry]
    tol = TOL64 if dtype == torch.float64 else TOL32
    _, x = _inputs(blob, plan, B, 1, dtype, gpu)
    cap = capture(lambda: call(plan, x))  # (a)
    try:
        assert cap.nodes["kernel"] >= 1
        for seed in (2, 3):  # (b) fresh inputs in place, replay, against an eager call on the same inputs
            s, fresh = _inputs(blob, plan, B, seed, dtype, gpu)
            for k in x:
                x[k].copy_(fresh[k])
            got = _host(cap.replay())
            with torch.cuda.stream(cap.stream):  # (the eager call on the capturing stream: same slab, same chunks)
                want = _host(call(plan, x))
            cap.stream.synchronize()
            for a, b in zip(got, want):
                assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"replay {seed} differs from the eager call"
            if check is not None:  # (c)
                idx = np.random.default_rng(seed).choice(B, N_ORACLE, replace=False)
                check(blob, {k: v[idx] for k, v in s.items()}, [a[idx] for a in got], tol)
        nodes = cap.nodes
    finally:
        cap.drop()
    # (d) after an eager call of 2B on a fresh stream: the same launch sequence
    _, x2 = _inputs(blob, plan, 2 * B, 4, dtype, gpu)
    cap2 = capture(lambda: call(plan, x), warm=lambda: call(plan, x2))
    try:
        assert cap2.nodes == nodes, f"{cap2.nodes} after a warm-up of 2B, {nodes} after one of B"
    finally:
        cap2.drop()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
# (id, model, switches, entry point, warm-up B, captured B, the slab that would have to grow): the interpreter's scratch slab (its
# persistent grid grows with the batch up to n_cu * waves tiles), the work slab of the difference batches (fixed 256 MiB chunks), and the
# zero block of the inverse OSIM's force-propagation route -- both batches of 257 tiles, so that its scratch slab (a grid of
# min(4 n_cu, tiles) wavefronts) keeps its size and only the zero block, B nv scalars, would grow
REFUSALS = [
    ("ensure_scratch", "urdf_mit_humanoid", {"GRBDA_NO_CHAIN": "1"}, "aba", 200, 4 * 4096 + 3, "scratch slab"),
    ("ensure_work", "urdf_mini_cheetah", {"GRBDA_NO_CRBA": "1"}, "mass_matrix", 200, 4 * 4096 + 3, "work buffer"),
    ("inv_osim_zero_block", "urdf_mini_cheetah", {}, "inv_osim", 4 * 4096 + 1, 4 * 4096 + 3, "work buffer"),
]


@pytest.mark.parametrize("what,model,env,entry,B_warm,B_big,slab", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_capture_of_a_larger_batch_is_refused(what, model, env, entry, B_warm, B_big, slab, gpu, monkeypatch):
    import torch

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob = _model(model)
    plan = G.Plan(blob)
    call, _ = ENTRY[entry]
    _, small = _inputs(blob, plan, B_warm, 1, torch.float64, gpu)
    _, big = _inputs(blob, plan, B_big, 2, torch.float64, gpu)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        call(plan, small)
    stream.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with pytest.raises(G.GrbdaError) as err:
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            call(plan, big)
    assert err.value.code == -1 and "capture" in str(err.value) and slab in str(err.value), str(err.value)  # GRBDA_EINVAL
    from graph_capture import node_counts

    assert node_counts(g)["kernel"] == 0  # (host-side, before any launch; the graph is never replayed)
    stream.synchronize()
    g.reset()
    # the stream is usable again, and the small batch still captures
    cap = capture(lambda: call(plan, small), stream=stream)
    cap.drop()


def test_release_work_during_capture_is_refused(gpu):
    import torch

    blob = zoo()["urdf_mini_cheetah"]
    plan = G.Plan(blob)  # (a fresh plan: its only slab is the capturing stream's)
    _, x = _inputs(blob, plan, 200, 1, torch.float64, gpu)
    call, _ = ENTRY["fd_derivatives"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        call(plan, x)
    stream.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with pytest.raises(G.GrbdaError) as err:
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            call(plan, x)
            plan.release_work()
    assert err.value.code == -1
    stream.synchronize()
    g.reset()
    assert plan.release_work() > 0  # (the slab was kept, and goes now)


def test_capped_derivatives_capture_after_their_warm_up(gpu, monkeypatch):
    """GRBDA_WORK_MAX_MB=1, Mini Cheetah fp32, 20 000 states: the whole-batch ydd alone is larger than the cap, so the forward dynamics
    run per chunk; the eager call keeps within the cap, its capture needs no larger slab, and the replay equals the uncapped (one-chunk)
    call bit for bit (test_chunk_seams_gpu.py holds this route against the oracle at its seams)."""
    import torch

    monkeypatch.setenv("GRBDA_WORK_MAX_MB", "1")
    blob = zoo()["urdf_mini_cheetah"]
    plan = G.Plan(blob)
    B = 20000
    call, _ = ENTRY["fd_derivatives"]
    _, x = _inputs(blob, plan, B, 1, torch.float32, gpu)
    cap = capture(lambda: call(plan, x))
    try:
        got = _host(cap.replay())
        with torch.cuda.stream(cap.stream):
            want = _host(call(plan, x))
        cap.stream.synchronize()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert cap.nodes["kernel"] >= 3 * 10  # (many chunks)
    finally:
        cap.drop()
    held = plan.release_work()
    assert 0 < held <= (1 << 20) + 256
    monkeypatch.delenv("GRBDA_WORK_MAX_MB")
    whole = _host(call(plan, x))
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(got, whole)), "the capped replay differs from the one-chunk call"
