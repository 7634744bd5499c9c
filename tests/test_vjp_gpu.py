"""The vector-Jacobian products on the GPU (run with -m gpu on an MI355X): Plan.id_vjp / fd_vjp (grbda_rnea_vjp_* / grbda_aba_vjp_*) and the
autograd functions built on them.

The cotangent g is drawn per state from a seeded generator and scaled to unit 1-norm, so that the matrix bounds of the project carry
over unchanged: |sum_i g_i (M - M_ref)_ij| <= max |M - M_ref|.  Every error below is relative to 1 + max |reference MATRIX| of the states
compared, as the matrix tests state theirs.

id_vjp, fp64: against einsum("bi,bij->bj", g, ref) of id_derivative_refs.refs_of -- "q" 2e-5, "qd" 1e-8, "ydd" 1e-9 -- on every state of
every batch size of id_derivative_refs.BATCHES and every model of id_derivative_refs.MODELS but tree16_fixed (nv = 4: sixteen states per
wavefront and partial packs; 18: three and idle lanes; 31 / 32: two per wavefront against one; 44 / 45: the fp32 interleave flip of the
run unpack; 64: every lane a column; 65: two column blocks, the second with one live lane, on the difference route; the four-bar and
GRBDA_NO_ANALYTIC: difference routes).  fd_vjp, fp64: "tau" and "qd" against g^T of the oracle's exact difference columns at 1e-8, "q"
against g^T of its central differences at 2e-5 (the first five states on the larger models), "ydd" the bits of forward_dynamics.

fp32, explicit models: against the same entry point's fp64 result on the rounded inputs.  id_vjp at 1e-3 of 1 + max |fp64 result| (nothing is
inverted).  fd_vjp has no figure of its own: on the same states g^T (the fp32 matrices of fd_derivatives) is formed too -- those matrices
ARE d ydd / d x, so no sign goes in front -- and its error against the fp64 result measured; fd_vjp is held to max(1e-3, twice that), the
factor covering the other summation order.  Both are printed.

Every call that is compared with a reference goes through entry_points.run_guarded (NaN-canary arenas around inputs and outputs)."""
import functools
import itertools
import os

import numpy as np
import pytest

import generalized_rbda_amd as G
from entry_points import TOL32, TOL64, _dq_oracle, _fd_columns, _host, _states, edge_states, run_guarded, same_bits_np
from graph_capture import capture
from id_derivative_refs import BATCHES, B_MAX, MODELS, blob_of, is_explicit, oracle_dq, refs_of, states_of

pytestmark = pytest.mark.gpu
ID_NAMES, FD_NAMES = ("q", "qd", "ydd"), ("q", "qd", "tau")
ID_REF = {"q": "dq", "qd": "dqd", "ydd": "dydd"}
ID_BOUND = {"q": 2e-5, "qd": 1e-8, "ydd": 1e-9}
FD_BOUND = {"q": 2e-5, "qd": 1e-8, "tau": 1e-8}
ID_MODELS = ["pair_rotor_chain_4", "mini_cheetah", "mini_cheetah_rpy", "tree31_fixed", "tree32_floating", "tree44_floating", "tree45_fixed",
             "tree64_floating", "tree65_fixed", "four_bar", "mini_cheetah_no_analytic"]
FD_MODELS = ["mini_cheetah", "mini_cheetah_rpy", "pair_rotor_chain_4", "tree64_floating", "four_bar"]
DQ_STATES = 5  # states of the oracle's d ydd / d q loop on models with more than four velocities (CPU time)


def _plan(name):
    """the model's plan under its plan-time switches"""
    if name not in _plan.made:
        env = dict(MODELS[name][1])
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            _plan.made[name] = G.Plan(blob_of(name))
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return _plan.made[name]


_plan.made = {}


def _dtype(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def unit_cotangent(B, nv, seed, dt="f64"):
    """g[B, nv], every row of unit 1-norm (then rounded to the type)"""
    g = np.random.default_rng([seed, 4711]).uniform(-1, 1, (B, nv))
    g /= np.abs(g).sum(axis=1, keepdims=True)
    return g if dt == "f64" else g.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs_of(name, dt="f64"):
    """the model's B_MAX states with their cotangents; shared, never written to (the forward side takes "ydd" as its tau)"""
    s = dict(states_of(name, dt))
    s["g"] = unit_cotangent(B_MAX, s["qd"].shape[1], len(name), dt)
    return s


def _id_call(want=ID_NAMES):
    return lambda plan, x: tuple(plan.id_vjp(x["q"], x["qd"], x["ydd"], x["g"], want=want).values())


def _fd_call(want=FD_NAMES):
    return lambda plan, x: tuple(plan.fd_vjp(x["q"], x["qd"], x["ydd"], x["g"], want=want).values())


def _run(call, names, name, dt, B, gpu, want=None, plan=None):
    want = names if want is None else want
    s = {k: v[:B] for k, v in inputs_of(name, dt).items()}
    keys = [k for k in names + ("ydd",) if k in want] if names is FD_NAMES else [k for k in names if k in want]
    return dict(zip(keys, run_guarded(plan or _plan(name), call(want), s, _dtype(dt), gpu, 0)))


def run_id(name, dt, B, gpu, want=None, plan=None):
    return _run(_id_call, ID_NAMES, name, dt, B, gpu, want, plan)


def run_fd(name, dt, B, gpu, want=None, plan=None):
    return _run(_fd_call, FD_NAMES, name, dt, B, gpu, want, plan)


def contract(g, M):
    return np.einsum("bi,bij->bj", g, M)


def rel_to_matrix(got, g, M):
    """max |got - g^T M| relative to 1 + max |M|"""
    return float(np.abs(got - contract(g, M)).max() / (1.0 + np.abs(M).max()))


@functools.lru_cache(maxsize=None)
def fd_refs_of(name):
    """the oracle's d ydd / d tau and d ydd / d qd of all B_MAX states and its d ydd / d q of the first n_dq"""
    blob, s = blob_of(name), inputs_of(name)
    n_dq = B_MAX if s["qd"].shape[1] <= 4 else DQ_STATES
    return {"tau": _fd_columns(blob, s["q"], s["qd"], s["ydd"], "dtau"), "qd": _fd_columns(blob, s["q"], s["qd"], s["ydd"], "dqd"),
            "q": _dq_oracle(blob, s["q"][:n_dq], s["qd"][:n_dq], s["ydd"][:n_dq])}


def hold_id_f64(name, got, B, what=""):
    g, ref = inputs_of(name)["g"][:B], refs_of(name)
    err = {k: rel_to_matrix(got[k], g, ref[ID_REF[k]][:B]) for k in got}
    print(f"{name} id_vjp f64 B={B}{what}: " + " ".join(f"{k} {e:.2e}" for k, e in err.items()))
    for k, e in err.items():
        assert e < ID_BOUND[k], (k, e)


def hold_fd_f64(name, got, B, what=""):
    g, ref = inputs_of(name)["g"][:B], fd_refs_of(name)
    err = {}
    for k in (k for k in FD_NAMES if k in got):
        n = min(B, len(ref[k]))
        err[k] = rel_to_matrix(got[k][:n], g[:n], ref[k][:n])
    print(f"{name} fd_vjp f64 B={B}{what}: " + " ".join(f"{k} {e:.2e}" for k, e in err.items()))
    for k, e in err.items():
        assert e < FD_BOUND[k], (k, e)


@pytest.mark.parametrize("name", ID_MODELS)
def test_id_vjp_matches_the_contracted_oracle_matrices_at_every_batch_size(name, gpu):
    plan = _plan(name)
    for B in BATCHES:
        got = run_id(name, "f64", B, gpu)
        assert list(got) == list(ID_NAMES) and all(v.shape == (B, plan.nv) for v in got.values())
        hold_id_f64(name, got, B)


@pytest.mark.parametrize("name", FD_MODELS)
def test_fd_vjp_matches_the_contracted_oracle_columns_at_every_batch_size(name, gpu):
    import torch

    plan, s = _plan(name), inputs_of(name)
    for B in BATCHES:
        got = run_fd(name, "f64", B, gpu, want=FD_NAMES + ("ydd",))
        assert list(got) == list(FD_NAMES) + ["ydd"] and all(v.shape == (B, plan.nv) for v in got.values())
        hold_fd_f64(name, got, B)
        q, qd, tau = (torch.as_tensor(s[k][:B], dtype=torch.float64, device=gpu) for k in ("q", "qd", "ydd"))
        assert np.array_equal(got["ydd"], plan.forward_dynamics(q, qd, tau).cpu().numpy()), "ydd has other bits than forward_dynamics"


@pytest.mark.parametrize("name", [n for n in ID_MODELS if is_explicit(blob_of(n))])
def test_id_vjp_fp32_follows_its_fp64_result(name, gpu):
    for B in BATCHES:
        got = run_id(name, "f32", B, gpu)
        s = {k: v[:B] for k, v in inputs_of(name, "f32").items()}
        want = dict(zip(ID_NAMES, run_guarded(_plan(name), _id_call(), s, _dtype("f64"), gpu, 0)))
        for k in ID_NAMES:
            err = np.abs(got[k] - want[k]).max() / (1.0 + np.abs(want[k]).max())
            print(f"{name} id_vjp f32 B={B} {k}: {err:.2e}")
            assert err < TOL32, (k, err)


@pytest.mark.parametrize("name", [n for n in FD_MODELS if is_explicit(blob_of(n))])
def test_fd_vjp_fp32_is_as_good_as_the_contracted_fp32_matrices(name, gpu):
    import torch

    plan = _plan(name)
    for B in BATCHES:
        got = run_fd(name, "f32", B, gpu)
        s = {k: v[:B] for k, v in inputs_of(name, "f32").items()}
        want = dict(zip(FD_NAMES, run_guarded(plan, _fd_call(), s, _dtype("f64"), gpu, 0)))
        q, qd, tau = (torch.as_tensor(s[k], dtype=torch.float32, device=gpu) for k in ("q", "qd", "ydd"))
        mats = {k: v.double().cpu().numpy() for k, v in plan.fd_derivatives(q, qd, tau).items()}
        for k, m in zip(FD_NAMES, ("dq", "dqd", "dtau")):
            scale = 1.0 + np.abs(want[k]).max()
            by_matrices = np.abs(contract(s["g"], mats[m]) - want[k]).max() / scale
            err = np.abs(got[k] - want[k]).max() / scale
            print(f"{name} fd_vjp f32 B={B} {k}: {err:.2e}; g^T fd_derivatives: {by_matrices:.2e}")
            assert err < max(TOL32, 2 * by_matrices), (k, err, by_matrices)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["mini_cheetah", "tree65_fixed"])
def test_every_subset_of_want_has_the_bits_of_the_full_call(name, dt, gpu):
    B = 7
    for run, names in ((run_id, ID_NAMES), (run_fd, FD_NAMES)):
        full = run(name, dt, B, gpu)
        for n in (1, 2):
            for want in itertools.combinations(names, n):
                got = run(name, dt, B, gpu, want)
                assert list(got) == list(want)
                for k in want:
                    assert np.array_equal(got[k], full[k]), f"{run.__name__}: {k} of want={want} differs from the call for all three"
    with_ydd = run_fd(name, dt, B, gpu, ("tau", "ydd"))
    assert list(with_ydd) == ["tau", "ydd"] and np.array_equal(with_ydd["tau"], full["tau"])


def test_a_chunk_seam_inside_the_batch(gpu, monkeypatch):
    """tree64_floating, B = 70 under GRBDA_WORK_MAX_MB=1: the slab holds one tile of 64 states (2 x 64 x 64 + O(64) doubles each), so the
    batch goes through in passes of 64 and 6 states"""
    name, B = "tree64_floating", 70
    plan = G.Plan(blob_of(name))  # (a plan of its own: its slabs are measured)
    nn = plan.nv * plan.nv
    for run, hold in ((run_id, hold_id_f64), (run_fd, hold_fd_f64)):
        monkeypatch.setenv("GRBDA_WORK_MAX_MB", "1")
        try:
            got = run(name, "f64", B, gpu, plan=plan)
        finally:
            monkeypatch.delenv("GRBDA_WORK_MAX_MB")
        held = plan.release_work()
        print(f"{run.__name__}: work slabs held {held} bytes; the matrices of the whole batch would take {B * 2 * nn * 8}")
        assert 64 * 2 * nn * 8 <= held < 65 * 2 * nn * 8 + 64 * 16 * plan.nv * 8  # one tile of states, not the batch
        hold(name, got, B, " in passes of 64 and 6")


def test_the_contraction_kernel_past_one_trip_of_its_grid(gpu):
    """pair_rotor_chain_4 at the smallest batch for which a workgroup of the contraction kernel takes a second unit (the launch rule:
    G.vjp_contract_launch), against the numpy contraction of id_derivatives on the edge states"""
    import torch

    plan = _plan("pair_rotor_chain_4")
    n_cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    cap = G.vjp_contract_launch(plan.nv, 1 << 40, n_cu)[1]  # the grid when there is no end of units
    B = cap * (64 // plan.nv) + 1
    assert G.vjp_contract_launch(plan.nv, B - 1, n_cu) == (cap, cap) and G.vjp_contract_launch(plan.nv, B, n_cu) == (cap + 1, cap)
    q, qd, ydd = _states(blob_of("pair_rotor_chain_4"), B, 31)
    s = {"q": q, "qd": qd, "ydd": ydd, "q_start": q, "g": unit_cotangent(B, plan.nv, 31)}
    got = dict(zip(ID_NAMES, run_guarded(plan, _id_call(), s, _dtype("f64"), gpu, 0)))
    x = {k: torch.as_tensor(v, dtype=torch.float64, device=gpu) for k, v in s.items()}
    idx = edge_states(B)
    mats = {k: v[torch.as_tensor(idx, device=gpu)].cpu().numpy() for k, v in plan.id_derivatives(x["q"], x["qd"], x["ydd"]).items()}
    for k in ID_NAMES:
        err = rel_to_matrix(got[k][idx], s["g"][idx], mats[ID_REF[k]])
        print(f"B={B} ({cap + 1} units on {cap} workgroups) {k} on states {idx.tolist()}: {err:.2e}")
        assert err < TOL64, (k, err)


def test_the_position_gradient_follows_gravity(gpu):
    blob = blob_of("mini_cheetah")
    plan = G.Plan(blob)
    plan.set_gravity((1.0, -2.0, -7.0))
    s = {k: v[:5] for k, v in inputs_of("mini_cheetah").items()}
    got, = run_guarded(plan, _id_call(("q",)), s, _dtype("f64"), gpu, 0)
    ref = oracle_dq(plan.blob, s["q"], s["qd"], s["ydd"])
    assert np.abs(ref - refs_of("mini_cheetah")["dq"][:5]).max() / (1 + np.abs(ref).max()) > 1e-3  # (the gravity matters to the reference)
    err = rel_to_matrix(got, s["g"], ref)
    print(f"grad_q at gravity (1, -2, -7): {err:.2e}")
    assert err < 2e-5


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,B", [("mini_cheetah", 70), ("four_bar", 37)])
@pytest.mark.parametrize("call", [_fd_call, _id_call], ids=["fd_vjp", "id_vjp"])
def test_a_captured_call_replays_the_bits_of_the_eager_call(call, name, B, dt, gpu):
    import torch

    plan = _plan(name)
    x = {k: torch.as_tensor(v[:B], dtype=_dtype(dt), device=gpu) for k, v in inputs_of(name, dt).items()}
    cap = capture(lambda: call()(plan, x))
    try:
        assert cap.nodes["kernel"] >= 1
        for k in x:  # (new inputs in place: the states in reverse order)
            x[k].copy_(x[k].flip(0))
        got = _host(cap.replay())
        with torch.cuda.stream(cap.stream):
            want = _host(call()(plan, x))
        cap.stream.synchronize()
        assert same_bits_np(got, want)
        assert all(np.isfinite(a).all() for a in got)
    finally:
        cap.drop()


@pytest.mark.parametrize("name", ["mini_cheetah", "tree65_fixed"])
def test_the_host_array_variants_give_the_bits_of_the_device_calls(name, gpu):
    plan, B = _plan(name), 5
    s = {k: np.ascontiguousarray(v[:B]) for k, v in inputs_of(name).items()}
    ptr = lambda a: a.ctypes.data
    for fn, run, n_out in ((G.lib().grbda_rnea_vjp_host_f64, run_id, 3), (G.lib().grbda_aba_vjp_host_f64, run_fd, 4)):
        out = np.full((n_out, B, plan.nv), np.nan)
        rc = fn(plan._h, ptr(s["q"]), ptr(s["qd"]), ptr(s["ydd"]), ptr(s["g"]), 1e-6, *[ptr(o) for o in out], B, gpu.index or 0)
        assert rc == 0, G.lib().grbda_last_error()
        want = run(name, "f64", B, gpu, want=FD_NAMES + ("ydd",) if n_out == 4 else None)
        for o, (k, w) in zip(out, want.items()):
            assert np.array_equal(o, w), f"{run.__name__}: {k} of the host variant differs from the device call"


@pytest.mark.parametrize("method", ["id_vjp", "fd_vjp"])
def test_the_tensor_arguments_follow_the_rules_of_the_binding(method, gpu):
    """what test_python_args_gpu.py holds every tensor method of Plan to, at B = 3: strided inputs and a side stream give the bits of the
    plain call; a CPU tensor is GrbdaError(-3), one float32 among float64 TypeError, a row short by one column ValueError"""
    import torch

    plan, B = _plan("pair_rotor_chain_4"), 3
    s = inputs_of("pair_rotor_chain_4")
    keys = ("q", "qd", "ydd", "g")
    plain = {k: torch.as_tensor(s[k][:B], dtype=torch.float64, device=gpu) for k in keys}
    call = lambda x, stream=None: list(getattr(plan, method)(*(x[k] for k in keys), stream=stream).values())
    want = [t.clone() for t in call(plain)]

    def strided():
        big = {k: torch.full((2 * B,) + v.shape[1:], float("nan"), dtype=torch.float64, device=gpu) for k, v in plain.items()}
        for k, v in plain.items():
            big[k][::2] = v
        views = {k: v[::2] for k, v in big.items()}
        assert not any(v.is_contiguous() for v in views.values())
        return views

    same = lambda got: all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(got, want)) and len(got) == len(want)
    assert same(call(strided()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = call(strided(), side)
    side.synchronize()
    assert same(got)
    for k in keys:
        with pytest.raises(G.GrbdaError) as e:
            call({**plain, k: plain[k].cpu()})
        assert e.value.code == -3
        with pytest.raises(TypeError):
            call({**plain, k: plain[k].float()})
        with pytest.raises(ValueError):
            call({**plain, k: plain[k][:, :-1]})


def _leaves(name, B, gpu, grads):
    import torch

    s = inputs_of(name)
    x = {k: torch.as_tensor(s[k][:B], dtype=torch.float64, device=gpu) for k in ("q", "qd", "ydd", "g")}
    return x, [x[k].clone().requires_grad_(k in grads) for k in ("q", "qd", "ydd")]


@pytest.mark.parametrize("name", ["mini_cheetah_rpy", "pair_rotor_chain_4"])
@pytest.mark.parametrize("forward", [True, False], ids=["forward_dynamics_ad", "inverse_dynamics_ad"])
def test_autograd_gives_the_bits_of_the_vjp(forward, name, gpu):
    import torch

    plan, B = _plan(name), 5
    x, (q, qd, last) = _leaves(name, B, gpu, ("q", "qd", "ydd"))
    out = (plan.forward_dynamics_ad if forward else plan.inverse_dynamics_ad)(q, qd, last)
    plain = (plan.forward_dynamics if forward else plan.inverse_dynamics)(x["q"], x["qd"], x["ydd"])
    assert torch.equal(out.detach().view(torch.int64), plain.view(torch.int64)), "the forward value has other bits"
    (out * x["g"]).sum().backward()
    want = (plan.fd_vjp if forward else plan.id_vjp)(x["q"], x["qd"], x["ydd"], x["g"])
    for leaf, k in zip((q, qd, last), FD_NAMES if forward else ID_NAMES):
        assert leaf.grad is not None and torch.equal(leaf.grad.view(torch.int64), want[k].view(torch.int64)), k
    # only the last input requires grad: the others get none (and backward asks the library for that one alone)
    x, (q, qd, last) = _leaves(name, B, gpu, ("ydd",))
    ((plan.forward_dynamics_ad if forward else plan.inverse_dynamics_ad)(q, qd, last) * x["g"]).sum().backward()
    assert q.grad is None and qd.grad is None
    assert torch.equal(last.grad.view(torch.int64), want["tau" if forward else "ydd"].view(torch.int64))


@pytest.mark.parametrize("forward", [True, False], ids=["forward_dynamics_ad", "inverse_dynamics_ad"])
def test_autograd_on_a_quaternion_base_refuses_q_and_serves_the_rest(forward, gpu):
    import torch

    plan, B = _plan("mini_cheetah"), 5
    fn = plan.forward_dynamics_ad if forward else plan.inverse_dynamics_ad
    x, (q, qd, last) = _leaves("mini_cheetah", B, gpu, ("q", "qd", "ydd"))
    with pytest.raises(ValueError, match="fd_vjp" if forward else "id_vjp"):
        fn(q, qd, last)
    x, (q, qd, last) = _leaves("mini_cheetah", B, gpu, ("qd", "ydd"))
    (fn(q, qd, last) * x["g"]).sum().backward()
    names = FD_NAMES if forward else ID_NAMES
    want = (plan.fd_vjp if forward else plan.id_vjp)(x["q"], x["qd"], x["ydd"], x["g"], want=names[1:])
    assert q.grad is None
    for leaf, k in zip((qd, last), names[1:]):
        assert torch.equal(leaf.grad.view(torch.int64), want[k].view(torch.int64)), k
