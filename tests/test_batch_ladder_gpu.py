"""Tiny, ragged and boundary batches of every device entry point against the oracle, and the independence of a state's result from
the states that share its tile or its group.

Tile ladder: B in 1, 2, 63, 64, 65, 127, 128, 129, 257 (a tile is 64 states), for what the older ladders leave out -- forward / inverse
dynamics in fp32, and in both types with f_ext (which sends forward dynamics to the interpreter), on the chain kernels and latency mode
(Mini Cheetah, MIT humanoid), differential segments (TelloWithArms), the single-cluster kernel (four-bar), the interpreter (MIT humanoid,
GRBDA_NO_CHAIN=1) and the spanning-tree route (parallel chain); and every other row of the entry-point table (entry_points.py) on that
row's own model -- the inverse-dynamics derivatives, integrate / step / rollout, contact points and contact dynamics, energy, the
centroidal quantities and the momentum matrix among them.  Group ladder: the derivative pipeline packs four states into one workgroup's
MFMA tiles and pads H with the identity, so fd_derivatives, fd_dtau and mass_matrix also run B in 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65 on
the minv route, the dense route (GRBDA_NO_MINV=1), the fp64 solve of fp32 batches (GRBDA_SOLVE_F64=1) and the manifold route (Tello), and
id_derivatives on its analytic route (Mini Cheetah).

The inputs of batch B are the first B rows of one draw of the ladder's largest batch, placed in guarded buffers (guarded.py): behind row
B - 1 lies a band of NaN, not the next valid state, and every output sits between canary bands (run_guarded asserts bounds, complete
writes, untouched inputs and finite outputs).  Every state of every batch is held against the oracle with the table's checker at the
table's tolerances; only the position derivatives (of the forward and of the inverse dynamics), whose oracle is taken state by state, are held on a sample
above 65 states (first, last, both ends of the last tile and of the last group, a seeded few).  Body twists, spanning accelerations and the
inverse OSIM's Jacobians are held to the numpy recursion of kinematics_ref.py, which the CPU suite pins to the oracle.  The draws of
those derivative rows bound the conditioning of the implicit loops as the older derivative tests do (entry_points.py, draw_bound).

Prefix invariance: where B and the ladder's largest batch launch the same kernels -- the same plan.kernel_name for forward / inverse
dynamics, the same number of kernel nodes in a captured call for the rest -- the B rows are bit-identical to the first B rows of the
largest batch's result.

Second route threshold: at most 4 n_cu tiles run the two-wavefront latency kernel, one state more the chain kernel, whose last tile then
holds ONE state.  B = 256 n_cu and 256 n_cu + 1 for the models with latency mode, the kernel names asserted, against the oracle on
the tile edges, the single last state and 4096 seeded states."""
import functools

import numpy as np
import pytest

from entry_points import CASES, DIFFERENTIATES, ENTRY, TILE, TOL32, TOL64, TYPED, _host, _host_inputs, _model, draw_bound, edge_states, plan_for, run_guarded, same_bits_np
from generalized_rbda_amd.states import parse_clusters
from graph_capture import capture

pytestmark = pytest.mark.gpu

TILES = [1, 2, 63, 64, 65, 127, 128, 129, 257]
GROUPS = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65]
SEED = 21
SAMPLED_ABOVE = 65  # entry points whose oracle is taken state by state: all states up to here, edge_states() beyond
SAMPLED = DIFFERENTIATES

DYNAMICS_MODELS = [("urdf_mini_cheetah", {}), ("urdf_mit_humanoid", {}), ("tello_with_arms", {}), ("urdf_four_bar", {}),
                   ("urdf_mit_humanoid", {"GRBDA_NO_CHAIN": "1"}), ("parallel_chain_exp_d10_l16", {})]
# (fp64 forward / inverse dynamics without f_ext: test_gpu_parity.py runs 1, 63, 64, 200 on the whole zoo)
DYNAMICS = [(m, e, ep, dt) for m, e in DYNAMICS_MODELS for ep, dts in (("aba", ("f32",)), ("rnea", ("f32",)), ("aba_fext", ("f32", "f64")),
                                                                       ("rnea_fext", ("f32", "f64"))) for dt in dts]
OTHERS = [(c[1], c[2], c[4], dt) for c in CASES if c[4] not in ("aba", "rnea", "aba_fext", "rnea_fext") for dt in ("f32", "f64") if (c, dt) in TYPED]
DERIV_ROUTES = [("minv", "urdf_mini_cheetah", {}, ("f32", "f64")), ("dense", "urdf_mini_cheetah", {"GRBDA_NO_MINV": "1"}, ("f32", "f64")),
                ("solve_f64", "urdf_mini_cheetah", {"GRBDA_SOLVE_F64": "1"}, ("f32",)), ("manifold", "tello", {}, ("f32", "f64"))]
DERIVS = [(model, env, ep, dt) for route, model, env, dts in DERIV_ROUTES for ep in ("fd_derivatives", "fd_dtau", "mass_matrix") for dt in dts]
# the inverse-dynamics derivatives pack groups of four on their analytic route (Mini Cheetah)
DERIVS += [("urdf_mini_cheetah", {}, "id_derivatives", dt) for dt in ("f32", "f64")]


def _id(case):
    model, env, ep, dt = case
    return "-".join([ep, model] + [k.replace("GRBDA_", "").lower() for k in sorted(env)] + [dt])


def _dtype(name):
    import torch

    return torch.float64 if name == "f64" else torch.float32


def _device_inputs(s, dtype, gpu):
    import torch

    x = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=dtype, device=gpu) for k, v in s.items()}
    x["q_proj"] = x["q_start"].clone()
    return x


@functools.lru_cache(maxsize=None)
def _launches(model, env, ep, dt, B, top, gpu):
    """what tells two batch sizes' launch sequences apart: the kernel's name where the library gives one, else the kernel nodes of a
    captured call"""
    plan = plan_for(model, env)
    if ep in ("aba", "rnea"):
        return plan.kernel_name(ep, dt, B)
    s = {k: v[:B] for k, v in _host_inputs(_model(model), plan.n_bodies, top, SEED, _dtype(dt), draw_bound(ep)).items()}
    x = _device_inputs(s, _dtype(dt), gpu)
    cap = capture(lambda: ENTRY[ep][0](plan, x))
    try:
        return cap.nodes["kernel"]
    finally:
        cap.drop()


@functools.lru_cache(maxsize=None)
def _result(model, env, ep, dt, B, top, gpu):
    """the outputs of the first B rows of the `top`-row draw, through guarded buffers, and those rows"""
    plan = plan_for(model, env)
    s = {k: v[:B] for k, v in _host_inputs(_model(model), plan.n_bodies, top, SEED, _dtype(dt), draw_bound(ep)).items()}
    return s, run_guarded(plan, ENTRY[ep][0], s, _dtype(dt), gpu, 0)


def _ladder_case(case, B, top, gpu):
    model, env, ep, dt = case
    env = tuple(sorted(env.items()))
    blob, check, tol = _model(model), ENTRY[ep][1], TOL64 if dt == "f64" else TOL32
    s, got = _result(model, env, ep, dt, B, top, gpu)
    assert all(len(o) == B for o in got)
    if check is not None:
        idx = edge_states(B, seed=B) if (ep in SAMPLED and B > SAMPLED_ABOVE) else np.arange(B)
        check(blob, {k: v[idx] for k, v in s.items()}, [o[idx] for o in got], tol)
    if B < top and _launches(model, env, ep, dt, B, top, gpu) == _launches(model, env, ep, dt, top, top, gpu):
        whole = _result(model, env, ep, dt, top, top, gpu)[1]
        for i, (a, b) in enumerate(zip(got, whole)):
            same = np.array([np.array_equal(a[j], b[j], equal_nan=True) for j in range(B)])
            assert same.all(), f"output {i}: states {np.flatnonzero(~same)[:8]} of {B} differ from the same states in a batch of {top}"


@pytest.mark.parametrize("B", TILES)
@pytest.mark.parametrize("case", DYNAMICS, ids=_id)
def test_tile_ladder_dynamics(case, B, gpu):
    _ladder_case(case, B, TILES[-1], gpu)


@pytest.mark.parametrize("B", TILES)
@pytest.mark.parametrize("case", OTHERS, ids=_id)
def test_tile_ladder_entry_points(case, B, gpu):
    _ladder_case(case, B, TILES[-1], gpu)


@pytest.mark.parametrize("B", GROUPS)
@pytest.mark.parametrize("case", DERIVS, ids=_id)
def test_group_ladder_derivatives(case, B, gpu):
    _ladder_case(case, B, GROUPS[-1], gpu)


def test_the_ladders_cross_their_routes(gpu):
    """What the ladders claim to run: latency mode and the chain / interpreter / single-cluster kernels by name."""
    name = lambda model, env, ep, dt, B: plan_for(model, tuple(sorted(env.items()))).kernel_name(ep, dt, B)
    for ep in ("aba", "rnea"):
        assert "_chain_lm_kernel<" in name("urdf_mini_cheetah", {}, ep, "f32", 65)
        assert "_chain_lm_kernel<" in name("tello_with_arms", {}, ep, "f32", 257)
        assert "_gen1_kernel<" in name("urdf_four_bar", {}, ep, "f32", 65)
        assert f"{ep}_kernel<" in name("urdf_mit_humanoid", {"GRBDA_NO_CHAIN": "1"}, ep, "f32", 65)
    assert plan_for("parallel_chain_exp_d10_l16", ()).info().spanning_tree_route == 1


# ---- the second route threshold --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("ep", ["aba", "rnea"])
@pytest.mark.parametrize("model", ["urdf_mini_cheetah", "urdf_mit_humanoid", "tello_with_arms"])
def test_second_route_threshold(model, ep, dt, gpu):
    """n_tiles <= 4 n_cu: the two-wavefront latency kernel; one state more: the chain kernel with a single state in its last tile.
    What the model can run is read from the kernel names at 64 and 2^20 states: a model without the latency-mode program of this type
    and direction (TelloWithArms in fp64, the MIT humanoid's fp64 inverse dynamics) runs one kernel on both sides, still against the
    oracle."""
    import torch

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    edge = TILE * 4 * n_cu
    plan, blob = plan_for(model, ()), _model(model)
    info = plan.info()
    small, far = plan.kernel_name(ep, dt, TILE), plan.kernel_name(ep, dt, 1 << 20)
    below, above = plan.kernel_name(ep, dt, edge), plan.kernel_name(ep, dt, edge + 1)
    if ep == "aba":
        assert ("_lm_kernel<" in small) == bool(info.latency_mode_f32 if dt == "f32" else info.latency_mode_f64), small
    if "_lm_kernel<" in small and "_chain_kernel<" in far:
        assert "_lm_kernel<" in below and ", 2" in below, below  # two wavefronts
        assert "_chain_kernel<" in above and "_lm_kernel<" not in above and above == far, above
    else:
        assert below == above == far
    dtype, tol = _dtype(dt), TOL64 if dt == "f64" else TOL32
    if any(c[9] >= 2 for c in parse_clusters(blob)["clusters"]):
        # implicit loops: states on the manifold cost a Newton projection each on the CPU -- 4096 of them, repeated (64 distinct per tile)
        base = _host_inputs(blob, plan.n_bodies, 4096, SEED, dtype)
        s_top = {k: v[np.arange(edge + 1) % 4096] for k, v in base.items()}
    else:
        s_top = _host_inputs(blob, plan.n_bodies, edge + 1, SEED, dtype)
    for B in (edge, edge + 1):
        s = {k: v[:B] for k, v in s_top.items()}
        got = run_guarded(plan, ENTRY[ep][0], s, dtype, gpu, 0, out_arena=ep)
        idx = np.union1d(edge_states(B, 4096, seed=B), [TILE - 1, TILE, edge - TILE, edge - 1])
        ENTRY[ep][1](blob, {k: v[idx] for k, v in s.items()}, [o[idx] for o in got], tol)
        last = np.array([B - 1])  # the single state of the last tile, on its own scale
        ENTRY[ep][1](blob, {k: v[last] for k, v in s.items()}, [o[last] for o in got], tol)
