"""Body twists, spanning accelerations and contact Jacobians of the device against the numpy recursion of kinematics_ref.py (which
test_kinematics_ref_cpu.py pins to the oracle), every state on its own scale.

fp64: plan.body_twists and the second output of plan.spanning on the whole zoo and the two spanning-tree models, B = 1, 65 and 130 (one
state; one tile and one state; two tiles and a ragged third), v and a apart, per state, at 1e-9.

fp32: the error of every state on the block's own scale (no `1 +`) against what single precision itself costs on the same float32-rounded
inputs -- the float32 run of the same recursion -- times term_states.MARGIN (term_states.within_float: worst and median).  The inputs
are the draws of the other tests: velocities and accelerations in U(-1, 1), so that gravity and the velocity products are as large in a
as S qdd is.  MARGINS holds the cases the kernel misses at that margin, as test_term_parity_gpu.MARGINS does.

The J of inv_osim in fp32 and on the unit-wrench route (GRBDA_NO_EFPA=1) against kinematics_ref.frame_jacobians."""
import functools

import numpy as np
import pytest

import entry_points as EP
import kinematics_ref as K
import term_states as TS
from models import zoo

pytestmark = pytest.mark.gpu
BATCHES = (1, 65, 130)
B_TOP = BATCHES[-1]
SEED = 61
MODELS64 = list(zoo()) + ["parallel_chain_exp_d10_l16", "two_parent"]
# the models of test_gpu_parity.test_apply_test_force_matches_oracle
MODELS32 = ("urdf_mini_cheetah", "urdf_mit_humanoid", "tree_mixed_float", "tello_with_arms", "urdf_four_bar", "urdf_mini_cheetah_rpy", "chain_tree_a",
            "chain_tree_b", "urdf_jvrc1_humanoid", "rev_rotor_chain_4", "tree_rev_fixed")
BLOCKS = {"v": slice(0, 6), "a": slice(6, 12)}
# (model, block) that is not run in fp32, with the reason (test_kinematics_ref_cpu.py asserts that every other one leaves out at most
# term_states.MAX_LEFT_OUT of its batch)
NOT_RUN = {}
# (model, block): (margin = twice the measured worst ratio, measured (worst, median) ratio to the float32 recursion on the MI355X, cause).
# All four are the models with implicit clusters, and one cause: the float32 recursion takes G = -K_d^-1 K_i and g of those clusters
# rounded from the fp64 oracle, the kernel solves K_d in fp32 on the device, which costs cond(K_d) eps (the draws admit cond up to 3000,
# generalized_rbda_amd/states.py).  The medians are those of ordinary states; the four-bar's worst is one state next to its flat pose
# (5.1e-06 of |a|).  Every explicit model measured at most 2.3 (worst) and 2.2 (median); fp64 holds all of these at 1e-9.
_SOLVE = "G and g of the implicit clusters: solved in fp32 on the device, rounded from fp64 in the yardstick"
MARGINS = {
    ("tello_with_arms", "v"): (20.7, (10.34, 4.14), _SOLVE),
    ("tello_with_arms", "a"): (13.8, (6.86, 5.52), _SOLVE),
    ("urdf_four_bar", "v"): (27.4, (13.68, 3.03), _SOLVE),
    ("urdf_four_bar", "a"): (236.3, (118.15, 1.00), _SOLVE),
}


@functools.lru_cache(maxsize=None)
def draw(name, rounded):
    """(q, qd, ydd) of B_TOP states of `name`, read-only; rounded: to float32-representable values"""
    q, qd, ydd = EP._states(EP._model(name), B_TOP, SEED)
    return tuple(TS._frozen(TS.fp32_rounded(a) if rounded else a) for a in (q, qd, ydd))


@functools.lru_cache(maxsize=None)
def references32(name):
    """(fp64 recursion, float32 recursion as fp64) of the rounded draw: [B, n_bodies, 12] each, computed once per process"""
    blob = EP._model(name)
    q, qd, ydd = draw(name, True)
    return (TS._frozen(K.body_twists(blob, q, qd, ydd, big=EP._big(blob))),
            TS._frozen(K.body_twists(blob, q, qd, ydd, big=EP._big(blob), dtype=np.float32).astype(np.float64)))


def block(V, name):
    """one block of twists [B, n_bodies, 12], flattened over the bodies: [B, 6 n_bodies]"""
    return V[:, :, BLOCKS[name]].reshape(V.shape[0], -1)


@pytest.mark.parametrize("name", MODELS64)
def test_twists_and_spanning_accelerations_fp64(name, gpu):
    import torch

    blob, plan = EP._model(name), EP.plan_for(name, ())
    q, qd, ydd = draw(name, False)
    big = EP._big(blob)
    V_ref = K.body_twists(blob, q, qd, ydd, big=big)
    as_ref = K.spanning_rates(blob, q, qd, ydd, big=big)[1]
    g = as_ref - K.spanning_rates(blob, q, np.zeros_like(qd), ydd, big=big)[1]  # the bias of the implicit clusters
    t = lambda a, B: torch.as_tensor(np.ascontiguousarray(a[:B]), dtype=torch.float64, device=gpu)
    for B in BATCHES:
        V = plan.body_twists(t(q, B), t(qd, B), t(ydd, B)).cpu().numpy()
        err = K.block_errors(V, V_ref[:B])
        print(f"{name} B={B}: v {err[:, 0].max():.2e}  a {err[:, 1].max():.2e}")
        assert err.max() < EP.TOL64, (B, int(err.max(axis=1).argmax()), err.max(axis=0))
        a_span = plan.spanning(t(q, B), t(qd, B), t(ydd, B))[1].cpu().numpy()
        e = np.abs(a_span - as_ref[:B]).max(axis=1) / (1.0 + np.abs(g[:B]).max(axis=1))
        assert e.max() < 1e-8, (B, int(e.argmax()), e.max())


CASES32 = [(m, b) for m in MODELS32 for b in BLOCKS if (m, b) not in NOT_RUN]


@pytest.mark.parametrize("name,blk", CASES32, ids=[f"{m}-{b}" for m, b in CASES32])
def test_twists_fp32_within_the_float_recursion(name, blk, gpu):
    import torch

    plan = EP.plan_for(name, ())
    q, qd, ydd = draw(name, True)
    ref64, ref32 = references32(name)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)
    got = plan.body_twists(t(q), t(qd), t(ydd)).double().cpu().numpy()
    assert np.isfinite(got).all()
    worst, median = TS.float_ratio(block(got, blk), block(ref64, blk), block(ref32, blk))
    print(f"{name} {blk}: kernel error / float32 recursion error: worst {worst:.2f}, median {median:.2f}")
    margin = MARGINS.get((name, blk), (TS.MARGIN,))[0]
    TS.within_float(block(got, blk), block(ref64, blk), block(ref32, blk), margin, what=f"{name} {blk}")


def osim_frames(name):
    """the contact frames of test_gpu_parity.OSIM_CASES: (body indices, offsets)"""
    from test_gpu_parity import OSIM_CASES, _body_index

    bodies = [_body_index(EP._model(name), f) for f in dict(OSIM_CASES)[name]]
    return bodies, np.random.default_rng(4).uniform(-0.2, 0.2, size=(len(bodies), 3))


OSIM = [(m, env, dt) for m in ("urdf_mini_cheetah", "tello_with_arms") for env, dt in (((), "f32"), ((("GRBDA_NO_EFPA", "1"),), "f32"),
                                                                                      ((("GRBDA_NO_EFPA", "1"),), "f64"))]


@pytest.mark.parametrize("name,env,dt", OSIM, ids=[f"{m}-{'no_efpa' if env else 'efpa'}-{dt}" for m, env, dt in OSIM])
def test_contact_jacobians_fp32_and_on_the_unit_wrench_route(name, env, dt, gpu):
    import torch

    blob, plan = EP._model(name), EP.plan_for(name, env)
    B = 65
    dtype, tol = (torch.float32, EP.TOL32) if dt == "f32" else (torch.float64, EP.TOL64)
    q = draw(name, dt == "f32")[0][:B]
    bodies, offsets = osim_frames(name)
    J_ref = K.frame_jacobians(blob, q, bodies, offsets)
    _, J = plan.inv_osim(torch.as_tensor(np.ascontiguousarray(q), dtype=dtype, device=gpu), bodies, offsets, with_jacobian=True)
    J = J.double().cpu().numpy()
    per_state = np.abs(J - J_ref).reshape(B, -1).max(axis=1) / (1.0 + np.abs(J_ref).reshape(B, -1).max(axis=1))
    print(f"{name} {dt} {'GRBDA_NO_EFPA=1' if env else ''}: J error {per_state.max():.2e}")
    assert per_state.max() < tol, (int(per_state.argmax()), per_state.max())
