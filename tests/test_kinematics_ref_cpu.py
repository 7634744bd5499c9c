"""The numpy kinematics of kinematics_ref.py is pinned to the oracle, and the checkers built on it have teeth (no GPU).

Pins: the recursion's twists carried through f = I a + v x* I v, a backward sum and G^T are oracle_py.inverse_dynamics; its spanning
velocities are oracle_py.spanning_state's, its poses oracle_py.body_poses, its frame Jacobians the oracle's unit-wrench Jacobians.

Seeded defects, applied to a copy of the reference's own output: the v x S qd term dropped on one body, gravity's sign flipped, one
state's rows taken from the next state, the frame offset ignored in J, g dropped from qdd_span.  Each fails the checker of the entry-point
table at its fp64 bound.  The velocity-product term and gravity wrong by 1 % fail the fp32 per-state yardstick of test_kinematics_gpu.py
on that file's own inputs, and pass the check the fp32 twists had before -- max |V32 - V| / (1 + max |V|) < 1e-3 over the batch, on the
inputs of test_gpu_parity.test_body_twists_are_the_derivatives_of_the_motion: the gap the yardstick closes."""
import numpy as np
import pytest

import entry_points as EP
import kinematics_ref as K
import oracle_py as O
import term_states as TS
import test_kinematics_gpu as TK
from models import valid_states, zoo

PIN_MODELS = list(zoo()) + ["parallel_chain_exp_d10_l16", "two_parent"]
N_PIN = 16


def _pin_states(name):
    blob = EP._model(name)
    big = EP._big(blob)
    return blob, big, valid_states(blob, N_PIN, config_index=71, big=big, scale=0.5 if big else 1.0, max_cond=50 if big else None)


def test_batched_builders_restate_the_single_state_ones():
    rng = np.random.default_rng(0)
    th, rpy, quat, v, r = rng.uniform(-3, 3, 4), rng.uniform(-3, 3, (4, 3)), rng.uniform(-1, 1, (4, 4)), rng.uniform(-1, 1, (4, 6)), rng.uniform(-1, 1, (4, 3))
    for b in range(4):
        for axis in range(3):
            assert np.array_equal(K.rot_axis(axis, th)[b], K.coordinate_rotation(axis, th[b]))
        assert np.abs(K.rot_rpy(rpy)[b] - K.rpy_to_rotmat(rpy[b])).max() < 1e-15
        assert np.abs(K.rot_quat(quat)[b] - K.quat_to_rotmat(quat[b])).max() < 1e-15
        E = K.rpy_to_rotmat(rpy[b])
        assert np.abs(K.xmot_b(K.rot_rpy(rpy), r)[b] - K.Xmot(E, r[b])).max() < 1e-15
        assert np.array_equal(K.crm_b(v)[b], K.crm(v[b])) and np.array_equal(K.crf_b(v)[b], K.crf(v[b]))


@pytest.mark.parametrize("name", PIN_MODELS)
def test_the_recursion_is_pinned_to_the_oracle(name):
    """inverse dynamics at 1e-11 (1 + max |tau|); spanning velocities and poses at 1e-12"""
    blob, big, (q, qd, ydd) = _pin_states(name)
    V = K.body_twists(blob, q, qd, ydd, big=big)
    tau = K.rnea_from_twists(blob, q, V[:, :, :6], V[:, :, 6:], big=big)
    ref = O.inverse_dynamics(blob, q, qd, ydd, big=big)
    e_tau = np.abs(tau - ref).max()
    vs_ref = O.spanning_state(blob, q, qd, big=big)[1]
    e_span = np.abs(K.spanning_rates(blob, q, qd, ydd, big=big)[0] - vs_ref).max() / (1.0 + np.abs(vs_ref).max())
    e_pose = 0.0
    if not big:  # (the oracle's body_poses is built for the structured limits only)
        e_pose = np.abs(K.body_poses(blob, q) - O.body_poses(blob, q, V.shape[1])).max()
    print(f"{name}: |tau - oracle| {e_tau:.1e} at max |tau| {np.abs(ref).max():.1e}; spanning velocities {e_span:.1e}; poses {e_pose:.1e}")
    assert e_tau < 1e-11 * (1.0 + np.abs(ref).max())
    assert e_span < 1e-12 and e_pose < 1e-12


@pytest.mark.parametrize("name", ["urdf_mini_cheetah", "tello_with_arms", "tree_mixed_float", "urdf_mini_cheetah_rpy"])
def test_frame_jacobians_are_the_oracle_s_unit_wrench_jacobians(name):
    blob = EP._model(name)
    nb = K._parse(blob)["nb"]
    q, _, _ = valid_states(blob, 8, config_index=53)
    bodies, offsets = [nb - 1, nb // 2, 0], [[0.05, -0.02, 0.1], [0.0, 0.03, -0.2], [0.1, 0.2, -0.3]]
    J, J_ref = K.frame_jacobians(blob, q, bodies, offsets), K.oracle_frame_jacobians(blob, q, bodies, offsets)
    err = np.abs(J - J_ref).max() / np.abs(J_ref).max()
    print(f"{name}: J against the unit-wrench Jacobians {err:.1e}")
    assert err < 1e-10


def test_the_float32_recursion_leaves_out_no_more_than_the_cap():
    """of every (model, block) the fp32 GPU test runs; and it is a yardstick: its own error is not zero"""
    for name, blk in TK.CASES32:
        ref64, ref32 = TK.references32(name)
        ref, fl = TK.block(ref64, blk), TK.block(ref32, blk)
        assert TS.left_out(ref) <= TS.MAX_LEFT_OUT, (name, blk, TS.left_out(ref))
        assert 0 < TS.term_error(fl, ref).max() < 1e-5, (name, blk)
        TS.within_float(TS.fp32_rounded(ref), ref, fl, what=f"{name} {blk}: the reference rounded to fp32")
    assert set(TK.MARGINS) <= set(TK.CASES32) and not set(TK.NOT_RUN) & set(TK.CASES32)
    assert all(margin > TS.MARGIN and abs(margin - 2 * worst) < 0.1 for margin, (worst, _), _ in TK.MARGINS.values())


# ---- seeded defects ------------------------------------------------------------------------------------------------------------------
def _refused(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _product_body(blob, q, qd, ydd):
    """the body whose velocity-product term is the largest of the model (median over the states), and the term [B, 6]"""
    kin = K._Kin(blob, q)
    vs, as_ = kin.rates(qd, ydd)
    v, _ = kin.propagate(vs, as_)
    terms = [K._mv(K.crm_b(v[:, b]), kin.joint_rate(b, vs)) for b in range(kin.m["nb"])]
    b = int(np.argmax([np.median(np.abs(t).max(axis=1)) for t in terms]))
    return b, terms[b]


def twist_defects(blob, q, qd, ydd, V, part):
    """copies of the twists V with `part` of the v x S qd term of one body taken out / `part` of gravity taken out of every body"""
    b, term = _product_body(blob, q, qd, ydd)
    product = V.copy()
    product[:, b, 6:] -= part * term
    E = K.body_poses(blob, q)[:, :, :9].reshape(V.shape[0], V.shape[1], 3, 3)
    gravity = V.copy()
    gravity[:, :, 9:] -= part * np.einsum("bnij,j->bni", E, -K._parse(blob)["grav"][3:])
    return {"velocity product": product, "gravity": gravity}


def _table_states(name, B=6, seed=5):
    import torch

    blob = EP._model(name)
    return blob, EP._host_inputs(blob, K._parse(blob)["nb"], B, seed, torch.float64)


@pytest.mark.parametrize("name", ["urdf_mini_cheetah", "tello_with_arms", "urdf_mini_cheetah_rpy"])
def test_the_twist_checker_refuses_the_seeded_defects(name):
    blob, s = _table_states(name)
    check = EP.ENTRY["body_twists"][1]
    V = K.body_twists(blob, s["q"], s["qd"], s["tau"])
    check(blob, s, [V], EP.TOL64)
    bad = twist_defects(blob, s["q"], s["qd"], s["tau"], V, 1.0)      # the term dropped
    bad["gravity"] = twist_defects(blob, s["q"], s["qd"], s["tau"], V, 2.0)["gravity"]  # the sign flipped
    shifted = V.copy()
    shifted[2] = V[3]
    bad["a state's rows from the next state"] = shifted
    for what, W in bad.items():
        assert _refused(check, blob, s, [W], EP.TOL64), what
        assert _refused(check, blob, s, [W], EP.TOL32), what + " (at the fp32 tolerance)"


def test_the_spanning_checker_refuses_a_dropped_bias():
    blob, s = _table_states("tello_with_arms")
    vs, as_ = K.spanning_rates(blob, s["q"], s["qd"], s["tau"])
    EP._chk_spanning(blob, s, [vs, as_], EP.TOL64)
    no_g = K.spanning_rates(blob, s["q"], np.zeros_like(s["qd"]), s["tau"])[1]
    assert np.abs(as_ - no_g).max() > 1.0  # (there is a bias to drop)
    assert _refused(EP._chk_spanning, blob, s, [vs, no_g], EP.TOL64)
    assert _refused(EP._chk_spanning, blob, s, [vs, no_g], EP.TOL32)
    shifted = as_.copy()
    shifted[2] = as_[3]
    assert _refused(EP._chk_spanning, blob, s, [vs, shifted], EP.TOL64)


def test_the_osim_checker_refuses_a_jacobian_the_identity_accepts():
    """Linv built from the defective J itself, as a kernel that misplaces the frame would: the identity Linv = J H^-1 J^T holds"""
    blob, s = _table_states("urdf_mini_cheetah")
    bodies, offsets = EP._osim_frames(blob)
    Hinv = EP._fd_columns(blob, s["q"], np.zeros_like(s["qd"]), np.zeros_like(s["qd"]), "dtau")
    linv = lambda J: np.einsum("bij,bjk,blk->bil", J, Hinv, J)
    J = K.frame_jacobians(blob, s["q"], bodies, offsets)
    EP._chk_osim(blob, s, [linv(J), J], EP.TOL64)
    bad = {"the offset ignored": K.frame_jacobians(blob, s["q"], bodies, np.zeros((2, 3))),
           "the frame on the parent body": K.frame_jacobians(blob, s["q"], [K._parse(blob)["bodies"][bodies[0]]["parent"], bodies[1]], offsets)}
    for what, Jb in bad.items():
        assert np.abs(Jb - J).max() > 1e-2
        assert _refused(EP._chk_osim, blob, s, [linv(Jb), Jb], EP.TOL64), what
        assert _refused(EP._chk_osim, blob, s, [linv(Jb), Jb], EP.TOL32), what + " (at the fp32 tolerance)"


@pytest.mark.parametrize("name", TK.MODELS32)
def test_one_per_cent_defects_fail_the_fp32_yardstick(name):
    """on the inputs of the GPU test, at the margin of the GPU test (MARGINS included)"""
    blob = EP._model(name)
    q, qd, ydd = TK.draw(name, True)
    ref64, ref32 = TK.references32(name)
    ref, fl = TK.block(ref64, "a"), TK.block(ref32, "a")
    margin = TK.MARGINS.get((name, "a"), (TS.MARGIN,))[0]
    for what, W in twist_defects(blob, q, qd, ydd, ref64, 0.01).items():
        if what == "gravity" and not np.abs(ref64 - twist_defects(blob, q, qd, ydd, ref64, 1.0)["gravity"]).max() > 0:
            continue
        assert not TS.passes_float(TS.fp32_rounded(TK.block(W, "a")), ref, fl, margin), (what, margin)


@pytest.mark.parametrize("name", ["urdf_mini_cheetah", "urdf_mit_humanoid", "tello_with_arms"])
def test_the_batch_wide_metric_accepts_the_one_per_cent_defects(name):
    """The gap on record: on the inputs of test_body_twists_are_the_derivatives_of_the_motion (accelerations of the forward dynamics,
    max |a| in the hundreds) 1 % of one body's velocity product or of gravity is below 1e-3 of 1 + max |V|; the per-state yardstick
    refuses both on the same inputs."""
    blob = EP._model(name)
    q, qd, tau = (TS.fp32_rounded(a) for a in valid_states(blob, 5, config_index=57))
    ydd = TS.fp32_rounded(O.forward_dynamics(blob, q, qd, tau))
    V = K.body_twists(blob, q, qd, ydd)
    fl = K.body_twists(blob, q, qd, ydd, dtype=np.float32).astype(np.float64)
    for what, W in twist_defects(blob, q, qd, ydd, V, 0.01).items():
        W = TS.fp32_rounded(W)
        assert np.abs(W - V).max() / (1.0 + np.abs(V).max()) < EP.TOL32, what
        assert not TS.passes_float(TK.block(W, "a"), TK.block(V, "a"), TK.block(fl, "a")), what
