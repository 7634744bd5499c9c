"""tests/wrench_ref.py against the oracle, without a device: the power identity.  With yd set and ydd = 0, the inverse dynamics with and
without external forces differ by J^T f, so  (tau(no force) - tau(force)) . yd = sum over the listed bodies of wrench . twist -- the
wrench and the twist of a body in ONE frame, either frame.  The twists come from kinematics_ref (pinned to the oracle by its own test)
and never pass through the force transform under test.  Bound 1e-10; each seeded defect of the transform must move it beyond 1e-3."""
import numpy as np
import pytest

import kinematics_ref as K
import oracle_py as O
import wrench_ref as W
from models import chain_test_tree, valid_states, zoo

BOUND, SEEN = 1e-10, 1e-3


def _blob(name):
    return chain_test_tree(31).serialize() if name == "chain_test_tree_31" else zoo()[name]


def _case(name, frame):
    blob = _blob(name)
    q, qd, _ = valid_states(blob, 6, config_index=41)
    nb = K.body_poses(blob, q).shape[1]
    rng = np.random.default_rng(3)
    bodies = [0, nb - 1, nb // 2, nb // 3, nb - 1]  # (the last body twice)
    wrench = rng.uniform(-1, 1, (q.shape[0], len(bodies), 6))
    twists = (K.body_twists(blob, q, qd, np.zeros_like(qd))[:, :, :6] if frame == "body" else W.world_twists(blob, q, qd))
    power = sum(np.einsum("bi,bi->b", wrench[:, i], twists[:, b]) for i, b in enumerate(bodies))
    return blob, q, qd, bodies, wrench, power


def _identity_error(blob, q, qd, f_ext, power):
    z = np.zeros_like(qd)
    got = np.einsum("bi,bi->b", O.inverse_dynamics(blob, q, qd, z) - O.inverse_dynamics(blob, q, qd, z, f_ext), qd)
    return np.abs(got - power).max() / (1 + np.abs(power).max())


@pytest.mark.parametrize("frame", ["body", "world"])
@pytest.mark.parametrize("name", ["chain_test_tree_31", "urdf_mit_humanoid", "rev_pair_rotor_chain_4", "tello_with_arms"])
def test_the_dense_forces_satisfy_the_power_identity(name, frame):
    blob, q, qd, bodies, wrench, power = _case(name, frame)
    assert np.abs(power).max() > 1e-2
    assert _identity_error(blob, q, qd, W.dense_f_ext(blob, q, bodies, wrench, frame), power) < BOUND


@pytest.mark.parametrize("defect", W.DEFECTS)
def test_a_seeded_defect_breaks_the_identity(defect):
    blob, q, qd, bodies, wrench, power = _case("chain_test_tree_31", "body")
    assert _identity_error(blob, q, qd, W.dense_f_ext(blob, q, bodies, wrench, "body", defect=defect), power) > SEEN


def test_world_frame_is_a_scatter_and_duplicates_add():
    blob, q, _, bodies, wrench, _ = _case("chain_test_tree_31", "world")
    f = W.dense_f_ext(blob, q, bodies, wrench, "world")
    assert np.array_equal(f[:, bodies[0]], wrench[:, 0])
    assert np.array_equal(f[:, bodies[1]], wrench[:, 1] + wrench[:, 4])
    assert np.count_nonzero(np.abs(f).sum(axis=(0, 2))) == len(set(bodies))


def test_the_places_of_a_chain_tree():
    p = W.tree_places(chain_test_tree(31).serialize())
    assert p["base"] == 0 and p["pairs"] and p["rotors"] and p["mid"] and p["tips"] and p["forks"]
    assert not set(p["links"]) & set(p["rotors"])
