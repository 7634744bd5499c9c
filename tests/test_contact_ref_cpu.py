"""tests/contact_ref.py against the oracle, on the CPU: the numpy reference of the contact entry points is held to
oracle_py.forward_dynamics / body_poses before any device result is compared with it (test_contact_gpu.py).

On 16 states each (entry_points._states, seed 61) of: Mini Cheetah with a foot on each knee link, TelloWithArms with both feet, MIT
Humanoid with four corners per sole (8 contacts of rank 12: damping 1e-3).
  (a) ydd by the closed form ydd_free + H^-1 J_w^T lambda equals the oracle's forward dynamics with the wrenches of lambda, to 1e-8;
  (b) p_ddot(ydd) + mu lambda = a_des, a_des in U(-1, 1), to 1e-8;
  (c) p_dot = J_w qd and p_ddot(ydd + d) - p_ddot(ydd) = J_w d, to 1e-12;
  (d) pos = r + E^T o of oracle_py.body_poses.
Measured here: cond(A + mu I) of the 8-contact set at mu = 1e-3 is at most 9.2e3 (asserted below 1e5)."""
import functools

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import oracle_py as O

B, SEED = 16, 61
CASES = [("cheetah_feet", 0.0), ("tello_feet", 0.0), ("humanoid_soles", 1e-3)]


@functools.lru_cache(maxsize=None)
def solved(key, mu):
    model, bodies, offsets = C.contact_set(key)
    blob = EP._model(model)
    q, qd, tau = EP._states(blob, B, SEED)
    a_des = np.random.default_rng(SEED).uniform(-1, 1, (B, len(bodies), 3))
    return blob, bodies, offsets, q, qd, tau, a_des, C.contact_dynamics(blob, q, qd, tau, bodies, offsets, a_des, mu)


@pytest.mark.parametrize("key,mu", CASES, ids=[c[0] for c in CASES])
def test_closed_form_equals_forward_dynamics_with_the_contact_wrenches(key, mu):
    blob, bodies, offsets, q, qd, tau, a_des, s = solved(key, mu)
    cond = np.linalg.cond(s["A"])
    print(f"{key}: cond(A + mu I) <= {cond.max():.2e}")
    if key == "humanoid_soles":
        assert cond.max() < 1e5
    ydd = O.forward_dynamics(blob, q, qd, tau, C.wrenches(blob, q, bodies, offsets, s["lam"]), big=EP._big(blob))
    err = C.rel_per_state(s["ydd"], ydd).max()
    print(f"{key}: closed form against the oracle with wrenches {err:.2e}")
    assert err < 1e-8


@pytest.mark.parametrize("key,mu", CASES, ids=[c[0] for c in CASES])
def test_the_constraint_holds_at_the_constrained_accelerations(key, mu):
    blob, bodies, offsets, q, qd, tau, a_des, s = solved(key, mu)
    acc = C.contact_points(blob, q, bodies, offsets, qd, s["ydd"])[2]
    err = C.rel_per_state(acc + mu * s["lam"], a_des).max()
    print(f"{key}: p_ddot(ydd) + mu lambda against a_des {err:.2e}")
    assert err < 1e-8


@pytest.mark.parametrize("key,mu", CASES, ids=[c[0] for c in CASES])
def test_velocity_is_the_jacobian_and_acceleration_is_linear_in_ydd(key, mu):
    blob, bodies, offsets, q, qd, tau, a_des, s = solved(key, mu)
    n = len(bodies)
    _, vel, acc = C.contact_points(blob, q, bodies, offsets, qd, s["ydd"])
    assert C.rel_per_state(vel, np.einsum("bij,bj->bi", s["Jw"], qd).reshape(B, n, 3)).max() < 1e-12
    d = np.random.default_rng(SEED + 1).uniform(-1, 1, qd.shape)
    step = C.contact_points(blob, q, bodies, offsets, qd, s["ydd"] + d)[2] - acc
    assert C.rel_per_state(step, np.einsum("bij,bj->bi", s["Jw"], d).reshape(B, n, 3)).max() < 1e-12


@pytest.mark.parametrize("key,mu", CASES, ids=[c[0] for c in CASES])
def test_positions_against_the_oracle_poses(key, mu):
    blob, bodies, offsets, q = solved(key, mu)[:4]
    Xa = O.body_poses(blob, q, EP.K._parse(blob)["nb"])[:, bodies]
    E, r = Xa[:, :, :9].reshape(B, len(bodies), 3, 3), Xa[:, :, 9:]
    ref = r + np.einsum("bcji,cj->bci", E, np.asarray(offsets))
    assert C.rel_per_state(C.contact_points(blob, q, bodies, offsets)[0], ref).max() < 1e-12


def test_singular_without_damping():
    """the 8-contact set has rank 12 of 24: what the damping is for"""
    blob, bodies, offsets, q = solved("humanoid_soles", 1e-3)[:4]
    s = solved("humanoid_soles", 1e-3)[-1]
    A0 = s["A"] - 1e-3 * np.eye(24)[None]
    assert (np.linalg.matrix_rank(A0, tol=1e-9) == 12).all()
