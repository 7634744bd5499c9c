"""tests/contact_step_ref.py, the reference of test_contact_step_gpu.py, held to the references it is built from -- no device call.

  * the all-ones mask gives contact_ref.contact_dynamics / impulse_ref.contact_impulse on the whole list, bit for bit (one group);
  * the zero mask gives oracle_py.forward_dynamics, an unchanged qd, and integrate_ref.reference_step on the free dynamics;
  * a plastic impact (e = 0) does not increase 1/2 qd^T H qd, and after it J_w qd+ is 0 on the active rows to 1e-9;
  * for cheetah_feet and tello_feet the contact matrix of every sub-list has a condition number no greater than the full set's -- eigenvalue
    interlacing for principal sub-matrices of an SPD matrix; asserted anyway, because the fp32 bound of the GPU test rests on it."""
import itertools

import numpy as np
import pytest

import contact_ref as C
import contact_step_ref as S
import entry_points as EP
import impulse_ref as IR
import integrate_ref as R
import oracle_py as O

B, SEED = 12, 67


def _case(key):
    model, bodies, offsets = C.contact_set(key)
    blob = EP._model(model)
    return (blob, list(bodies), [tuple(o) for o in offsets]) + tuple(EP._states(blob, B, SEED))


@pytest.mark.parametrize("key", ["cheetah_feet", "tello_feet"])
def test_the_full_mask_is_the_existing_references(key):
    blob, bodies, offsets, q, qd, tau = _case(key)
    n = len(bodies)
    rng = np.random.default_rng(SEED)
    want, full = rng.uniform(-1, 1, (B, n, 3)), np.full(B, (1 << n) - 1 | 1 << 20, dtype=np.int32)  # (a bit above n is ignored)
    got, ref = S.contact_dynamics_active(blob, q, qd, tau, bodies, offsets, full, want, 0.0, 0.0), C.contact_dynamics(blob, q, qd, tau, bodies, offsets, want)
    assert all(np.array_equal(got[k], ref[k]) for k in ("ydd", "lam", "ydd_free"))
    got, ref = S.contact_impulse_active(blob, q, qd, bodies, offsets, full, want, 0.5, 0.0), IR.contact_impulse(blob, q, qd, bodies, offsets, want, 0.5)
    assert all(np.array_equal(got[k], ref[k]) for k in ("qd_next", "impulse"))
    # kd enters as a_des - kd p_dot
    vel = C.contact_points(blob, q, bodies, offsets, qd)[1]
    got, ref = S.contact_dynamics_active(blob, q, qd, tau, bodies, offsets, full, want, 3.0, 0.0), C.contact_dynamics(blob, q, qd, tau, bodies, offsets, want - 3.0 * vel)
    assert np.array_equal(got["ydd"], ref["ydd"]) and np.abs(got["ydd"] - S.contact_dynamics_active(blob, q, qd, tau, bodies, offsets, full, want)["ydd"]).max() > 1e-3


@pytest.mark.parametrize("key", ["cheetah_feet", "tello_feet"])
def test_the_zero_mask_is_the_free_dynamics(key):
    blob, bodies, offsets, q, qd, tau = _case(key)
    zero, dt = np.zeros(B, dtype=np.int32), EP._dt(blob)
    free = O.forward_dynamics(blob, q, qd, tau, None, big=EP._big(blob))
    step = S.contact_step(blob, q, qd, tau, bodies, offsets, zero, np.full(B, 3, dtype=np.int32), 7.0, 0.5, 0.0, dt)
    assert np.array_equal(step["ydd"], free) and np.array_equal(step["ydd_free"], free) and not step["lam"].any() and not step["impulse"].any()
    assert np.array_equal(step["qd_plus"], qd)
    qn, vn, ok, _ = R.reference_step(blob, q, qd, free, dt, big=EP._big(blob))
    assert np.array_equal(step["q_next"], qn) and np.array_equal(step["qd_next"], vn) and np.array_equal(step["ok"], ok)


def test_a_mixed_schedule_is_zero_off_the_set_and_closes_with_every_closed_contact():
    blob, bodies, offsets, q, qd, tau = _case("cheetah_feet")
    n = len(bodies)
    active, prev = S.shuffled_masks(B, n, 0), S.shuffled_masks(B, n, 1)
    on = ((active[:, None] >> np.arange(n)[None]) & 1).astype(bool)
    out = S.contact_dynamics_active(blob, q, qd, tau, bodies, offsets, active)
    assert (out["lam"][~on] == 0).all() and (out["lam"][on] != 0).all()
    impact = S.impact_masks(active, prev, n)
    assert set(np.unique(impact)) <= set(np.unique(active)) | {0}
    assert all((impact[b] == active[b]) if active[b] & ~prev[b] else impact[b] == 0 for b in range(B))
    assert (impact != 0).any() and (impact == 0).any()


@pytest.mark.parametrize("key", ["cheetah_feet", "tello_feet"])
def test_a_plastic_impact_loses_energy_and_stops_the_active_points(key):
    blob, bodies, offsets, q, qd, tau = _case(key)
    n = len(bodies)
    active = S.shuffled_masks(B, n, 0)
    out = S.contact_impulse_active(blob, q, qd, bodies, offsets, active, None, 0.0, 0.0)
    H = EP._mass_oracle(IR.without_gravity(blob), q)
    before, after = IR.kinetic(H, qd), IR.kinetic(H, out["qd_next"])
    assert (after <= before * (1 + 1e-12)).all() and (after < before).any()
    v = np.einsum("bij,bj->bi", C.world_jacobian(blob, q, bodies, offsets), out["qd_next"]).reshape(B, n, 3)
    on = ((active[:, None] >> np.arange(n)[None]) & 1).astype(bool)
    assert on.any() and np.abs(v[on]).max() < 1e-9
    assert np.abs(v[~on]).max() > 1e-3  # (the open points keep moving)


@pytest.mark.parametrize("key", ["cheetah_feet", "tello_feet"])
def test_no_sub_list_is_worse_conditioned_than_the_full_set(key):
    blob, bodies, offsets, q, qd, tau = _case(key)
    n = len(bodies)
    A = IR.contact_impulse(blob, q, qd, bodies, offsets)["A"]
    full = np.linalg.cond(A)
    print(f"{key}: cond of the full set up to {full.max():.3g}")
    for k in range(1, n):
        for on in itertools.combinations(range(n), k):
            rows = [3 * c + i for c in on for i in range(3)]
            sub = np.linalg.cond(A[:, rows][:, :, rows])
            assert (sub <= full * (1 + 1e-9)).all(), on
