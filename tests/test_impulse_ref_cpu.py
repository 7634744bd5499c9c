"""tests/impulse_ref.py pinned on the CPU, before any device result is compared with it (test_impulse_gpu.py, test_impulse_solve_gpu.py).

On 16 states each (entry_points._states, seed 73) of: Mini Cheetah with a foot on each knee link, TelloWithArms with both feet, and a
fixed-base chain of revolute pairs (rev_pair_chain_4) with one point on its last link (all three with independent contacts: mu = 0 is well-posed):
  (a) J_w qd_next = v_des - e v- - mu Lambda, to 1e-10, for (e, mu) in (0, 0), (0.5, 0), (0.3, 1e-3), v_des in U(-1, 1);
  (b) e = 0, mu = 0, v_des = 0: the kinetic energy 1/2 qd^T H qd drops by exactly 1/2 v-^T A^-1 v-;
  (c) e = 1, mu = 0, v_des = 0: the kinetic energy is unchanged;
  (d) qd_next - qd = FD(q, 0, 0, wrenches(Lambda)) - FD(q, 0, 0, none) of the oracle: the wrench convention is the oracle's f_ext;
  (e) v- = 0 and v_des = 0 give Lambda = 0.
Then every case of the GPU tests (impulse_ref.CASES, 130 states each): cond(A) is finite and the reference is finite in every state, so
the GPU tests leave out no state.  Measured here: cond(A) <= 3.5e4 over all cases (asserted below 1e5, as test_contact_ref_cpu.py does)."""
import functools

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import impulse_ref as I
import oracle_py as O

B = 16
SETS = ["cheetah_feet", "tello_feet", "rev_pair_chain_4"]


@functools.lru_cache(maxsize=None)
def inputs(key):
    if key in C.SETS:
        model, bodies, offsets = C.contact_set(key)
    else:
        from test_contact_gpu import points_of

        model, (bodies, offsets) = key, points_of(key)
    blob = EP._model(model)
    q, qd, _ = EP._states(blob, B, I.SEED)
    v_des = np.random.default_rng(I.SEED).uniform(-1, 1, (B, len(bodies), 3))
    return blob, list(bodies), offsets, q, qd, v_des


@pytest.mark.parametrize("e,mu", [(0.0, 0.0), (0.5, 0.0), (0.3, 1e-3)])
@pytest.mark.parametrize("key", SETS)
def test_the_points_leave_with_the_velocity_asked_for(key, e, mu):
    blob, bodies, offsets, q, qd, v_des = inputs(key)
    s = I.contact_impulse(blob, q, qd, bodies, offsets, v_des, e, mu)
    assert C.rel_per_state(s["v_minus"], C.contact_points(blob, q, bodies, offsets, qd)[1]).max() < 1e-12
    after = np.einsum("bij,bj->bi", s["Jw"], s["qd_next"]).reshape(B, len(bodies), 3)
    err = C.rel_per_state(after, v_des - e * s["v_minus"] - mu * s["impulse"]).max()
    print(f"{key} e={e} mu={mu}: J_w qd_next against v_des - e v- - mu Lambda {err:.2e}, cond(A) <= {np.linalg.cond(s['A']).max():.2e}")
    assert err < 1e-10


@pytest.mark.parametrize("key", SETS)
def test_plastic_impact_loses_the_energy_of_the_contact_velocities(key):
    blob, bodies, offsets, q, qd, _ = inputs(key)
    s = I.contact_impulse(blob, q, qd, bodies, offsets)
    v = s["v_minus"].reshape(B, -1)
    drop = 0.5 * np.einsum("bi,bi->b", v, np.linalg.solve(s["A"], v[:, :, None])[:, :, 0])
    before, after = I.kinetic(s["H"], qd), I.kinetic(s["H"], s["qd_next"])
    err = np.abs(before - after - drop) / (1 + before)
    print(f"{key}: energy drop against 1/2 v-^T A^-1 v- {err.max():.2e}")
    assert (drop > 0).all() and err.max() < 1e-10


@pytest.mark.parametrize("key", SETS)
def test_elastic_impact_keeps_the_energy(key):
    blob, bodies, offsets, q, qd, _ = inputs(key)
    s = I.contact_impulse(blob, q, qd, bodies, offsets, None, 1.0, 0.0)
    before, after = I.kinetic(s["H"], qd), I.kinetic(s["H"], s["qd_next"])
    err = np.abs(before - after) / (1 + before)
    print(f"{key}: e = 1 energy change {err.max():.2e}")
    assert err.max() < 1e-10


@pytest.mark.parametrize("key", SETS)
def test_velocity_change_is_the_oracles_forward_dynamics_of_the_impulse_wrenches(key):
    blob, bodies, offsets, q, qd, v_des = inputs(key)
    s = I.contact_impulse(blob, q, qd, bodies, offsets, v_des, 0.5, 0.0)
    z = np.zeros_like(qd)
    w = C.wrenches(blob, q, bodies, offsets, s["impulse"])
    delta = O.forward_dynamics(blob, q, z, z, w, big=EP._big(blob)) - O.forward_dynamics(blob, q, z, z, None, big=EP._big(blob))
    err = C.rel_per_state(s["qd_next"] - qd, delta).max()
    print(f"{key}: qd_next - qd against FD(wrenches) - FD(none) {err:.2e}")
    assert err < 1e-8


@pytest.mark.parametrize("key", SETS)
def test_points_at_rest_take_no_impulse(key):
    blob, bodies, offsets, q, qd, _ = inputs(key)
    s = I.contact_impulse(blob, q, np.zeros_like(qd), bodies, offsets)
    assert (s["impulse"] == 0).all() and (s["qd_next"] == 0).all()


@pytest.mark.parametrize("cid", [c[0] for c in I.CASES])
def test_every_state_of_the_gpu_cases_has_a_reference(cid):
    for rounded in (False, True):
        ref = I.case(cid, rounded)[-1]
        cond = np.linalg.cond(ref["A"])
        print(f"{cid}{' rounded' if rounded else ''}: cond(A) <= {cond.max():.2e}")
        assert np.isfinite(cond).all() and cond.max() < 1e5
        assert np.isfinite(ref["qd_next"]).all() and np.isfinite(ref["impulse"]).all()
        assert np.linalg.eigvalsh(ref["A"]).min() > 0
