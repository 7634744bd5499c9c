"""tests/contact_ref.py and tests/impulse_ref.py away from the native gravity, on the CPU.  Every model of the zoo is built at
(0, 0, -9.81), so the tests that pin the two references (test_contact_ref_cpu.py, test_impulse_ref_cpu.py) multiply g[0] and g[1] by
nothing but zero; test_gravity_gpu.py holds the device's contact entry points to these references at an oblique gravity, and here the
references earn that first.  Descriptions at another gravity: term_states.with_gravity; 16 states each (entry_points._states, seed 61).

  (a) free fall: a floating-base model at rest with no torques, accelerated by the ORACLE's forward dynamics at that gravity -- every
      contact point then accelerates at g.  The reference's own gravity term enters once (the `+ g` of contact_points against the -g the
      oracle's base acceleration answers with), not twice, so a swapped or sign-flipped axis in it shows.
  (b) contact_points returns kinematic quantities: position, velocity and acceleration are the same at the oblique and at zero gravity.
  (c) contact_dynamics at the oblique gravity: contact_points at the returned ydd gives a_des back, the closed form equals the oracle's
      forward dynamics with the wrenches of lambda, and ydd_free is the oracle's forward dynamics of the re-gravitated description -- at
      the bounds test_contact_ref_cpu.py applies at the native gravity.
  (d) impulse_ref.contact_impulse reads no gravity: identical arrays from the native, the zero and the oblique description."""
import functools

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import impulse_ref as I
import oracle_py as O
import term_states as TS

B, SEED = 16, 61
ZERO = (0.0, 0.0, 0.0)
GRAVITIES = {"oblique": TS.OBLIQUE, "zero": ZERO}
POINTS = ["urdf_mini_cheetah", "tello_with_arms", "parallel_chain_exp_d10_l16"]  # (the contact sets of entry_points._contacts)


@functools.lru_cache(maxsize=None)
def at(model, gname):
    """the description of `model` at the gravity `gname` ("native": as built)"""
    blob = EP._model(model)
    if gname == "native":
        return blob
    out = TS.with_gravity(blob, GRAVITIES[gname])
    if EP._big(blob):
        EP._BIG.add(out)  # (the oracle with room for the big clusters)
    return out


@functools.lru_cache(maxsize=None)
def states(model):
    return tuple(TS._frozen(a) for a in EP._states(EP._model(model), B, SEED))


@pytest.mark.parametrize("gname", list(GRAVITIES))
def test_points_of_a_body_in_free_fall_accelerate_at_g(gname):
    model = "urdf_mini_cheetah"
    blob, g = at(model, gname), np.array(GRAVITIES[gname])
    q, qd, _ = states(model)
    zero = np.zeros_like(qd)
    ydd = O.forward_dynamics(blob, q, zero, zero)
    bodies, offsets = EP._contacts(EP._model(model))
    assert len(bodies) == 4
    pos, vel, acc = C.contact_points(blob, q, bodies, offsets, zero, ydd)
    err = np.abs(acc - g[None, None]).max() / (1 + np.abs(g).max())
    print(f"{model} {gname}: contact accelerations in free fall against g {err:.2e}")
    assert not vel.any() and err < 1e-10
    if gname == "oblique":  # (and the identity can fail: the points of a model that falls along another g)
        wrong = O.forward_dynamics(TS.with_gravity(blob, (g[1], g[0], g[2])), q, zero, zero)
        assert np.abs(C.contact_points(blob, q, bodies, offsets, zero, wrong)[2] - g[None, None]).max() > 1.0


@pytest.mark.parametrize("model", POINTS)
def test_contact_points_do_not_read_gravity(model):
    q, qd, ydd = states(model)  # (the third array as ydd, as the entry-point table feeds it)
    bodies, offsets = EP._contacts(EP._model(model))
    assert len(bodies) == {"urdf_mini_cheetah": 4, "tello_with_arms": 2}.get(model, 1)
    a, b = (C.contact_points(at(model, g), q, bodies, offsets, qd, ydd) for g in ("oblique", "zero"))
    for what, x, y in zip(("pos", "vel", "acc"), a, b):
        err = C.rel_per_state(x, y).max()
        print(f"{model} {what}: oblique against zero gravity {err:.2e}")
        assert err < 1e-12
    assert np.abs(a[2]).max() > 1.0  # (there is an acceleration to compare)


@pytest.mark.parametrize("key", ["cheetah_feet", "tello_feet"])
def test_contact_dynamics_closes_at_the_oblique_gravity(key):
    model, bodies, offsets = C.contact_set(key)
    blob = at(model, "oblique")
    q, qd, tau = states(model)
    a_des = np.random.default_rng(SEED).uniform(-1, 1, (B, len(bodies), 3))
    s = C.contact_dynamics(blob, q, qd, tau, bodies, offsets, a_des, 0.0)
    err = C.rel_per_state(C.contact_points(blob, q, bodies, offsets, qd, s["ydd"])[2], a_des).max()
    print(f"{key} oblique: p_ddot(ydd) against a_des {err:.2e}")
    assert err < 1e-8
    free = O.forward_dynamics(blob, q, qd, tau, big=EP._big(blob))
    assert C.rel_per_state(s["ydd_free"], free).max() < 1e-8
    assert C.rel_per_state(free, O.forward_dynamics(at(model, "native"), q, qd, tau, big=EP._big(blob))).max() > 1e-3  # (another gravity)
    ydd = O.forward_dynamics(blob, q, qd, tau, C.wrenches(blob, q, bodies, offsets, s["lam"]), big=EP._big(blob))
    err = C.rel_per_state(s["ydd"], ydd).max()
    print(f"{key} oblique: closed form against the oracle with wrenches {err:.2e}")
    assert err < 1e-8


@pytest.mark.parametrize("key", ["cheetah_feet", "tello_feet"])
def test_the_impulse_reference_reads_no_gravity(key):
    model, bodies, offsets = C.contact_set(key)
    q, qd, _ = states(model)
    v_des = np.random.default_rng(SEED).uniform(-1, 1, (B, len(bodies), 3))
    ref = {g: I.contact_impulse(at(model, g), q, qd, bodies, offsets, v_des, 0.25, 0.0) for g in ("native", "zero", "oblique")}
    for g in ("zero", "oblique"):
        for k in ("qd_next", "impulse", "A", "H", "Jw", "v_minus"):
            assert np.array_equal(ref[g][k], ref["native"][k]), f"{k} at the {g} gravity differs from the native one"
