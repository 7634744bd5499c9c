"""frame_jacobian_ref, the numpy reference of the frame Jacobians and their drift, pinned to what the project already trusts: the oracle's
unit-wrench Jacobians (kinematics_ref.oracle_frame_jacobians) and the contact-point kinematics of contact_ref.  8 states, fp64, 1e-9 as
max |got - ref| / (1 + max |ref|).  No device and no call of the entry points."""
import functools

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import frame_jacobian_ref as FJ
import kinematics_ref as K
import term_states as TS
import wrench_ref as W
from deriv_recursion_numpy import parse

MODELS = ("rev_rotor_chain_3", "urdf_mini_cheetah")
B, SEED, TOL = 8, 71, 1e-9
OFFSETS = [(0.03, -0.07, 0.11), (-0.05, 0.02, -0.2), (0.013, 0.09, 0.04)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(blob, blob at the oblique gravity, q, qd, ydd, bodies, offsets): the deepest link, a rotor and the first body"""
    blob = EP._model(name)
    parent = [b["parent"] for b in parse(blob)["bodies"]]
    places = W.tree_places(blob)
    depth = lambda b: 0 if b < 0 else 1 + depth(parent[b])
    bodies = [max(places["links"], key=lambda b: (depth(b), b)), places["rotors"][-1], 0]
    q, qd, ydd = EP._states(blob, B, SEED)
    return blob, TS.with_gravity(blob, TS.OBLIQUE), q, qd, ydd, bodies, OFFSETS


def _held(got, ref, what):
    err = EP._rel(np.asarray(got).reshape(B, -1), np.asarray(ref).reshape(B, -1))
    print(f"{what}: {err:.2e}")
    assert np.isfinite(got).all() and err < TOL, (what, err)


@pytest.mark.parametrize("name", MODELS)
def test_the_body_frame_jacobian_is_the_oracles_unit_wrench_jacobian(name):
    blob, _, q, _, _, bodies, offsets = case(name)
    J = FJ.jacobians(blob, q, bodies, offsets, "body")
    assert J.shape == (B, 3, 6, parse(blob)["nv"])
    _held(J, K.oracle_frame_jacobians(blob, q, bodies, offsets), f"{name} body-frame J")
    assert np.abs(J).max() > 0.1


@pytest.mark.parametrize("name", MODELS)
def test_the_world_frame_jacobian_gives_the_point_velocity(name):
    blob, _, q, qd, _, bodies, offsets = case(name)
    J = FJ.jacobians(blob, q, bodies, offsets, "world")
    vel = C.contact_points(blob, q, bodies, offsets, qd)[1]
    _held(np.einsum("bcik,bk->bci", J[:, :, 3:], qd), vel, f"{name} world-frame J qd, linear rows")
    assert np.abs(vel).max() > 0.1


@pytest.mark.parametrize("name", MODELS)
def test_the_world_frame_linear_drift_is_the_point_acceleration_at_any_gravity(name):
    blob, oblique, q, qd, _, bodies, offsets = case(name)
    acc = C.contact_points(oblique, q, bodies, offsets, qd, np.zeros_like(qd))[2]
    d = FJ.drift(oblique, q, qd, bodies, offsets, "world")
    _held(d[:, :, 3:], acc, f"{name} world-frame linear drift at the oblique gravity")
    for frame in ("body", "world"):  # the drift does not see the gravity
        _held(FJ.drift(oblique, q, qd, bodies, offsets, frame), FJ.drift(blob, q, qd, bodies, offsets, frame), f"{name} {frame} drift, two gravities")
    assert np.abs(acc).max() > 0.1


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("frame", ["body", "world"])
def test_the_jacobian_and_the_drift_make_the_frame_acceleration(name, frame):
    _, oblique, q, qd, ydd, bodies, offsets = case(name)
    ydd = np.random.default_rng(SEED).uniform(-3, 3, size=ydd.shape)
    J, d = FJ.jacobians(oblique, q, bodies, offsets, frame), FJ.drift(oblique, q, qd, bodies, offsets, frame)
    acc = FJ.frame_acceleration(oblique, q, qd, ydd, bodies, offsets, frame)
    _held(np.einsum("bcik,bk->bci", J, ydd) + d, acc, f"{name} {frame} J ydd + drift")
    assert np.abs(d).max() > 0.1 and np.abs(acc - d).max() > 0.1


def test_no_offsets_means_the_body_origins():
    blob, _, q, qd, _, bodies, _ = case("urdf_mini_cheetah")
    zero = [(0.0, 0.0, 0.0)] * len(bodies)
    for frame in ("body", "world"):
        assert np.array_equal(FJ.jacobians(blob, q, bodies, None, frame), FJ.jacobians(blob, q, bodies, zero, frame))
        assert np.array_equal(FJ.drift(blob, q, qd, bodies, None, frame), FJ.drift(blob, q, qd, bodies, zero, frame))


@pytest.mark.parametrize("name", MODELS)
def test_a_list_assembled_from_every_bodys_quantities_is_the_direct_one(name):
    """all_bodies / assemble, what the device test builds its many lists from, against jacobians() and drift()"""
    _, oblique, q, qd, _, bodies, offsets = case(name)
    every = FJ.all_bodies(oblique, q, qd)
    for frame in ("body", "world"):
        for off in (offsets, None):
            J, d = FJ.assemble(*every, bodies, off, frame)
            _held(J, FJ.jacobians(oblique, q, bodies, off, frame), f"{name} {frame} assembled J")
            _held(d, FJ.drift(oblique, q, qd, bodies, off, frame), f"{name} {frame} assembled drift")
