"""jacobian_product_ref, the numpy reference of J v and J^T f at a listed few body frames, pinned independently of the einsum over
frame_jacobian_ref.jacobians that it is.  5 states, fp64, no device and no call of the entry points.

  jv   against the velocity half of frame_jacobian_ref.twists_without_gravity(q, v, 0) -- the recursion of the body twists, which forms no
       Jacobian -- moved to the point, [w ; v + w x o], and for world frames turned with E^T.
  jtf  against the oracle's inverse dynamics through wrench_ref.dense_f_ext: at qd = ydd = 0,
           jtf(f) = ID(no wrench) - ID(the listed wrenches applied),
       the joint torques that BALANCE the wrenches.  The wrench f_i = [moment; force] acts at the frame's point offsets[i], in the body's
       axes (frame="body") or in world axes (frame="world"); wrench_ref takes a body-frame wrench at the body's ORIGIN, so the test turns a
       world-frame wrench with E and moves the moment, n + o x f, before it hands it over.
  the duality f . jv(v) == jtf(f) . v to 1e-12 (relative to the size of the terms).
Every list holds a body twice with two offsets, next to the first body and the deepest leaf."""
import functools

import numpy as np
import pytest

import entry_points as EP
import frame_jacobian_ref as FJ
import jacobian_product_ref as JP
import kinematics_ref as K
import oracle_py as O
import term_states as TS
import wrench_ref as W
from deriv_recursion_numpy import parse

MODELS = ("rev_rotor_chain_3", "urdf_mini_cheetah", "tello_with_arms")
FRAMES = ("body", "world")
B, SEED, TOL = 5, 83, 1e-9
OFFSETS = [(0.03, -0.07, 0.11), (-0.05, 0.02, -0.2), (0.013, 0.09, 0.04), (0.08, 0.06, -0.03)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(blob at the oblique gravity, q, v, f, bodies, offsets): the deepest leaf, the last body, the first body, the deepest leaf again"""
    blob = EP._model(name)
    parent = [b["parent"] for b in parse(blob)["bodies"]]
    depth = lambda b: 0 if b < 0 else 1 + depth(parent[b])
    deepest = max((b for b in range(len(parent)) if b not in parent), key=lambda b: (depth(b), b))
    bodies = [deepest, len(parent) - 1, 0, deepest]
    q = EP._states(blob, B, SEED)[0]
    rng = np.random.default_rng(SEED)
    v = rng.uniform(-2, 2, size=(B, parse(blob)["nv"]))
    f = rng.uniform(-3, 3, size=(B, len(bodies), 6))
    return TS.with_gravity(blob, TS.OBLIQUE), q, v, f, bodies, OFFSETS


def _held(got, ref, what, tol=TOL):
    err = EP._rel(np.asarray(got).reshape(B, -1), np.asarray(ref).reshape(B, -1))
    print(f"{what}: {err:.2e}")
    assert np.isfinite(got).all() and err < tol, (what, err)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("frame", FRAMES)
def test_jv_is_the_listed_twist_moved_to_the_point(name, frame):
    blob, q, v, _, bodies, offsets = case(name)
    got = JP.jv(blob, q, v, bodies, offsets, frame)
    assert got.shape == (B, len(bodies), 6)
    V = FJ.twists_without_gravity(blob, q, v, np.zeros_like(v), bodies)
    o = np.asarray(offsets)[None]
    w, lin = V[:, :, 0:3], V[:, :, 3:6] + np.cross(V[:, :, 0:3], o)
    if frame == "world":
        E = K.body_poses(blob, q)[:, bodies, :9].reshape(B, len(bodies), 3, 3)
        w, lin = FJ.to_world(E, w), FJ.to_world(E, lin)
    _held(got, np.concatenate([w, lin], axis=2), f"{name} {frame} jv against the listed twists")
    assert np.abs(got).max() > 0.1


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("frame", FRAMES)
def test_jtf_is_what_inverse_dynamics_loses_to_the_wrenches(name, frame):
    blob, q, _, f, bodies, offsets = case(name)
    got = JP.jtf(blob, q, f, bodies, offsets, frame)
    assert got.shape == (B, parse(blob)["nv"])
    n, fo = f[:, :, :3], f[:, :, 3:]
    if frame == "world":  # into the body's axes
        E = K.body_poses(blob, q)[:, bodies, :9].reshape(B, len(bodies), 3, 3)
        n, fo = np.einsum("bcij,bcj->bci", E, n), np.einsum("bcij,bcj->bci", E, fo)
    at_origin = np.concatenate([n + np.cross(np.asarray(offsets)[None], fo), fo], axis=2)
    zero = np.zeros((B, parse(blob)["nv"]))
    free = O.inverse_dynamics(blob, q, zero, zero)
    loaded = O.inverse_dynamics(blob, q, zero, zero, W.dense_f_ext(blob, q, bodies, at_origin, "body"))
    _held(got, free - loaded, f"{name} {frame} jtf against ID - ID with the wrenches")
    assert np.abs(got).max() > 0.1
    # a frame listed twice contributes twice: the list is the sum of its frames
    parts = sum(JP.jtf(blob, q, f[:, i:i + 1], bodies[i:i + 1], offsets[i:i + 1], frame) for i in range(len(bodies)))
    _held(got, parts, f"{name} {frame} jtf of the list against the sum over its frames", 1e-12)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("frame", FRAMES)
def test_the_two_products_are_dual(name, frame):
    blob, q, v, f, bodies, offsets = case(name)
    lhs = np.einsum("bci,bci->b", f, JP.jv(blob, q, v, bodies, offsets, frame))
    rhs = np.einsum("bk,bk->b", JP.jtf(blob, q, f, bodies, offsets, frame), v)
    size = np.einsum("bci,bci->b", np.abs(f), np.abs(JP.jv(blob, q, v, bodies, offsets, frame)))
    err = float((np.abs(lhs - rhs) / (1 + size)).max())
    print(f"{name} {frame} f . jv(v) - jtf(f) . v: {err:.2e}")
    assert err < 1e-12 and np.abs(lhs).max() > 0.1


def test_no_offsets_means_the_body_origins():
    blob, q, v, f, bodies, _ = case("urdf_mini_cheetah")
    zero = [(0.0, 0.0, 0.0)] * len(bodies)
    for frame in FRAMES:
        assert np.array_equal(JP.jv(blob, q, v, bodies, None, frame), JP.jv(blob, q, v, bodies, zero, frame))
        assert np.array_equal(JP.jtf(blob, q, f, bodies, None, frame), JP.jtf(blob, q, f, bodies, zero, frame))
