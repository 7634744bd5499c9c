"""Test infrastructure: frame Jacobians and their drift at a listed few body frames in numpy, from kinematics_ref alone -- the reference
the device entry points of include/grbda_hip_jacobians.h are held to.  A helper module, not a test file; nothing here calls the library
under test.  tests/test_frame_jacobian_ref_cpu.py pins it to the oracle's unit-wrench Jacobians and to contact_ref.

A frame is the point o = offsets[i] (the reference's body axes) fixed in body bodies[i].  With E the body's rotation world -> body and
[w; v | al; a] its twist at (q, qd, 0) in body axes, a WITHOUT the gravity term (body_twists starts the root from -gravity, which reaches
body b as [0; E_b (-g)]: added back here):
    body frame    J = K.frame_jacobians                      drift = [al ; a + al x o]
    world frame   J = [E^T J_ang ; E^T J_lin]                drift = [E^T al ; E^T (a + al x o + w x (v + w x o))]"""
import numpy as np

import kinematics_ref as K


def _rotations(blob, q, bodies, big):
    Xa = K.body_poses(blob, q, big=big)[:, list(bodies)]
    return Xa[:, :, :9].reshape(q.shape[0], len(bodies), 3, 3)


def _offsets(bodies, offsets):
    return np.zeros((len(bodies), 3)) if offsets is None else np.asarray(offsets, dtype=np.float64).reshape(len(bodies), 3)


def to_world(E, x):
    """E^T x for E[B, n, 3, 3] and x[B, n, 3, ...]"""
    return np.einsum("bcji,bcj...->bci...", E, x)


def jacobians(blob, q, bodies, offsets=None, frame="body", big=False):
    """J[B, n, 6, nv], each frame [angular 3; linear 3]"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    off = _offsets(bodies, offsets)
    J = K.frame_jacobians(blob, q, list(bodies), [tuple(o) for o in off], big=big).reshape(q.shape[0], len(bodies), 6, -1)
    if frame == "body":
        return J
    E = _rotations(blob, q, bodies, big)
    return np.concatenate([to_world(E, J[:, :, :3]), to_world(E, J[:, :, 3:])], axis=2)


def twists_without_gravity(blob, q, qd, ydd, bodies, big=False):
    """[B, n, 12] = K.body_twists at the listed bodies with the gravity term taken out of the acceleration"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    V = K.body_twists(blob, q, qd, ydd, big=big)[:, list(bodies)].copy()
    g = K._parse(blob)["grav"]
    assert not g[:3].any()
    V[:, :, 9:] += np.einsum("bcij,j->bci", _rotations(blob, q, bodies, big), g[3:])
    return V


def frame_acceleration(blob, q, qd, ydd, bodies, offsets=None, frame="body", big=False):
    """[B, n, 6]: the frame's acceleration at (q, qd, ydd) without gravity, by the formulas of the module docstring"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    o = _offsets(bodies, offsets)[None]
    V = twists_without_gravity(blob, q, qd, ydd, bodies, big)
    w, v, al, a = V[:, :, 0:3], V[:, :, 3:6], V[:, :, 6:9], V[:, :, 9:12]
    lin = a + np.cross(al, o)
    if frame == "body":
        return np.concatenate([al, lin], axis=2)
    E = _rotations(blob, q, bodies, big)
    return np.concatenate([to_world(E, al), to_world(E, lin + np.cross(w, v + np.cross(w, o)))], axis=2)


def drift(blob, q, qd, bodies, offsets=None, frame="body", big=False):
    """Jdot qd [B, n, 6]: the frame's acceleration at ydd = 0"""
    return frame_acceleration(blob, q, qd, np.zeros_like(np.asarray(qd, dtype=np.float64)), bodies, offsets, frame, big)


# ---- many lists on the same states: the quantities of every body once, a list assembled from them -------------------------------------
def all_bodies(blob, q, qd, big=False):
    """(J0[B, nb, 6, nv], E[B, nb, 3, 3], V0[B, nb, 12]): the body-frame Jacobians at the body origins, the rotations and the twists at
    (q, qd, 0) without gravity, of every body"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    nb = K._parse(blob)["nb"]
    every = list(range(nb))
    return (jacobians(blob, q, every, None, "body", big), _rotations(blob, q, every, big),
            twists_without_gravity(blob, q, qd, np.zeros_like(np.asarray(qd, dtype=np.float64)), every, big))


def assemble(J0, E, V0, bodies, offsets=None, frame="body"):
    """(J[B, n, 6, nv], drift[B, n, 6]) of a list from all_bodies: the same formulas as jacobians() and drift(), the offset applied to the
    origin's columns (v + w x o is linear in the column)"""
    bodies = list(bodies)
    o = _offsets(bodies, offsets)[None]
    J, E, V = J0[:, bodies].copy(), E[:, bodies], V0[:, bodies]
    J[:, :, 3:] += np.cross(J[:, :, :3], o[:, :, :, None], axisa=2, axisb=2, axisc=2)
    w, v, al, a = V[:, :, 0:3], V[:, :, 3:6], V[:, :, 6:9], V[:, :, 9:12]
    lin = a + np.cross(al, o)
    if frame == "body":
        return J, np.concatenate([al, lin], axis=2)
    J = np.concatenate([to_world(E, J[:, :, :3]), to_world(E, J[:, :, 3:])], axis=2)
    return J, np.concatenate([to_world(E, al), to_world(E, lin + np.cross(w, v + np.cross(w, o)))], axis=2)
