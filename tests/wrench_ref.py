"""Test infrastructure for the sparse body wrenches (include/grbda_hip_wrench.h): (bodies, wrench, frame) -> the oracle's dense world-frame
f_ext, in plain numpy on the poses of kinematics_ref; and the bodies of a model by their place in the tree.  A helper module, not a test
file; nothing here calls the library under test.

With E (world -> body axes) and r (the body's origin in world coordinates) of a body's pose, a body-frame wrench [n_b; f_b] is the
world-frame row  f_w = E^T f_b,  n_w = E^T n_b + r x f_w  (the inverse of Xa.transformForceVector, SpatialTransforms.cpp:62-71).
tests/test_wrench_ref_cpu.py holds the helper to the oracle by the power identity; `defect` seeds the three mistakes that test must see."""
import numpy as np

import kinematics_ref as K
from deriv_recursion_numpy import parse

DEFECTS = ("halves_swapped", "E_transposed", "r_cross_f_dropped")


def dense_f_ext(blob, q, bodies, wrench, frame, defect=None):
    """f_ext[B, n_bodies, 6] for wrench[B, n, 6] on bodies[n]; wrenches on one body add"""
    wrench = np.asarray(wrench, dtype=np.float64)
    Xa = K.body_poses(blob, q)
    f = np.zeros((q.shape[0], Xa.shape[1], 6))
    for i, b in enumerate(bodies):
        n, fo = wrench[:, i, :3], wrench[:, i, 3:]
        if defect == "halves_swapped":
            n, fo = fo, n
        if frame == "body":
            E, r = Xa[:, b, :9].reshape(-1, 3, 3), Xa[:, b, 9:]
            Et = E if defect == "E_transposed" else E.transpose(0, 2, 1)
            fw = np.einsum("bij,bj->bi", Et, fo)
            nw = np.einsum("bij,bj->bi", Et, n)
            if defect != "r_cross_f_dropped":
                nw = nw + np.cross(r, fw)
            n, fo = nw, fw
        f[:, b, :3] += n
        f[:, b, 3:] += fo
    return f


def world_twists(blob, q, qd):
    """[B, n_bodies, 6]: the body velocities [omega; v of the point at the world origin] in world axes"""
    Xa = K.body_poses(blob, q)
    v = K.body_twists(blob, q, qd, np.zeros_like(qd))[:, :, :6]
    E, r = Xa[:, :, :9].reshape(q.shape[0], -1, 3, 3), Xa[:, :, 9:]
    om = np.einsum("bnji,bnj->bni", E, v[:, :, :3])
    lin = np.einsum("bnji,bnj->bni", E, v[:, :, 3:]) + np.cross(r, om)
    return np.concatenate([om, lin], axis=2)


def tree_places(blob):
    """The bodies of a model of revolute links, links with rotors, leaf pairs and a base (models.chain_test_tree, the URDF humanoids) by
    place: dict(base, links -- the link body of every one- or two-body cluster --, rotors, pairs -- (link1, link2) --, mid -- links with one
    child cluster --, tips -- links without --, forks -- links with two or more)."""
    m = parse(blob)
    bodies, clusters = m["bodies"], m["clusters"]
    members = {c: [i for i, b in enumerate(bodies) if b["cluster"] == c] for c in range(len(clusters))}
    out = dict(base=None, links=[], rotors=[], pairs=[], mid=[], tips=[], forks=[])
    for c, mem in members.items():
        inside = [i for i in mem if bodies[i]["parent"] in mem]
        if len(mem) == 1:
            (out["links"].append(mem[0]) if bodies[mem[0]]["parent"] >= 0 or clusters[c][6] == 1 else out.__setitem__("base", mem[0]))
        elif len(mem) == 2 and not inside:  # link and rotor side by side: the rotor is the one nothing hangs off, the second by registration
            out["links"].append(mem[0])
            out["rotors"].append(mem[1])
        elif len(mem) == 4 and len(inside) == 1:
            l2 = inside[0]
            out["pairs"].append((bodies[l2]["parent"], l2))
            out["rotors"] += [i for i in mem if i not in (l2, bodies[l2]["parent"])]
    for l in out["links"]:
        kids = {bodies[i]["cluster"] for i in range(len(bodies)) if bodies[i]["parent"] == l}
        out["tips" if not kids else "mid" if len(kids) == 1 else "forks"].append(l)
    return out
