"""Test infrastructure: the spanning-tree kinematics of a model description in plain numpy -- body twists, spanning rates, frame
Jacobians and body poses -- the reference the device outputs grbda_body_twists_*, grbda_spanning_* and the J of grbda_inv_osim_* are held
to.  A helper module, not a test file; nothing here calls the library under test.

The recursion, in body coordinates (X_i = Xmot(rot(axis_i, q_i) E_i, r_i), E_i / r_i of the description; a free base: Xmot(R(q), p)):
    v_i = X_i v_p + S_i qd_i                          v_ground = 0
    a_i = X_i a_p + S_i qdd_i + v_i x S_i qd_i        a_ground = -gravity (the convention of include/grbda_hip.h)
with the spanning rates qd_span = G yd, qdd_span = G ydd + g: G the description's constant for explicit clusters; for implicit clusters
G(q), g(q, qd) of oracle_py.cluster_constraint, one call per state and cluster (the joint angle is the spanning position).  Everything
else is batched over the states with array operations.  tests/test_kinematics_ref_cpu.py pins the module to the oracle: through
f = I a + v x* I v, a backward sum and G^T it reproduces oracle_py.inverse_dynamics (rnea_from_twists), its poses are
oracle_py.body_poses, its Jacobians the oracle's unit-wrench Jacobians.

dtype = np.float32 runs the same recursion in single precision on the same inputs (G and g of implicit clusters are rounded from the
oracle's): what single precision itself costs -- the yardstick of term_states.within_float, never the reference of a comparison.

The single-state builders Xmot, crm, crf (deriv_recursion_numpy) and coordinate_rotation, quat_to_rotmat, rpy_to_rotmat (modeldesc) are
what the batched builders below restate; the CPU test holds each batched builder to its single-state original."""
import functools

import numpy as np

import oracle_py as O
from deriv_recursion_numpy import Xmot, crf, crm, parse  # noqa: F401  (the single-state originals of the batched builders)
from generalized_rbda_amd.modeldesc import coordinate_rotation, quat_to_rotmat, rpy_to_rotmat  # noqa: F401

_parse = functools.lru_cache(maxsize=None)(parse)


# ---- batched builders: [B, ...] in, [B, 3, 3] / [B, 6, 6] out, in the dtype of the input ----------------------------------------------
def rot_axis(axis, th):
    """coordinate_rotation for angles th[B]"""
    s, c, o, z = np.sin(th), np.cos(th), np.ones_like(th), np.zeros_like(th)
    rows = ([o, z, z, z, c, s, z, -s, c], [c, z, -s, z, o, z, s, z, c], [c, s, z, -s, c, z, z, z, o])[axis]
    return np.stack(rows, axis=-1).reshape(-1, 3, 3)


def rot_rpy(rpy):
    """rpy_to_rotmat for rpy[B, 3]"""
    return rot_axis(0, rpy[:, 0]) @ rot_axis(1, rpy[:, 1]) @ rot_axis(2, rpy[:, 2])


def rot_quat(e):
    """quat_to_rotmat for e[B, 4], scalar first; the quaternion is used as it is (not normalised)"""
    e0, e1, e2, e3 = e.T
    one = np.ones_like(e0)
    cols = [one - 2 * (e2 * e2 + e3 * e3), 2 * (e1 * e2 - e0 * e3), 2 * (e1 * e3 + e0 * e2),
            2 * (e1 * e2 + e0 * e3), one - 2 * (e1 * e1 + e3 * e3), 2 * (e2 * e3 - e0 * e1),
            2 * (e1 * e3 - e0 * e2), 2 * (e2 * e3 + e0 * e1), one - 2 * (e1 * e1 + e2 * e2)]
    return np.stack(cols, axis=-1).reshape(-1, 3, 3).transpose(0, 2, 1)


def skew_b(v):
    z = np.zeros_like(v[:, 0])
    return np.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], axis=-1).reshape(-1, 3, 3)


def xmot_b(E, r):
    """Xmot for E[B, 3, 3], r[B, 3]"""
    X = np.zeros((E.shape[0], 6, 6), dtype=E.dtype)
    X[:, :3, :3] = E
    X[:, 3:, 3:] = E
    X[:, 3:, :3] = -E @ skew_b(r)
    return X


def crm_b(v):
    """crm for v[B, 6]"""
    M = np.zeros((v.shape[0], 6, 6), dtype=v.dtype)
    M[:, :3, :3] = M[:, 3:, 3:] = skew_b(v[:, :3])
    M[:, 3:, :3] = skew_b(v[:, 3:])
    return M


def crf_b(v):
    return -crm_b(v).transpose(0, 2, 1)


def _mv(M, x):
    return np.einsum("bij,bj->bi", M, x)


# ---- the model at B states -----------------------------------------------------------------------------------------------------------
class _Kin:
    """transforms of every body at the states q, and the spanning maps of every cluster"""

    def __init__(self, blob, q, big=False, dtype=np.float64):
        self.blob, self.big, self.dtype = blob, big, dtype
        self.m = m = _parse(blob)
        self.q64 = np.ascontiguousarray(q, dtype=np.float64)
        self.q = q = self.q64.astype(dtype)
        self.B = B = q.shape[0]
        nb = m["nb"]
        # where each cluster starts in the spanning layout, and each body's row there
        self.span_at, at = [], 0
        for cl in m["clusters"]:
            self.span_at.append(at)
            at += cl[8]
        self.n_span = at
        self.row = [self.span_at[bd["cluster"]] + (0 if bd["jtype"] == 1 else bd["sub"]) for bd in m["bodies"]]
        # joint angles: explicit clusters G q_cluster, implicit clusters the spanning positions themselves
        angle = [None] * nb
        for cl in m["clusters"]:
            pc, fb, k, qi, npos, vi, n, nsp, nsv, ctype = cl[:10]
            if ctype == 0:
                assert npos == n and nsv == k
                Gc = m["dbls"][cl[13]:cl[13] + nsv * n].reshape(nsv, n).astype(dtype)
                ang = q[:, qi:qi + n] @ Gc.T
            elif ctype in (2, 3):
                assert npos == k
                ang = q[:, qi:qi + k]
            else:
                continue
            for i in range(k):
                assert m["bodies"][fb + i]["sub"] == i
                angle[fb + i] = ang[:, i]
        self.X, self.E, self.r = [None] * nb, [None] * nb, [None] * nb  # X: parent -> body; E, r: world -> body (TreeNode::Xa_)
        for b, bd in enumerate(m["bodies"]):
            p = bd["parent"]
            if bd["jtype"] == 1:
                assert p < 0, "a free joint hangs off the ground"
                qi = m["clusters"][bd["cluster"]][3]
                E = rot_quat(q[:, qi + 3:qi + 7]) if m["ori"] == 0 else rot_rpy(q[:, qi + 3:qi + 6])
                r = q[:, qi:qi + 3]
            else:
                E = rot_axis(bd["axis"], angle[b]) @ bd["E"].astype(dtype)
                r = np.broadcast_to(bd["r"].astype(dtype), (B, 3))
            self.X[b] = xmot_b(E, r)
            if p < 0:
                self.E[b], self.r[b] = E, r
            else:
                self.E[b] = E @ self.E[p]
                self.r[b] = self.r[p] + np.einsum("bji,bj->bi", self.E[p], r)

    def maps(self, qd=None):
        """per cluster (G[B, n_span_vel, n_vel], g[B, n_span_vel]); qd None: g = 0 (G does not depend on the velocities)"""
        m, B, dtype = self.m, self.B, self.dtype
        qd64 = np.zeros((B, m["nv"])) if qd is None else np.ascontiguousarray(qd, dtype=np.float64)
        out = []
        for ci, cl in enumerate(m["clusters"]):
            pc, fb, k, qi, npos, vi, n, nsp, nsv, ctype, rows = cl[:11]
            g = np.zeros((B, nsv), dtype=dtype)
            if ctype == 1:
                G = np.broadcast_to(np.eye(6, dtype=dtype), (B, 6, 6))
            elif ctype == 0:
                G = np.broadcast_to(m["dbls"][cl[13]:cl[13] + nsv * n].reshape(nsv, n).astype(dtype), (B, nsv, n))
            else:
                G = np.empty((B, nsv, n), dtype=dtype)
                for b in range(B):
                    Gb, gb = O.cluster_constraint(self.blob, ci, self.q64[b], qd64[b], nsv, n, rows, big=self.big)[:2]
                    G[b], g[b] = Gb, gb
            out.append((G, g))
        return out

    def rates(self, qd, ydd):
        """(qd_span, qdd_span) in the layout of grbda_spanning_*"""
        qd_, ydd_ = np.asarray(qd).astype(self.dtype), np.asarray(ydd).astype(self.dtype)
        vs, as_ = (np.zeros((self.B, self.n_span), dtype=self.dtype) for _ in range(2))
        for cl, at, (G, g) in zip(self.m["clusters"], self.span_at, self.maps(qd)):
            vi, n, nsv = cl[5], cl[6], cl[8]
            vs[:, at:at + nsv] = _mv(G, qd_[:, vi:vi + n])
            as_[:, at:at + nsv] = _mv(G, ydd_[:, vi:vi + n]) + g
        return vs, as_

    def joint_rate(self, b, span):
        """S_b times the body's rows of a spanning array: [B, 6]"""
        bd = self.m["bodies"][b]
        if bd["jtype"] == 1:
            return span[:, self.row[b]:self.row[b] + 6]
        out = np.zeros((self.B, 6), dtype=self.dtype)
        out[:, bd["axis"]] = span[:, self.row[b]]
        return out

    def propagate(self, vs, as_=None):
        """v[B, nb, 6] (and a[B, nb, 6] when the spanning accelerations are given) of the recursion in the module docstring"""
        m, nb = self.m, self.m["nb"]
        v = np.zeros((self.B, nb, 6), dtype=self.dtype)
        a = None if as_ is None else np.zeros((self.B, nb, 6), dtype=self.dtype)
        a0 = np.broadcast_to((-m["grav"]).astype(self.dtype), (self.B, 6))
        for b, bd in enumerate(m["bodies"]):
            p = bd["parent"]
            vj = self.joint_rate(b, vs)
            v[:, b] = vj if p < 0 else _mv(self.X[b], v[:, p]) + vj
            if a is not None:
                a[:, b] = _mv(self.X[b], a0 if p < 0 else a[:, p]) + self.joint_rate(b, as_) + _mv(crm_b(v[:, b]), vj)
        return v, a


# ---- what the tests use --------------------------------------------------------------------------------------------------------------
def spanning_rates(blob, q, qd, ydd, big=False, dtype=np.float64):
    """(qd_span, qdd_span) = (G yd, G ydd + g), [B, n_span_vel] each, in the layout of grbda_spanning_*: the free base's 6 components
    unchanged, then the clusters in model order, bodies by sub-index"""
    return _Kin(blob, q, big, dtype).rates(qd, ydd)


def body_twists(blob, q, qd, ydd, big=False, dtype=np.float64):
    """[B, n_bodies, 12] = [v 6 | a 6], each [angular 3; linear 3], in the body's own coordinates; the base starts from -gravity"""
    kin = _Kin(blob, q, big, dtype)
    v, a = kin.propagate(*kin.rates(qd, ydd))
    return np.concatenate([v, a], axis=2)


def body_poses(blob, q, big=False, dtype=np.float64):
    """[B, n_bodies, 12] = E (9, row-major, world -> body) then the body origin r in world coordinates: the layout of grbda_body_poses_*"""
    kin = _Kin(blob, q, big, dtype)
    return np.stack([np.concatenate([E.reshape(-1, 9), r], axis=1) for E, r in zip(kin.E, kin.r)], axis=1)


def frame_jacobians(blob, q, bodies, offsets, big=False, dtype=np.float64):
    """[B, 6 n, nv]: frame c sits at the body-fixed point offsets[c] of body bodies[c], with the body's axes.  Column k is the velocity of
    body_twists(q, e_k, 0) moved to the point: [omega; v + omega x offset]"""
    kin = _Kin(blob, q, big, dtype)
    nv = kin.m["nv"]
    maps = kin.maps()
    J = np.zeros((kin.B, 6 * len(bodies), nv), dtype=dtype)
    for cl, at, (G, _) in zip(kin.m["clusters"], kin.span_at, maps):
        vi, n, nsv = cl[5], cl[6], cl[8]
        for k in range(n):  # yd = e_(vi + k): only this cluster has spanning rates
            vs = np.zeros((kin.B, kin.n_span), dtype=dtype)
            vs[:, at:at + nsv] = G[:, :, k]
            v, _ = kin.propagate(vs)
            for c, (bd, off) in enumerate(zip(bodies, offsets)):
                w = v[:, bd, :3]
                J[:, 6 * c:6 * c + 3, vi + k] = w
                J[:, 6 * c + 3:6 * c + 6, vi + k] = v[:, bd, 3:] + np.cross(w, np.asarray(off, dtype=dtype)[None])
    return J


def rnea_from_twists(blob, q, v, a, big=False):
    """tau[B, nv] of the twists v, a[B, n_bodies, 6]: f = I a + v x* I v, summed towards the root, projected on the joint axes and
    through G^T.  With the twists of body_twists this is the inverse dynamics -- what pins the module to oracle_py.inverse_dynamics"""
    kin = _Kin(blob, q, big)
    m = kin.m
    f = np.zeros_like(v)
    for b, bd in enumerate(m["bodies"]):
        Iv = v[:, b] @ bd["I"].T
        f[:, b] = a[:, b] @ bd["I"].T + _mv(crf_b(v[:, b]), Iv)
    tau_span = np.zeros((kin.B, kin.n_span))
    for b in range(m["nb"] - 1, -1, -1):
        bd = m["bodies"][b]
        if bd["jtype"] == 1:
            tau_span[:, kin.row[b]:kin.row[b] + 6] = f[:, b]
        else:
            tau_span[:, kin.row[b]] = f[:, b, bd["axis"]]
        if bd["parent"] >= 0:
            f[:, bd["parent"]] += np.einsum("bji,bj->bi", kin.X[b], f[:, b])
    tau = np.zeros((kin.B, m["nv"]))
    for cl, at, (G, _) in zip(m["clusters"], kin.span_at, kin.maps()):
        vi, n, nsv = cl[5], cl[6], cl[8]
        tau[:, vi:vi + n] = np.einsum("bij,bi->bj", G, tau_span[:, at:at + nsv])
    return tau


def oracle_frame_jacobians(blob, q, bodies, offsets):
    """The same Jacobians from the ORACLE's inverse dynamics with unit wrenches: row k of frame c is tau(no wrench) - tau(unit wrench k
    of the frame, as a world wrench on its body) at zero velocity and acceleration.  The route the older tests use; independent of the
    recursion above."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    B, m = q.shape[0], _parse(blob)
    nb, nv = m["nb"], m["nv"]
    Xa = O.body_poses(blob, q, nb)
    zero = np.zeros((B, nv))
    tau0 = O.inverse_dynamics(blob, q, zero, zero)
    J = np.zeros((B, 6 * len(bodies), nv))
    for c, (bd, off) in enumerate(zip(bodies, offsets)):
        E, r = Xa[:, bd, :9].reshape(B, 3, 3), Xa[:, bd, 9:]
        p = r + np.einsum("bji,j->bi", E, np.asarray(off, dtype=np.float64))
        for k in range(6):
            e = E[:, k % 3, :]  # body axis in world coordinates
            fext = np.zeros((B, nb, 6))
            if k < 3:
                fext[:, bd, :3] = e
            else:
                fext[:, bd, :3] = np.cross(p, e)
                fext[:, bd, 3:] = e
            J[:, 6 * c + k] = tau0 - O.inverse_dynamics(blob, q, zero, zero, f_ext=fext)
    return J


# ---- the measure of the checkers ------------------------------------------------------------------------------------------------------
def block_errors(got, ref):
    """per state, v and a blocks apart: |got - ref|_inf / (1 + |ref|_inf of that state and block) of twists [B, n_bodies, 12] -> [B, 2]"""
    B = ref.shape[0]
    out = np.empty((B, 2))
    for i, sl in enumerate((slice(0, 6), slice(6, 12))):
        d = np.abs(got[:, :, sl] - ref[:, :, sl]).reshape(B, -1).max(axis=1)
        out[:, i] = d / (1.0 + np.abs(ref[:, :, sl]).reshape(B, -1).max(axis=1))
    return out
