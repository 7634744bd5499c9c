"""CPU reference of the step / rollout vector-Jacobian products (a helper module, not a test file; nothing here calls the library):
the closed form of include/grbda_hip_step_vjp.h in numpy, the tangent step and its inverse on whole states, and the step and rollout
compositions over numpy arrays.

One step (integrate_ref.reference_step): qd' = qd + dt ydd, q' = q (+) dt qd'.  With omega' = qd'[base 0..2], v' = qd'[base 3..5],
phi = omega' dt, theta = |phi|, E = Exp([phi]x) = I + a [phi]x + b [phi]x^2 and J_r^T = I + b [phi]x + c [phi]x^2,
    a = sin(theta) / theta,   b = (1 - cos(theta)) / theta^2 = 2 (sin(theta / 2) / theta)^2,   c = (theta - sin(theta)) / theta^3,
the cotangents (g_q', g_qd') of the stepped state pull back to
    g_v          = g_qd' + dt g_q'                      explicit coordinates
    g_v[omega]   = g_qd'[omega] + dt J_r^T g_r'         base
    g_v[v]       = g_qd'[v] + dt E g_p'
    grad_ydd     = dt g_v,   grad_qd = g_v
    grad_q       = g_q'                                 explicit coordinates
    grad_q[rot]  = E g_r' + dt v' x (E g_p')            base
    grad_q[pos]  = E g_p'
Every position cotangent is [B, nv], along the tangent step of grbda_fd_dq_* (tangent_plus below)."""
import numpy as np

from generalized_rbda_amd.modeldesc import C_FREE, C_LOOP_POSITION, C_TRIG_POLY
from generalized_rbda_amd.states import parse_clusters

SERIES_BELOW = 0.1  # theta under which c is its series (the threshold of integrate_vjp_kernel)
DEFECTS = ("E_transposed", "Jr_identity", "cross_dropped", "cross_negated", "dt_missing")


def layout(blob):
    """(nq, nv, base, pairs): base = (q_index, v_index) of the quaternion base or None; pairs = [(q column, v column)] of every
    explicit coordinate.  Models with implicit clusters or a roll-pitch-yaw base have no closed form here."""
    m = parse_clusters(blob)
    base, pairs = None, []
    for c in m["clusters"]:
        (pc, fb, k, qi, npos, vi, nvel, nsp, nsv, ctype, rows, io, ni, do, nd, _) = c
        assert ctype not in (C_LOOP_POSITION, C_TRIG_POLY), "implicit clusters are not covered"
        if ctype == C_FREE:
            assert npos == 7 and base is None, "one quaternion base"
            base = (qi, vi)
        else:
            assert npos == nvel
            pairs += [(qi + a, vi + a) for a in range(nvel)]
    return m["nq"], m["nv"], base, pairs


def so3_coefficients(theta):
    """(a, b, c) of the docstring for an array of angles, in the array's type; a = 1, b = 1/2, c = 1/6 at theta = 0"""
    dt = theta.dtype.type
    safe = np.where(theta > 0, theta, dt(1))
    a = np.where(theta > 0, np.sin(safe) / safe, dt(1))
    s = np.sin(dt(0.5) * safe) / safe
    b = np.where(theta > 0, dt(2) * s * s, dt(0.5))
    t2 = theta * theta
    series = dt(1.0 / 6.0) - t2 * (dt(1.0 / 120.0) - t2 * dt(1.0 / 5040.0))
    big = np.where(theta >= dt(SERIES_BELOW), theta, dt(1))
    c = np.where(theta >= dt(SERIES_BELOW), (big - np.sin(big)) / (big * big * big), series)
    return a, b, c


def _apply(phi, k1, k2, g):
    """(I + k1 [phi]x + k2 [phi]x^2) g for [B,3] arrays and [B] coefficients"""
    x1 = np.cross(phi, g)
    return g + k1[:, None] * x1 + k2[:, None] * np.cross(phi, x1)


def integrate_vjp(blob, qd_next, dt, g_q=None, g_qd=None, dtype=np.float64, defect=None):
    """(grad_q, grad_qd, grad_ydd), each [B, nv], in `dtype` arithmetic.  defect: one of DEFECTS, a deliberately wrong formula (the
    difference test shows that it notices each)."""
    assert defect is None or defect in DEFECTS
    nq, nv, base, pairs = layout(blob)
    T = np.dtype(dtype).type
    qn = np.asarray(qd_next, dtype=dtype)
    gq = np.zeros_like(qn) if g_q is None else np.asarray(g_q, dtype=dtype)
    gqd = np.zeros_like(qn) if g_qd is None else np.asarray(g_qd, dtype=dtype)
    h = T(dt)
    grad_q = gq.copy()
    gv = gqd + h * gq
    if base is not None:
        vi = base[1]
        w, v = qn[:, vi:vi + 3], qn[:, vi + 3:vi + 6]
        gr, gp = gq[:, vi:vi + 3], gq[:, vi + 3:vi + 6]
        phi = w * h
        theta = np.sqrt((phi * phi).sum(axis=1))
        a, b, c = so3_coefficients(theta)
        Egr, Egp, Jgr = _apply(phi, a, b, gr), _apply(phi, a, b, gp), _apply(phi, b, c, gr)
        if defect == "E_transposed":
            Egr, Egp = _apply(phi, -a, b, gr), _apply(phi, -a, b, gp)
        if defect == "Jr_identity":
            Jgr = gr
        cross = np.cross(v, Egp)
        sign = {"cross_dropped": T(0), "cross_negated": T(-1)}.get(defect, T(1))
        grad_q[:, vi:vi + 3] = Egr + sign * h * cross
        grad_q[:, vi + 3:vi + 6] = Egp
        gv[:, vi:vi + 3] = gqd[:, vi:vi + 3] + h * Jgr
        gv[:, vi + 3:vi + 6] = gqd[:, vi + 3:vi + 6] + (T(1) if defect == "dt_missing" else h) * Egp
    return grad_q, gv, h * gv


def _qmul(p, q):
    """quaternion product of [B,4] scalar-first arrays"""
    pw, pv, qw, qv = p[:, :1], p[:, 1:], q[:, :1], q[:, 1:]
    return np.concatenate([pw * qw - (pv * qv).sum(axis=1, keepdims=True), pw * qv + qw * pv + np.cross(pv, qv)], axis=1)


def _rot_t(quat):
    """R(quat)^T [B,3,3]: body axes into world axes (integrate_ref.rot_t)"""
    e0, e1, e2, e3 = quat.T
    return np.stack([1 - 2 * (e2 * e2 + e3 * e3), 2 * (e1 * e2 - e0 * e3), 2 * (e1 * e3 + e0 * e2),
                     2 * (e1 * e2 + e0 * e3), 1 - 2 * (e1 * e1 + e3 * e3), 2 * (e2 * e3 - e0 * e1),
                     2 * (e1 * e3 - e0 * e2), 2 * (e2 * e3 + e0 * e1), 1 - 2 * (e1 * e1 + e2 * e2)], axis=1).reshape(-1, 3, 3)


def tangent_plus(blob, q, d):
    """the state after the tangent step d[B, nv], all entries at once (test_gpu_parity._reference_plus, entry by entry):
    q_i += d, quat += quat x (0, d_r) / 2, p += R^T d_p"""
    nq, nv, base, pairs = layout(blob)
    q, d = np.asarray(q, dtype=np.float64), np.asarray(d, dtype=np.float64)
    out = q.copy()
    for qc, vc in pairs:
        out[:, qc] += d[:, vc]
    if base is not None:
        qi, vi = base
        quat = q[:, qi + 3:qi + 7]
        zero_d = np.concatenate([np.zeros((len(q), 1)), d[:, vi:vi + 3]], axis=1)
        out[:, qi + 3:qi + 7] = quat + 0.5 * _qmul(quat, zero_d)
        out[:, qi:qi + 3] += np.einsum("bij,bj->bi", _rot_t(quat), d[:, vi + 3:vi + 6])
    return out


def tangent_minus(blob, q_a, q_b):
    """d[B, nv], the tangent vector at q_b that leads to q_a: q_a - q_b on explicit coordinates, twice the logarithm of
    quat_b^-1 x quat_a (its rotation vector, body axes) and R_b (p_a - p_b) on the base"""
    nq, nv, base, pairs = layout(blob)
    q_a, q_b = np.asarray(q_a, dtype=np.float64), np.asarray(q_b, dtype=np.float64)
    d = np.zeros((len(q_a), nv))
    for qc, vc in pairs:
        d[:, vc] = q_a[:, qc] - q_b[:, qc]
    if base is not None:
        qi, vi = base
        qa, qb = q_a[:, qi + 3:qi + 7], q_b[:, qi + 3:qi + 7]
        rel = _qmul(qb * np.array([1.0, -1.0, -1.0, -1.0]), qa)  # (the scale of either quaternion drops out of atan2 below)
        rel = np.where(rel[:, :1] < 0, -rel, rel)
        n = np.linalg.norm(rel[:, 1:], axis=1)
        angle = 2.0 * np.arctan2(n, rel[:, 0])
        scale = np.where(n > 0, angle / np.where(n > 0, n, 1.0), 0.0)
        d[:, vi:vi + 3] = scale[:, None] * rel[:, 1:]
        d[:, vi + 3:vi + 6] = np.einsum("bji,bj->bi", _rot_t(qb), q_a[:, qi:qi + 3] - q_b[:, qi:qi + 3])
    return d


def step_vjp(integrate_vjp_fn, fd_vjp_fn, q, qd, tau, qd_next, g_q, g_qd, want=("q", "qd", "tau")):
    """The three stages of grbda_step_vjp_* over callables: integrate_vjp_fn(qd_next, g_q, g_qd) -> (i_q, i_qd, g_ydd),
    fd_vjp_fn(q, qd, tau, g_ydd) -> (a_q, a_qd, a_tau); grad_q = i_q + a_q, grad_qd = i_qd + a_qd, grad_tau = a_tau."""
    i_q, i_qd, g_ydd = integrate_vjp_fn(qd_next, g_q, g_qd)
    a_q, a_qd, a_tau = fd_vjp_fn(q, qd, tau, g_ydd)
    out = {"q": i_q + a_q, "qd": i_qd + a_qd, "tau": a_tau}
    return {k: out[k] for k in want}


def rollout_vjp(step_vjp_fn, q0, qd0, q_traj, qd_traj, tau, g_q, g_qd):
    """The loop of grbda_rollout_vjp_* over step_vjp_fn(q, qd, tau, qd_next, g_q, g_qd) -> {"q", "qd", "tau"}.  tau: [B, nv] or
    [T, B, nv]; g_q, g_qd: [B, nv] (state T only) or [T, B, nv] (states 1 .. T), either may be None.  Returns {"q", "qd", "tau"}:
    the gradients of state 0 and of tau, shaped like tau (the sum over the steps, last step first, when one tau is held)."""
    T = len(qd_traj)
    per_step_tau = tau.ndim == 3
    per_step_g = (g_q if g_q is not None else g_qd).ndim == 3
    pick = lambda g, k: None if g is None else (g[k - 1] if per_step_g else g)  # the cotangent of state k
    lam_q, lam_qd = pick(g_q, T), pick(g_qd, T)
    rows = [None] * T
    for k in range(T - 1, -1, -1):
        qk, qdk = (q0, qd0) if k == 0 else (q_traj[k - 1], qd_traj[k - 1])
        got = step_vjp_fn(qk, qdk, tau[k] if per_step_tau else tau, qd_traj[k], lam_q, lam_qd)
        rows[k] = got["tau"]
        lam_q, lam_qd = got["q"], got["qd"]
        if k >= 1 and per_step_g:
            if g_q is not None:
                lam_q = lam_q + g_q[k - 1]
            if g_qd is not None:
                lam_qd = lam_qd + g_qd[k - 1]
    if per_step_tau:
        grad_tau = rows
    else:
        grad_tau = rows[T - 1]
        for k in range(T - 2, -1, -1):
            grad_tau = grad_tau + rows[k]
    return {"q": lam_q, "qd": lam_qd, "tau": grad_tau}
