"""Contact-point kinematics and contact-constrained forward dynamics in numpy: the reference of test_contact_gpu.py, pinned to the oracle
by test_contact_ref_cpu.py.  A plain module that never calls the library; it is built from what is already pinned:
oracle_py.forward_dynamics (with f_ext), entry_points._mass_oracle, and kinematics_ref.frame_jacobians / body_twists / body_poses.

A contact c is the point offsets[c] (body coordinates) fixed in body bodies[c].  With E, r the body's pose (world -> body, origin in the
world), [omega; v | alpha; a] its twist halves in body axes (a carrying -gravity) and g the model's gravity:
    p      = r + E^T o
    p_dot  = E^T (v + omega x o)
    p_ddot = E^T (a + alpha x o + omega x (v + omega x o)) + g
and, with J_w [3 n, nv] = E^T times the force rows of the frame Jacobians and H the joint-space inertia:
    ydd_free = FD(q, qd, tau, f_ext)
    (J_w H^-1 J_w^T + mu I) lambda = a_des - p_ddot(ydd_free)
    ydd = ydd_free + H^-1 J_w^T lambda"""
import numpy as np

import entry_points as EP
import kinematics_ref as K
import oracle_py as O


def _poses(blob, q, bodies):
    Xa = K.body_poses(blob, q, big=EP._big(blob))[:, list(bodies)]  # [B, n, 12]
    return Xa[:, :, :9].reshape(q.shape[0], len(bodies), 3, 3), Xa[:, :, 9:]


def _to_world(E, x):
    return np.einsum("bcji,bcj->bci", E, x)  # E^T x per state and contact


def contact_points(blob, q, bodies, offsets, qd=None, ydd=None):
    """(pos, vel, acc), [B, n, 3] each in world axes; vel is None without qd, acc is None without qd and ydd"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    o = np.asarray(offsets, dtype=np.float64)[None]  # [1, n, 3]
    E, r = _poses(blob, q, bodies)
    pos = r + _to_world(E, np.broadcast_to(o, r.shape))
    if qd is None:
        return pos, None, None
    V = K.body_twists(blob, q, qd, np.zeros_like(qd) if ydd is None else ydd, big=EP._big(blob))[:, list(bodies)]
    w, v, al, a = V[:, :, 0:3], V[:, :, 3:6], V[:, :, 6:9], V[:, :, 9:12]
    u = v + np.cross(w, o)
    vel = _to_world(E, u)
    if ydd is None:
        return pos, vel, None
    g = K._parse(blob)["grav"][3:]
    acc = _to_world(E, a + np.cross(al, o) + np.cross(w, u)) + g[None, None]
    return pos, vel, acc


def world_jacobian(blob, q, bodies, offsets):
    """J_w [B, 3 n, nv]: p_dot = J_w qd"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    J = K.frame_jacobians(blob, q, list(bodies), [tuple(o) for o in offsets], big=EP._big(blob))
    E, _ = _poses(blob, q, bodies)
    n, nv = len(bodies), J.shape[2]
    Jf = J.reshape(q.shape[0], n, 6, nv)[:, :, 3:]
    return np.einsum("bcji,bcjk->bcik", E, Jf).reshape(q.shape[0], 3 * n, nv)


def wrenches(blob, q, bodies, offsets, lam, f_ext=None):
    """[B, n_bodies, 6]: f_ext (or zeros) plus the world wrenches [p x lambda_c ; lambda_c] on bodies[c]"""
    nb = K._parse(blob)["nb"]
    pos = contact_points(blob, q, bodies, offsets)[0]
    out = np.zeros((q.shape[0], nb, 6)) if f_ext is None else np.array(f_ext, dtype=np.float64)
    for c, bd in enumerate(bodies):
        out[:, bd, :3] += np.cross(pos[:, c], lam[:, c])
        out[:, bd, 3:] += lam[:, c]
    return out


def contact_dynamics(blob, q, qd, tau, bodies, offsets, a_des=None, damping=0.0, f_ext=None):
    """dict: ydd [B, nv] (closed form), lam [B, n, 3], ydd_free [B, nv], A [B, 3 n, 3 n] = J_w H^-1 J_w^T + mu I, Jw, Hinv"""
    q, qd, tau = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, qd, tau))
    B, n = q.shape[0], len(bodies)
    free = O.forward_dynamics(blob, q, qd, tau, f_ext, big=EP._big(blob))
    Jw = world_jacobian(blob, q, bodies, offsets)
    Hinv = np.linalg.inv(EP._mass_oracle(blob, q))
    A = np.einsum("bij,bjk,blk->bil", Jw, Hinv, Jw) + damping * np.eye(3 * n)[None]
    acc = contact_points(blob, q, bodies, offsets, qd, free)[2]
    rhs = (np.zeros((B, n, 3)) if a_des is None else np.asarray(a_des, dtype=np.float64)) - acc
    lam = np.linalg.solve(A, rhs.reshape(B, 3 * n, 1))[:, :, 0]
    ydd = free + np.einsum("bij,bkj,bk->bi", Hinv, Jw, lam)
    return {"ydd": ydd, "lam": lam.reshape(B, n, 3), "ydd_free": free, "A": A, "Jw": Jw, "Hinv": Hinv}


# ---- the contact sets of the tests ----------------------------------------------------------------------------------------------------
def body_index(blob, name):
    from test_gpu_parity import _body_index

    return _body_index(blob, name)


_CORNERS = [(sx * 0.1, sy * 0.05, -0.05) for sx in (1, -1) for sy in (1, -1)]
SETS = {
    # four knee links of the Mini Cheetah, the feet at the end of the shanks
    "cheetah_feet": ("urdf_mini_cheetah", ["FR_knee_link", "FL_knee_link", "HR_knee_link", "HL_knee_link"], [(0.0, 0.0, -0.2)] * 4),
    "cheetah_one": ("urdf_mini_cheetah", ["FL_knee_link"], [(0.0, 0.0, -0.2)]),
    "tello_feet": ("tello_with_arms", ["left-foot", "right-foot"], [(0.0, 0.0, -0.05)] * 2),
    # four corners of each sole of the MIT Humanoid: 8 contacts, rank 12 of 24 -- singular without damping
    "humanoid_soles": ("urdf_mit_humanoid", ["left_ankle_link"] * 4 + ["right_ankle_link"] * 4, _CORNERS * 2),
}
# the Mini Cheetah sets of test_contact_solve_gpu.py, one per contact count: up to four feet; four feet and a point of the floating-base
# body; four feet and 2, 3, 4 further points along shanks that already carry a foot (several contacts on one body: singular without damping)
_KNEES = SETS["cheetah_feet"][1]
_SHANK = [(0.03, 0.01, -0.1), (-0.02, 0.015, -0.05), (0.01, -0.02, -0.15), (0.02, 0.02, -0.12)]
for _n in range(1, 9):
    _names = _KNEES[:_n] if _n <= 4 else _KNEES + (["Floating Base"] if _n == 5 else _KNEES[: _n - 4])
    _offs = [(0.0, 0.0, -0.2)] * min(_n, 4) + ([(0.15, -0.04, 0.03)] if _n == 5 else _SHANK[: max(_n - 4, 0)])
    SETS[f"cheetah_n{_n}"] = ("urdf_mini_cheetah", _names, _offs)


def contact_set(key):
    """(model name, body indices, offsets) of SETS[key]"""
    model, names, offsets = SETS[key]
    blob = EP._model(model)
    return model, [body_index(blob, nm) for nm in names], offsets


# ---- the solve alone: what contact_solve_kernel reads, and how well its lambda solves it (test_contact_solve_gpu.py) -----------------
def solve_inputs(Linv, Xa, V, bodies, offsets, a_des, mu, g):
    """(A [B, 3 n, 3 n], rhs [B, 3 n]) of the contact solve in float64 from the arrays the kernel reads -- the header comment of
    contact_kernels.hip restated: Linv [B, 6 n, 6 n] (inv_osim), Xa [B, n_bodies, 12] (body_poses), V [B, n_bodies, 12] (body_twists at
    ydd_free), g the gravity's linear part:
        A   = R Linv_ff R^T + mu I,  R = blockdiag E_c^T, Linv_ff the force-force 3 x 3 blocks
        rhs = a_des - p_ddot,        p_ddot = E^T (a + alpha x o + omega x (v + omega x o)) + g
    The kernel factors the lower triangle (blocks c2 <= c1 of Linv_ff and, of a diagonal block's product, the entries j <= i): A is the
    symmetric matrix of that triangle, so what Linv lacks in symmetry is not charged to the solve."""
    Linv, Xa, V = (np.asarray(a, dtype=np.float64) for a in (Linv, Xa, V))
    B, n = Linv.shape[0], len(bodies)
    o = np.asarray(offsets, dtype=np.float64)[None]
    E = Xa[:, list(bodies), :9].reshape(B, n, 3, 3)
    Lff = Linv.reshape(B, n, 6, n, 6)[:, :, 3:, :, 3:]  # [B, c1, 3, c2, 3]
    A = np.einsum("bcki,bckdl,bdlj->bcidj", E, Lff, E).reshape(B, 3 * n, 3 * n)
    A = np.tril(A) + np.swapaxes(np.tril(A, -1), 1, 2) + mu * np.eye(3 * n)[None]
    W = V[:, list(bodies)]
    w, v, al, a = W[:, :, 0:3], W[:, :, 3:6], W[:, :, 6:9], W[:, :, 9:12]
    acc = _to_world(E, a + np.cross(al, o) + np.cross(w, v + np.cross(w, o))) + np.asarray(g, dtype=np.float64)[None, None]
    rhs = (np.zeros((B, n, 3)) if a_des is None else np.asarray(a_des, dtype=np.float64)) - acc
    return A, rhs.reshape(B, 3 * n)


def backward_error(A, lam, rhs):
    """|A lam - rhs|_inf / (|A|_inf |lam|_inf + |rhs|_inf) per state: small for every solve that is stable, whatever cond(A).  The
    residual is evaluated in extended precision: in float64 its own rounding is as large as the residual of a good fp64 solve."""
    A, rhs = np.asarray(A, dtype=np.longdouble), np.asarray(rhs, dtype=np.longdouble)
    lam = np.asarray(lam, dtype=np.longdouble).reshape(rhs.shape)
    res = np.abs((A * lam[:, None, :]).sum(axis=2) - rhs).max(axis=1)
    return (res / (np.abs(A).sum(axis=2).max(axis=1) * np.abs(lam).max(axis=1) + np.abs(rhs).max(axis=1))).astype(np.float64)


def cholesky_solve(A, rhs, dtype):
    """lambda [B, m] of a plain Cholesky solve carried out in `dtype` on A and rhs rounded to it (the yardstick of the kernel's solve)"""
    A, y = np.array(A, dtype=dtype), np.array(rhs, dtype=dtype)
    m = A.shape[1]
    L = np.zeros_like(A)
    for j in range(m):
        L[:, j, j] = np.sqrt(A[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(axis=1, dtype=dtype))
        for i in range(j + 1, m):
            L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1, dtype=dtype)) / L[:, j, j]
    for i in range(m):
        y[:, i] = (y[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1, dtype=dtype)) / L[:, i, i]
    for i in range(m - 1, -1, -1):
        y[:, i] = (y[:, i] - (L[:, i + 1:, i] * y[:, i + 1:]).sum(axis=1, dtype=dtype)) / L[:, i, i]
    assert y.dtype == np.dtype(dtype)
    return y


def cholesky_bound(m, dtype):
    """m (3 m + 1) u: the backward error a Cholesky solve of order m in `dtype` is bounded by (Higham, Accuracy and Stability of
    Numerical Algorithms, theorem 10.4, gamma_{3 m + 1} to first order and summed over a row for the infinity norm)"""
    return m * (3 * m + 1) * float(np.finfo(dtype).eps) / 2


def rel_per_state(got, ref):
    """|got - ref|_inf / (1 + |ref|_inf), state by state"""
    B = ref.shape[0]
    return np.abs(got - ref).reshape(B, -1).max(axis=1) / (1.0 + np.abs(ref).reshape(B, -1).max(axis=1))
