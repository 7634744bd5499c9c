"""CPU reference of the Jacobian-vector products (a helper module, not a test file; nothing here calls the library): the forward map of
one integrate step in numpy, the closed form of include/grbda_hip_jvp.h, built on step_vjp_ref.layout / so3_coefficients.

With omega' = qd'[base 0..2], v' = qd'[base 3..5], phi = omega' dt, theta = |phi|, E^T = I - a [phi]x + b [phi]x^2 and
J_r = I - b [phi]x + c [phi]x^2 (the transposes of what step_vjp_ref.integrate_vjp applies), the tangents (dq, dqd, dydd) go to
    dqd'  = dqd + dt dydd
    d'    = d + dt dqd'                                explicit coordinates
    d_r'  = E^T d_r + dt J_r domega'                   base rotation
    d_p'  = E^T (d_p - dt [v']x d_r + dt dv')          base position
Every position tangent is [B, nv], along the tangent step of grbda_fd_dq_* (step_vjp_ref.tangent_plus)."""
import numpy as np

from step_vjp_ref import _apply, layout, so3_coefficients

DEFECTS = ("E_not_transposed", "Jr_identity", "cross_dropped", "cross_negated", "dt_missing")


def integrate_jvp(blob, qd_next, dt, dq=None, dqd=None, dydd=None, dtype=np.float64, defect=None):
    """(dq_next, dqd_next), each [B, nv], in `dtype` arithmetic; a tangent that is None is zero.  defect: one of DEFECTS, a deliberately
    wrong formula (test_jvp_ref_cpu.py shows that the difference test and the adjoint test notice each)."""
    assert defect is None or defect in DEFECTS
    nq, nv, base, pairs = layout(blob)
    T = np.dtype(dtype).type
    qn = np.asarray(qd_next, dtype=dtype)
    d, dv, da = (np.zeros_like(qn) if a is None else np.asarray(a, dtype=dtype) for a in (dq, dqd, dydd))
    h = T(dt)
    vn = dv + h * da
    out = d + h * vn
    if base is not None:
        vi = base[1]
        w, v = qn[:, vi:vi + 3], qn[:, vi + 3:vi + 6]
        dr, dp = d[:, vi:vi + 3], d[:, vi + 3:vi + 6]
        dw, dl = vn[:, vi:vi + 3], vn[:, vi + 3:vi + 6]
        phi = w * h
        theta = np.sqrt((phi * phi).sum(axis=1))
        a, b, c = so3_coefficients(theta)
        ea = a if defect == "E_not_transposed" else -a
        Jdw = dw if defect == "Jr_identity" else _apply(phi, -b, c, dw)
        sign = {"cross_dropped": T(0), "cross_negated": T(-1)}.get(defect, T(1))
        out[:, vi:vi + 3] = _apply(phi, ea, b, dr) + h * Jdw
        out[:, vi + 3:vi + 6] = _apply(phi, ea, b, dp - sign * h * np.cross(v, dr) + (T(1) if defect == "dt_missing" else h) * dl)
    return out, vn


def unit_tangent(B, nv, seed, dt="f64"):
    """u[B, nv], every row of unit 1-norm (then rounded to the type): the mirror of test_vjp_gpu.unit_cotangent on another stream of
    the generator"""
    u = np.random.default_rng([seed, 1066]).uniform(-1, 1, (B, nv))
    u /= np.abs(u).sum(axis=1, keepdims=True)
    return u if dt == "f64" else u.astype(np.float32).astype(np.float64)
