"""Test infrastructure: energy, centre of mass and centroidal momentum of a model description in plain numpy, the reference the device
outputs grbda_energy_*, grbda_centroidal_* and grbda_centroidal_matrix_* are held to.  A helper module, not a test file; nothing here
calls the library under test.

Built on the poses and twists of kinematics_ref.py (body_poses / body_twists: world pose (E, r), velocity v and acceleration a of every
body in its own coordinates, a carrying -gravity) and the parsed description's body inertias bd["I"] (6 x 6, [angular; linear]).  Per body,
with m = I[3, 3], h = m c read from the block m c x of I and l = I v = [n; p]:
    KE   += 1/2 v . l
    mc_w += m r + E^T h
    P    += E^T p                      h_O += E^T n + r x (E^T p)
    f     = I a + v x* l
    F    += E^T f_lin                  N_O += E^T f_ang + r x (E^T f_lin)
and then, with M the total mass and g the description's gravity:
    c = mc_w / M      c_dot = P / M        h_G = h_O - c x P
    PE = -g . mc_w    P_dot = F + M g      h_G_dot = N_O + mc_w x g - c x P_dot
tests/test_centroidal_ref_cpu.py pins the module to the oracle: KE = 1/2 yd^T H yd, A yd = h, and the momentum balance with the oracle's
forward dynamics.

dtype = np.float32 runs the same summation -- about the world origin, then shifted to the centre of mass -- in single precision on the
same inputs: what single precision itself costs, the yardstick of term_states.within_float, never the reference of a comparison."""
import numpy as np

import kinematics_ref as K

OUTPUTS = ("kinetic", "potential", "com", "com_vel", "h", "hdot")


def total_mass(blob):
    return float(sum(bd["I"][3, 3] for bd in K._parse(blob)["bodies"]))


def _to_world(E, x):
    return np.einsum("bji,bj->bi", E, x)


def _sums(kin, v=None, a=None):
    """the sums of the module docstring over the bodies of kin: a dict of [B] / [B, 3] arrays in kin.dtype"""
    B, dt = kin.B, kin.dtype
    out = {k: np.zeros((B, 3), dtype=dt) for k in ("mc", "P", "hO", "F", "NO")}
    out["KE"] = np.zeros(B, dtype=dt)
    out["M"] = dt(0)
    for b, bd in enumerate(kin.m["bodies"]):
        I = bd["I"].astype(dt)
        E, r = kin.E[b], kin.r[b]
        m, mcb = I[3, 3], np.array([I[2, 4], I[0, 5], I[1, 3]], dtype=dt)  # c x: (2, 1) = c_x, (0, 2) = c_y, (1, 0) = c_z
        out["M"] = out["M"] + m
        out["mc"] += m * r + E.transpose(0, 2, 1) @ mcb
        if v is None:
            continue
        l = v[:, b] @ I.T
        out["KE"] += dt(0.5) * np.einsum("bi,bi->b", v[:, b], l)
        p_w = _to_world(E, l[:, 3:])
        out["P"] += p_w
        out["hO"] += _to_world(E, l[:, :3]) + np.cross(r, p_w)
        if a is None:
            continue
        f = a[:, b] @ I.T + K._mv(K.crf_b(v[:, b]), l)
        f_w = _to_world(E, f[:, 3:])
        out["F"] += f_w
        out["NO"] += _to_world(E, f[:, :3]) + np.cross(r, f_w)
    return out


def _finish(kin, s, have_v, have_a):
    dt = kin.dtype
    g = kin.m["grav"][3:].astype(dt)
    M = s["M"]
    c = s["mc"] / M
    out = {"mass": float(M), "potential": -(s["mc"] @ g), "com": c}
    if have_v:
        out["kinetic"] = s["KE"]
        out["com_vel"] = s["P"] / M
        out["h"] = np.concatenate([s["hO"] - np.cross(c, s["P"]), s["P"]], axis=1)
    if have_a:
        Pd = s["F"] + M * g
        out["hdot"] = np.concatenate([s["NO"] + np.cross(s["mc"], g) - np.cross(c, Pd), Pd], axis=1)
    return out


def centroidal(blob, q, qd=None, ydd=None, big=False, dtype=np.float64):
    """dict of mass, potential[B], com[B, 3]; with qd also kinetic[B], com_vel[B, 3], h[B, 6]; with qd and ydd also hdot[B, 6]
    (world axes; h and hdot [angular about the centre of mass; linear]).  The arrays are of `dtype`."""
    kin = K._Kin(blob, q, big, dtype)
    v = a = None
    if qd is not None:
        vs, as_ = kin.rates(qd, np.zeros_like(qd) if ydd is None else ydd)
        v, a = kin.propagate(vs, None if ydd is None else as_)
    return _finish(kin, _sums(kin, v, a), v is not None, a is not None)


def momentum_matrix(blob, q, big=False):
    """A[B, 6, nv], h = A yd: column k is the h of (q, e_k)"""
    kin = K._Kin(blob, q, big)
    nv = kin.m["nv"]
    A = np.zeros((kin.B, 6, nv))
    for cl, at, (G, _) in zip(kin.m["clusters"], kin.span_at, kin.maps()):
        vi, n, nsv = cl[5], cl[6], cl[8]
        for k in range(n):
            vs = np.zeros((kin.B, kin.n_span))
            vs[:, at:at + nsv] = G[:, :, k]
            v, _ = kin.propagate(vs)
            A[:, :, vi + k] = _finish(kin, _sums(kin, v), True, False)["h"]
    return A


def wrench_about(com, f_ext):
    """the sum of the world-frame wrenches f_ext[B, n_bodies, 6] ([moment about the world origin; force]) taken about com[B, 3]"""
    n, f = f_ext[:, :, :3].sum(axis=1), f_ext[:, :, 3:].sum(axis=1)
    return np.concatenate([n - np.cross(com, f), f], axis=1)


def scale_error(got, ref):
    """per state, on the quantity's own scale: |got - ref|_inf / (1 + |ref|_inf of that state) -> [B]"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    B = ref.shape[0]
    return np.abs(got - ref).reshape(B, -1).max(axis=1) / (1.0 + np.abs(ref).reshape(B, -1).max(axis=1))
