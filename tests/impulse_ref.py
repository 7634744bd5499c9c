"""Contact impulses in numpy: the reference of test_impulse_gpu.py and test_impulse_solve_gpu.py, pinned by test_impulse_ref_cpu.py.  A
plain module that never calls the library; it is built from what is already pinned: contact_ref.world_jacobian / contact_points,
entry_points._mass_oracle and oracle_py.

With J_w [3 n, nv] the world-frame Jacobian of the points, v- = J_w qd, H the joint-space inertia, e the restitution, mu the damping:
    (J_w H^-1 J_w^T + mu I) Lambda = v_des - (1 + e) v-
    qd_next = qd + H^-1 J_w^T Lambda
so that J_w qd_next = v_des - e v- - mu Lambda.  Gravity and tau do not enter: H is taken from the description with its gravity set to
zero (entry_points._mass_oracle subtracts two inverse dynamics that both hold gravity, which moves H by some 1e-14 with it), so the
arrays returned are the same bit for bit at every gravity (test_contact_refs_gravity_cpu.py)."""
import functools

import numpy as np

import contact_ref as C
import entry_points as EP


def without_gravity(blob):
    """the description with its gravity (six doubles at byte 48, as kinematics_ref._parse reads them) set to zero"""
    out = bytes(blob[:48]) + bytes(48) + bytes(blob[96:])
    assert len(out) == len(blob) and not C.K._parse(out)["grav"].any()
    if EP._big(blob):
        EP._BIG.add(out)
    return out


def contact_impulse(blob, q, qd, bodies, offsets, v_des=None, e=0.0, mu=0.0):
    """dict: qd_next [B, nv], impulse [B, n, 3], A [B, 3 n, 3 n] = J_w H^-1 J_w^T + mu I, Jw, Hinv, H, v_minus [B, n, 3] -- by dense
    numpy.linalg.solve in float64"""
    q, qd = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, qd))
    B, n = q.shape[0], len(bodies)
    Jw = C.world_jacobian(blob, q, bodies, offsets)
    H = EP._mass_oracle(without_gravity(blob), q)
    Hinv = np.linalg.inv(H)
    A = np.einsum("bij,bjk,blk->bil", Jw, Hinv, Jw) + mu * np.eye(3 * n)[None]
    v_minus = np.einsum("bij,bj->bi", Jw, qd)
    want = np.zeros((B, 3 * n)) if v_des is None else np.asarray(v_des, dtype=np.float64).reshape(B, 3 * n)
    lam = np.linalg.solve(A, (want - (1.0 + e) * v_minus)[:, :, None])[:, :, 0]
    qd_next = qd + np.einsum("bij,bkj,bk->bi", Hinv, Jw, lam)
    return {"qd_next": qd_next, "impulse": lam.reshape(B, n, 3), "A": A, "Jw": Jw, "Hinv": Hinv, "H": H, "v_minus": v_minus.reshape(B, n, 3)}


def contact_impulse_in(dtype, ref, qd, v_des=None, e=0.0, mu=0.0):
    """(qd_next, impulse) of the same closed form carried out in `dtype` on ref's Jw and H rounded to it: what working precision alone
    costs on these inputs (the fp32 yardstick of test_impulse_gpu.py)"""
    Jw, H, qd = (np.asarray(a, dtype=dtype) for a in (ref["Jw"], ref["H"], qd))
    B, m = Jw.shape[0], Jw.shape[1]
    Hinv = np.linalg.inv(H).astype(dtype)
    A = (np.einsum("bij,bjk,blk->bil", Jw, Hinv, Jw) + dtype(mu) * np.eye(m, dtype=dtype)[None]).astype(dtype)
    v_minus = np.einsum("bij,bj->bi", Jw, qd).astype(dtype)
    want = np.zeros((B, m), dtype=dtype) if v_des is None else np.asarray(v_des, dtype=dtype).reshape(B, m)
    lam = C.cholesky_solve(A, want - dtype(1.0 + e) * v_minus, dtype)
    qd_next = (qd + np.einsum("bij,bkj,bk->bi", Hinv, Jw, lam)).astype(dtype)
    return qd_next, lam.reshape(B, m // 3, 3)


def kinetic(H, qd):
    """1/2 qd^T H qd per state"""
    return 0.5 * np.einsum("bi,bij,bj->b", qd, H, qd)


# ---- the cases of the GPU tests (test_impulse_ref_cpu.py holds the reference on every one of them) ------------------------------------
SEED = 73  # of entry_points._states and of the v_des draws
B_TOP = 130
# (id, model, plan-time switches, contact set of contact_ref.SETS or None = test_contact_gpu.points_of(model), damping, restitution,
#  random v_des)
CASES = [
    ("cheetah_n1", "urdf_mini_cheetah", (), "cheetah_n1", 0.0, 0.0, False),
    ("cheetah_n3", "urdf_mini_cheetah", (), "cheetah_n3", 0.0, 0.25, True),
    ("cheetah_n5", "urdf_mini_cheetah", (), "cheetah_n5", 0.0, 1.0, False),
    ("cheetah_n8", "urdf_mini_cheetah", (), "cheetah_n8", 1e-3, 0.5, True),
    ("cheetah_feet", "urdf_mini_cheetah", (), "cheetah_feet", 0.0, 0.0, True),
    ("tello_feet", "tello_with_arms", (), "tello_feet", 0.0, 0.0, True),
    ("cheetah_rpy2", "urdf_mini_cheetah_rpy", (), None, 0.0, 0.5, True),
    ("two_parent1", "two_parent", (), None, 0.0, 0.0, True),
    ("humanoid_soles", "urdf_mit_humanoid", (), "humanoid_soles", 1e-3, 0.0, False),
    ("chain1_damped", "rev_rotor_chain_4", (), None, 1e-3, 0.0, False),
]
CASE = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case(cid, rounded=False):
    """(blob, bodies, offsets, (q, qd, v_des or None), mu, e, contact_impulse(...)) of B_TOP states, computed once per process and
    never written to; `rounded`: every input rounded to float32 first (the reference stays float64)"""
    import term_states as TS
    from test_contact_gpu import points_of

    _, name, env, key, mu, e, rand = CASE[cid]
    blob = EP._model(name)
    bodies, offsets = C.contact_set(key)[1:] if key else points_of(name)
    rnd = TS.fp32_rounded if rounded else (lambda a: a)
    q, qd, _ = (TS._frozen(rnd(a)) for a in EP._states(blob, B_TOP, SEED))
    vd = TS._frozen(rnd(np.random.default_rng(SEED).uniform(-1, 1, (B_TOP, len(bodies), 3)))) if rand else None
    return blob, list(bodies), [tuple(o) for o in offsets], (q, qd, vd), mu, e, contact_impulse(blob, q, qd, bodies, offsets, vd, e, mu)


def solve_inputs(Linv, Xa, V, bodies, offsets, v_des, e, mu):
    """(A [B, 3 n, 3 n], rhs [B, 3 n]) of the impulse solve in float64 from the arrays impulse_solve_kernel reads -- Linv [B, 6 n, 6 n]
    (inv_osim), Xa [B, n_bodies, 12] (body_poses), V [B, n_bodies, 12] (body_twists; the velocity halves only):
        A   = R Linv_ff R^T + mu I    (contact_ref.solve_inputs: the symmetric matrix of the lower triangle the kernel factors)
        rhs = v_des - (1 + e) p_dot,  p_dot = E^T (v + omega x o)"""
    Xa, V = (np.asarray(a, dtype=np.float64) for a in (Xa, V))
    B, n = Xa.shape[0], len(bodies)
    A = C.solve_inputs(Linv, Xa, np.zeros_like(V), bodies, offsets, None, mu, np.zeros(3))[0]
    o = np.asarray(offsets, dtype=np.float64)[None]
    E = Xa[:, list(bodies), :9].reshape(B, n, 3, 3)
    W = V[:, list(bodies)]
    vel = C._to_world(E, W[:, :, 3:6] + np.cross(W[:, :, 0:3], o))
    rhs = (np.zeros((B, n, 3)) if v_des is None else np.asarray(v_des, dtype=np.float64)) - (1.0 + e) * vel
    return A, rhs.reshape(B, 3 * n)
