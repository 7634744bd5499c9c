"""Scheduled contacts in numpy: the reference of test_contact_step_gpu.py, pinned by test_contact_step_ref_cpu.py.  A helper module, not a
test file, and it never calls the library.  Nothing new is derived here: the states of a batch are grouped by their mask, and every group
goes through the references that are already pinned -- contact_ref.contact_dynamics / impulse_ref.contact_impulse on the SUB-LIST of the
group's closed contacts, oracle_py.forward_dynamics and an unchanged qd for the group whose set is empty -- and the step is composed with
integrate_ref.reference_step.

    contact_dynamics_active   a_des - kd p_dot handed to contact_ref.contact_dynamics as its a_des (p_dot from contact_ref.contact_points)
    contact_impulse_active    impulse_ref.contact_impulse per group
    contact_step              closing = active & ~prev: the impact on (closing ? active : 0) with v_des = 0, the dynamics at the
                              velocities after it with a_des = 0, one reference_step"""
import numpy as np

import contact_ref as C
import entry_points as EP
import impulse_ref as IR
import integrate_ref as R
import oracle_py as O


def groups(active, n):
    """[(mask, state indices, closed contacts)] of the masks that occur, bits at n and above ignored"""
    masks = np.asarray(active).astype(np.int64) & ((1 << n) - 1)
    return [(int(m), np.nonzero(masks == m)[0], [c for c in range(n) if (int(m) >> c) & 1]) for m in np.unique(masks)]


def contact_dynamics_active(blob, q, qd, tau, bodies, offsets, active, a_des=None, kd=0.0, damping=0.0):
    """dict: ydd [B, nv], lam [B, n, 3] (zero off the set), ydd_free [B, nv]"""
    q, qd, tau = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, qd, tau))
    B, n = q.shape[0], len(bodies)
    free = O.forward_dynamics(blob, q, qd, tau, None, big=EP._big(blob))
    ydd, lam = free.copy(), np.zeros((B, n, 3))
    for _, idx, on in groups(active, n):
        if not on:
            continue
        bod, off = [bodies[c] for c in on], [offsets[c] for c in on]
        want = np.zeros((len(idx), len(on), 3)) if a_des is None else np.asarray(a_des, dtype=np.float64)[np.ix_(idx, on)]
        if kd:
            want = want - kd * C.contact_points(blob, q[idx], bod, off, qd[idx])[1]
        r = C.contact_dynamics(blob, q[idx], qd[idx], tau[idx], bod, off, want, damping)
        ydd[idx] = r["ydd"]
        lam[np.ix_(idx, on)] = r["lam"]
    return {"ydd": ydd, "lam": lam, "ydd_free": free}


def contact_impulse_active(blob, q, qd, bodies, offsets, active, v_des=None, e=0.0, mu=0.0):
    """dict: qd_next [B, nv] (qd itself where the set is empty), impulse [B, n, 3] (zero off the set)"""
    q, qd = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, qd))
    B, n = q.shape[0], len(bodies)
    qd_next, imp = qd.copy(), np.zeros((B, n, 3))
    for _, idx, on in groups(active, n):
        if not on:
            continue
        vd = None if v_des is None else np.asarray(v_des, dtype=np.float64)[np.ix_(idx, on)]
        r = IR.contact_impulse(blob, q[idx], qd[idx], [bodies[c] for c in on], [offsets[c] for c in on], vd, e, mu)
        qd_next[idx] = r["qd_next"]
        imp[np.ix_(idx, on)] = r["impulse"]
    return {"qd_next": qd_next, "impulse": imp}


def impact_masks(active, prev_active, n):
    """the contacts a step solves its impact with: every closed one where any closes, none elsewhere"""
    a = np.asarray(active).astype(np.int64) & ((1 << n) - 1)
    return np.where((a & ~np.asarray(prev_active).astype(np.int64)) != 0, a, 0)


def contact_step(blob, q, qd, tau, bodies, offsets, active, prev_active, kd, e, damping, dt):
    """dict: q_next, qd_next, ok, phi (integrate_ref.reference_step), ydd, lam, ydd_free, qd_plus, impulse (None without prev_active)"""
    qd_plus, imp = np.ascontiguousarray(qd, dtype=np.float64), None
    if prev_active is not None:
        r = contact_impulse_active(blob, q, qd, bodies, offsets, impact_masks(active, prev_active, len(bodies)), None, e, damping)
        qd_plus, imp = r["qd_next"], r["impulse"]
    out = contact_dynamics_active(blob, q, qd_plus, tau, bodies, offsets, active, None, kd, damping)
    qn, vn, ok, phi = R.reference_step(blob, q, qd_plus, out["ydd"], dt, big=EP._big(blob))
    out.update(q_next=qn, qd_next=vn, ok=ok, phi=phi, qd_plus=qd_plus, impulse=imp)
    return out


def shuffled_masks(B, n, seed=0):
    """state b gets mask b mod 2^n, shuffled with a fixed seed: every wavefront mixes empty, partial and full sets"""
    m = (np.arange(B) % (1 << n)).astype(np.int32)
    np.random.default_rng(seed).shuffle(m)
    return m
