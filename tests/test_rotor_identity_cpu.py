"""The closed form of the axisymmetric rotor (chain_kernels.hip, rotor_terms), proved in numpy and fp64 without any kernel.

A rotor whose spatial inertia I is invariant under rotation about its joint axis z hangs off a body that moves with vp; X0 is its tree
transform, om its rate, w = X0 vp, v = w + om z, c = v x (om z), h = I z.  What the articulated-body algorithm takes from it is the
joint-space bias b = z . (pA + I c) and the force tp = X0^T (pA + I c) on the parent, pA = v x* I v.  The kernels use

    b  = 0
    tp = vp x* (X0^T I X0) vp + om (vp x* X0^T h)

Both sides are evaluated from their definitions with dense 6 x 6 matrices (Featherstone's crm / crf, no packed storage, nothing shared
with the kernels' code).  Bound: 1e-12 relative to |tp| -- about 100 fp64 operations of 1.1e-16 each, derived, not measured."""
import numpy as np

N_CASES = 100
TOL = 1e-12
Z = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def crm(v):
    """motion cross product matrix: crm(v) u = v x u"""
    out = np.zeros((6, 6))
    out[:3, :3] = skew(v[:3])
    out[3:, :3] = skew(v[3:])
    out[3:, 3:] = skew(v[:3])
    return out


def crf(v):
    """force cross product matrix: crf(v) f = v x* f"""
    return -crm(v).T


def xform(E, r):
    """motion transform of the frame rotated by E and moved by r: [[E, 0], [-E r^, E]]"""
    X = np.zeros((6, 6))
    X[:3, :3] = E
    X[3:, 3:] = E
    X[3:, :3] = -E @ skew(r)
    return X


def inertia(I3, m, com):
    """spatial inertia about the frame origin of a body with rotational inertia I3 about its centre of mass `com`"""
    C = skew(com)
    out = np.zeros((6, 6))
    out[:3, :3] = I3 + m * C @ C.T
    out[:3, 3:] = m * C
    out[3:, :3] = m * C.T
    out[3:, 3:] = m * np.eye(3)
    return out


def random_rotation(rng):
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def draw(rng, transverse_ratio=1.0):
    """(I, X0, vp, om): inertia (A, A * transverse_ratio, B, m, c_z) about z, a random tree transform, parent velocity and rotor rate"""
    A, B, m, cz = rng.uniform(1e-4, 5e-3), rng.uniform(1e-4, 5e-3), rng.uniform(0.02, 0.2), rng.uniform(-0.05, 0.05)
    I = inertia(np.diag([A, A * transverse_ratio, B]), m, np.array([0.0, 0.0, cz]))
    X0 = xform(random_rotation(rng), rng.uniform(-0.5, 0.5, 3))
    return I, X0, rng.uniform(-1.0, 1.0, 6), rng.uniform(-30.0, 30.0)


def from_definition(I, X0, vp, om):
    """(b, tp) as the algorithm states them: the rotor evaluated in its own frame"""
    v = X0 @ vp + om * Z
    c = crm(v) @ (om * Z)
    t = crf(v) @ (I @ v) + I @ c
    return Z @ t, X0.T @ t


def closed_form(I, X0, vp, om):
    return 0.0, crf(vp) @ (X0.T @ I @ X0 @ vp) + om * (crf(vp) @ (X0.T @ (I @ Z)))


def test_axisymmetric_rotor_identity():
    rng = np.random.default_rng(7)
    worst_b = worst_tp = 0.0
    for _ in range(N_CASES):
        I, X0, vp, om = draw(rng)
        # the premises: z x* I = I z x (invariance under rotation about z), I z = B z
        assert np.abs(crf(Z) @ I - I @ crm(Z)).max() <= 1e-15 * np.abs(I).max()
        assert np.abs(I @ Z - I[2, 2] * Z).max() == 0.0
        b, tp = from_definition(I, X0, vp, om)
        b0, tp0 = closed_form(I, X0, vp, om)
        scale = np.abs(tp).max()
        assert scale > 0
        worst_b = max(worst_b, abs(b - b0) / scale)
        worst_tp = max(worst_tp, np.abs(tp - tp0).max() / scale)
    print(f"rotor identity over {N_CASES} cases: |b| / |tp| <= {worst_b:.2e}, |tp - closed form| / |tp| <= {worst_tp:.2e}")
    assert worst_b <= TOL and worst_tp <= TOL


def test_quadratic_term_is_the_parents_bias_force_with_the_folded_inertia():
    """where the first term of tp goes: the parent's bias force v x* (I_body + X0^T I X0) v is its own plus exactly that term"""
    rng = np.random.default_rng(8)
    for _ in range(N_CASES):
        I, X0, vp, om = draw(rng)
        A = rng.normal(size=(3, 3))
        Ib = inertia(A @ A.T * 0.05 + np.eye(3) * 1e-2, rng.uniform(0.2, 2.0), rng.uniform(-0.3, 0.3, 3))
        folded = crf(vp) @ ((Ib + X0.T @ I @ X0) @ vp)
        _, tp = from_definition(I, X0, vp, om)
        total = crf(vp) @ (Ib @ vp) + tp
        linear = om * (crf(vp) @ (X0.T @ (I @ Z)))
        assert np.abs(total - (folded + linear)).max() <= TOL * np.abs(total).max()


def test_a_rotor_that_is_not_axisymmetric_violates_it():
    """the test can fail: transverse inertias 1 % apart break the identity by more than 1e-3 of |tp|"""
    rng = np.random.default_rng(9)
    worst = 0.0
    for _ in range(N_CASES):
        I, X0, vp, om = draw(rng, transverse_ratio=1.01)
        b, tp = from_definition(I, X0, vp, om)
        b0, tp0 = closed_form(I, X0, vp, om)
        worst = max(worst, abs(b - b0) / np.abs(tp).max(), np.abs(tp - tp0).max() / np.abs(tp).max())
    print(f"transverse inertias 1 % apart: the identity is off by {worst:.2e} of |tp|")
    assert worst > 1e-3
