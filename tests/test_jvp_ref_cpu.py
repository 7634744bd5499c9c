"""The closed form of the integrate JVP (tests/jvp_ref.py, the yardstick of tests/test_jvp_gpu.py) against central differences of
integrate_ref.reference_step and against its transpose, step_vjp_ref.integrate_vjp; CPU only.

Central difference: the Jacobian of one step, d (q', qd') / d (q, qd, ydd) in tangent coordinates, column by column from
jvp_ref.integrate_jvp on unit tangents, against the one test_step_vjp_ref_cpu.py takes by central differences (h = 1e-6, along
tangent_plus, read back with tangent_minus; B = 8, states 0 .. 4 with |omega'| dt = 0, 1e-9, 1e-4, 1e-2, 3).  The bound is that file's
1e-7, relative to 1 + max |Jacobian entry|, for the reason given there.

Adjointness: <g', JVP(d)> = <VJP(g'), d> for random g' = (g_q', g_qd') and d = (dq, dqd, dydd), state by state, to 1e-12 |g'|_2 |d|_2:
both sides are sums of some 3 nv products of entries of size |g'| |d| |J| with |J| about 1, each rounded to 1e-16.

Every seeded defect of jvp_ref.DEFECTS breaks both."""
import numpy as np
import pytest

import integrate_ref as R
import jvp_ref as J
import step_vjp_ref as S
from test_step_vjp_ref_cpu import B, BOUND, SPECIAL_ANGLES, _err, _jacobians

ADJOINT_BOUND = 1e-12
FLOATING = [m for m in R.EXPLICIT_MODELS if S.layout(R.blob_of(m))[2] is not None]


def jacobian_by_jvp(blob, qd_next, dt, defect=None):
    """[B, 2 nv, 3 nv]: rows (d q', d qd'), columns (d q, d qd, d ydd)"""
    nv = qd_next.shape[1]
    out = np.empty((len(qd_next), 2 * nv, 3 * nv))
    for j in range(3 * nv):
        u = np.zeros((len(qd_next), nv))
        u[:, j % nv] = 1.0
        tangents = [u if j // nv == k else None for k in range(3)]
        out[:, :, j] = np.concatenate(J.integrate_jvp(blob, qd_next, dt, *tangents, defect=defect), axis=1)
    return out


def adjoint_gap(blob, qd_next, dt, defect=None):
    """max over the states of |<g', JVP(d)> - <VJP(g'), d>| / (|g'|_2 |d|_2)"""
    rng = np.random.default_rng(29)
    g = rng.uniform(-1, 1, (2,) + qd_next.shape)
    d = rng.uniform(-1, 1, (3,) + qd_next.shape)
    pushed = J.integrate_jvp(blob, qd_next, dt, *d, defect=defect)
    pulled = S.integrate_vjp(blob, qd_next, dt, g[0], g[1])
    lhs = sum((a * b).sum(axis=1) for a, b in zip(g, pushed))
    rhs = sum((a * b).sum(axis=1) for a, b in zip(pulled, d))
    norms = np.sqrt((g * g).sum(axis=(0, 2))) * np.sqrt((d * d).sum(axis=(0, 2)))
    return float((np.abs(lhs - rhs) / norms).max())


@pytest.mark.parametrize("model", R.EXPLICIT_MODELS)
def test_the_closed_form_is_the_jacobian_of_the_reference_step(model):
    blob, qd_next, dt, ref = _jacobians(model)
    assert len(qd_next) == B == 8
    base = S.layout(blob)[2]
    if base is not None:
        theta = np.linalg.norm(qd_next[:, base[1]:base[1] + 3], axis=1) * dt
        assert np.allclose(theta[:5], SPECIAL_ANGLES, rtol=1e-12, atol=0) and theta[0] == 0.0
    err = _err(jacobian_by_jvp(blob, qd_next, dt), ref)
    print(f"{model}: integrate JVP against central differences, dt = {dt}: {err:.2e} (max |J| {np.abs(ref).max():.3g})")
    assert err < BOUND


@pytest.mark.parametrize("model", R.EXPLICIT_MODELS)
def test_the_closed_form_is_the_transpose_of_the_integrate_vjp(model):
    blob, qd_next, dt, _ = _jacobians(model)
    gap = adjoint_gap(blob, qd_next, dt)
    print(f"{model}: <g', JVP(d)> against <VJP(g'), d>: {gap:.2e}")
    assert gap < ADJOINT_BOUND


@pytest.mark.parametrize("model", R.EXPLICIT_MODELS)
def test_a_tangent_that_is_none_is_zero(model):
    blob, qd_next, dt, _ = _jacobians(model)
    d = np.random.default_rng(31).uniform(-1, 1, (3,) + qd_next.shape)
    z = np.zeros_like(qd_next)
    for k in range(3):
        alone = [d[i] if i == k else None for i in range(3)]
        filled = [d[i] if i == k else z for i in range(3)]
        for a, b in zip(J.integrate_jvp(blob, qd_next, dt, *alone), J.integrate_jvp(blob, qd_next, dt, *filled)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("defect", J.DEFECTS)
@pytest.mark.parametrize("model", FLOATING)
def test_both_tests_notice_a_seeded_defect(model, defect):
    blob, qd_next, dt, ref = _jacobians(model)
    err = _err(jacobian_by_jvp(blob, qd_next, dt, defect=defect), ref)
    gap = adjoint_gap(blob, qd_next, dt, defect=defect)
    print(f"{model}: {defect}: differences {err:.2e}, adjoint {gap:.2e}")
    assert err > BOUND and gap > ADJOINT_BOUND


def test_unit_tangents_have_unit_rows():
    u = J.unit_tangent(7, 18, 3)
    assert u.shape == (7, 18) and np.allclose(np.abs(u).sum(axis=1), 1.0, rtol=1e-15)
    assert np.array_equal(u, J.unit_tangent(7, 18, 3)) and not np.array_equal(u, J.unit_tangent(7, 18, 4))
    u32 = J.unit_tangent(7, 18, 3, "f32")
    assert np.array_equal(u32, u32.astype(np.float32).astype(np.float64)) and np.abs(u32 - u).max() < 1e-7
