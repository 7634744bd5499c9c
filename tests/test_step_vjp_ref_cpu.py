"""The closed form of the integrate VJP (tests/step_vjp_ref.py, the yardstick of tests/test_step_vjp_gpu.py) against central differences of
integrate_ref.reference_step, and Plan.tangent_cotangent against differences of the tangent step; CPU only.

The whole Jacobian of one step, d (q', qd') / d (q, qd, ydd) in tangent coordinates, is built twice per state: row by row from
step_vjp_ref.integrate_vjp on unit cotangents, and column by column from central differences (h = 1e-6) taken along tangent_plus and
read back with tangent_minus.  The bound is 1e-7 relative to 1 + max |Jacobian entry|: the rounding of a central difference is about
eps / h = 2e-10 times the size of the entries of q' (below 100 here), and 1e-7 leaves a factor of five.  States 0 .. 4 of every model
carry |omega'| dt = 0, 1e-9, 1e-4, 1e-2 and 3 (near pi).

Measured (this file, float64; max |Jacobian entry| is 1 on all three models): rev_rotor_chain_3 7.0e-11, urdf_mini_cheetah 3.7e-10,
tree_generic_float 3.7e-10; tangent_cotangent at most 3.1e-11.  The seeded defects, the smaller figure of the two floating-base models:
E transposed 2.3e-1, J_r replaced by I 1.2e-1, the [v']x term dropped 1.4e-1, negated 2.9e-1, a missing dt 3.8e-1.  The float32 run of
the reference stays within 2.0e-7 of its float64 run."""
import numpy as np
import pytest

import generalized_rbda_amd as G
import integrate_ref as R
import step_vjp_ref as S

H = 1e-6
BOUND = 1e-7
SPECIAL_ANGLES = (0.0, 1e-9, 1e-4, 1e-2, 3.0)
B = 8


def special_states(model, n=B):
    """(q, qd, ydd) of integrate_ref.states_of with the base's angular velocity of states 0 .. 4 set so that |omega'| dt is one of
    SPECIAL_ANGLES after the step (omega' = qd + dt ydd: the acceleration entries are zeroed there)"""
    blob = R.blob_of(model)
    q, qd, ydd = (a.copy() for a in R.states_of(model, n))
    base = S.layout(blob)[2]
    if base is not None:
        vi = base[1]
        axes = np.random.default_rng(11).normal(size=(len(SPECIAL_ANGLES), 3))
        axes /= np.linalg.norm(axes, axis=1, keepdims=True)
        for b, angle in enumerate(SPECIAL_ANGLES):
            ydd[b, vi:vi + 3] = 0.0
            qd[b, vi:vi + 3] = axes[b] * (angle / R.dt_of(model))
    return blob, q, qd, ydd


def jacobian_by_differences(blob, q, qd, ydd, dt):
    """[B, 2 nv, 3 nv]: rows (d q', d qd'), columns (d q, d qd, d ydd)"""
    nv = qd.shape[1]
    q0, v0 = R.reference_step(blob, q, qd, ydd, dt)[:2]
    J = np.empty((len(q), 2 * nv, 3 * nv))
    for j in range(3 * nv):
        side = []
        for s in (+H, -H):
            d = np.zeros((len(q), nv))
            d[:, j % nv] = s
            args = (S.tangent_plus(blob, q, d), qd, ydd) if j < nv else (q, qd + d, ydd) if j < 2 * nv else (q, qd, ydd + d)
            qn, vn = R.reference_step(blob, *args, dt)[:2]
            side.append(np.concatenate([S.tangent_minus(blob, qn, q0), vn - v0], axis=1))
        J[:, :, j] = (side[0] - side[1]) / (2 * H)
    return J


def jacobian_by_vjp(blob, qd_next, dt, defect=None):
    nv = qd_next.shape[1]
    J = np.empty((len(qd_next), 2 * nv, 3 * nv))
    for i in range(2 * nv):
        g = np.zeros((len(qd_next), nv))
        g[:, i % nv] = 1.0
        got = S.integrate_vjp(blob, qd_next, dt, g if i < nv else None, g if i >= nv else None, defect=defect)
        J[:, i, :] = np.concatenate(got, axis=1)
    return J


_cache = {}


def _jacobians(model):
    if model not in _cache:
        blob, q, qd, ydd = special_states(model)
        dt = R.dt_of(model)
        _cache[model] = (blob, R.reference_step(blob, q, qd, ydd, dt)[1], dt, jacobian_by_differences(blob, q, qd, ydd, dt))
    return _cache[model]


def _err(J, ref):
    return float(np.abs(J - ref).max() / (1.0 + np.abs(ref).max()))


@pytest.mark.parametrize("model", R.EXPLICIT_MODELS)
def test_the_closed_form_is_the_jacobian_of_the_reference_step(model):
    blob, qd_next, dt, ref = _jacobians(model)
    base = S.layout(blob)[2]
    if base is not None:
        theta = np.linalg.norm(qd_next[:, base[1]:base[1] + 3], axis=1) * dt
        assert np.allclose(theta[:5], SPECIAL_ANGLES, rtol=1e-12, atol=0) and theta[0] == 0.0
    err = _err(jacobian_by_vjp(blob, qd_next, dt), ref)
    print(f"{model}: integrate VJP against central differences, dt = {dt}: {err:.2e} (max |J| {np.abs(ref).max():.3g})")
    assert err < BOUND


@pytest.mark.parametrize("defect", S.DEFECTS)
@pytest.mark.parametrize("model", [m for m in R.EXPLICIT_MODELS if S.layout(R.blob_of(m))[2] is not None])
def test_the_difference_test_notices_a_seeded_defect(model, defect):
    blob, qd_next, dt, ref = _jacobians(model)
    err = _err(jacobian_by_vjp(blob, qd_next, dt, defect=defect), ref)
    print(f"{model}: {defect}: {err:.2e}")
    assert err > BOUND


def test_the_float32_reference_follows_the_float64_one():
    blob, qd_next, dt, _ = _jacobians("urdf_mini_cheetah")
    g = np.random.default_rng(5).uniform(-1, 1, (2,) + qd_next.shape)
    v32 = qd_next.astype(np.float32)
    got = S.integrate_vjp(blob, v32, dt, g[0].astype(np.float32), g[1].astype(np.float32), dtype=np.float32)
    want = S.integrate_vjp(blob, v32.astype(np.float64), dt, g[0].astype(np.float32).astype(np.float64), g[1].astype(np.float32).astype(np.float64))
    assert all(a.dtype == np.float32 for a in got)
    err = max(float(np.abs(a - b).max() / (1.0 + np.abs(b).max())) for a, b in zip(got, want))
    print(f"float32 reference against float64: {err:.2e}")
    assert err < 1e-5


@pytest.mark.parametrize("model", R.EXPLICIT_MODELS)
def test_tangent_plus_and_minus_are_inverse_to_second_order(model):
    blob, q, _, _ = special_states(model)
    d = np.random.default_rng(3).uniform(-1, 1, (len(q), S.layout(blob)[1])) * 1e-4
    back = S.tangent_minus(blob, S.tangent_plus(blob, q, d), q)
    assert np.abs(back - d).max() < 1e-11  # (third order in |d| on the base, rounding elsewhere)


def test_tangent_plus_agrees_with_the_parity_tests_entry_by_entry():
    from generalized_rbda_amd.states import parse_clusters
    from test_gpu_parity import _reference_plus

    for model in R.EXPLICIT_MODELS:
        blob, q, _, _ = special_states(model)
        q = q[:3]
        m = parse_clusters(blob)
        for k in range(m["nv"]):
            d = np.zeros((len(q), m["nv"]))
            d[:, k] = 0.37
            want = np.stack([_reference_plus(m, q[b], k, 0.37) for b in range(len(q))])
            assert np.abs(S.tangent_plus(blob, q, d) - want).max() < 1e-15, (model, k)  # (einsum against @: the last bit)


@pytest.mark.parametrize("model", R.EXPLICIT_MODELS)
def test_tangent_cotangent_is_the_pull_back_through_the_tangent_step(model):
    """<g, d tangent_plus(q, d) / d d_i at d = 0> by central differences, for an ambient cotangent g[B, nq], on CPU tensors"""
    import torch

    blob, q, _, _ = special_states(model)
    plan = G.Plan(blob)
    g = np.random.default_rng(7).uniform(-1, 1, q.shape)
    got = plan.tangent_cotangent(torch.as_tensor(q), torch.as_tensor(g)).numpy()
    assert got.shape == (len(q), plan.nv)
    ref = np.empty_like(got)
    for i in range(plan.nv):
        d = np.zeros((len(q), plan.nv))
        d[:, i] = H
        ref[:, i] = ((S.tangent_plus(blob, q, d) - S.tangent_plus(blob, q, -d)) * g).sum(axis=1) / (2 * H)
    err = float(np.abs(got - ref).max() / (1.0 + np.abs(ref).max()))
    print(f"{model}: tangent_cotangent against central differences: {err:.2e}")
    assert err < BOUND
    # leading batch dimensions pass through
    both = plan.tangent_cotangent(torch.as_tensor(np.stack([q, q])), torch.as_tensor(np.stack([g, g]))).numpy()
    assert both.shape == (2, len(q), plan.nv) and np.array_equal(both[1], got)


def test_tangent_cotangent_refuses_implicit_clusters():
    import torch

    plan = G.Plan(R.blob_of("urdf_four_bar"))
    with pytest.raises(ValueError):
        plan.tangent_cotangent(torch.zeros((1, plan.nq), dtype=torch.float64), torch.zeros((1, plan.nq), dtype=torch.float64))
