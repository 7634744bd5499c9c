"""grbda_step_* and grbda_rollout_* on the GPU (run with -m gpu on an MI355X): a step is forward dynamics followed by integrate, a
rollout is T steps in place -- bit for bit --, a rollout can be captured into a graph after one eager call, and the scheme is first
order in dt."""
import numpy as np
import pytest

import generalized_rbda_amd as G
import graph_capture as GC
import integrate_ref as R
from test_integrate_gpu import dev, host, plan_of

pytestmark = pytest.mark.gpu
EINVAL = -1


def same_bits(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def _dtype(name):
    import torch

    return torch.float64 if name == "f64" else torch.float32


def _f_ext(plan, B, dtype, gpu):
    rng = np.random.default_rng(17)
    return dev(rng.uniform(-1, 1, (B, plan.n_bodies, 6)), dtype, gpu)


@pytest.mark.parametrize("with_f_ext", [False, True])
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("B", [65, 130])
@pytest.mark.parametrize("model", ["urdf_mini_cheetah", "tello_with_arms", "urdf_four_bar"])
def test_step_is_forward_dynamics_then_integrate(model, B, dtype_name, with_f_ext, gpu):
    import torch

    dtype, plan, dt = _dtype(dtype_name), plan_of(model), R.dt_of(model)
    q, qd, tau = (dev(a, dtype, gpu) for a in R.states_of(model, B))
    fe = _f_ext(plan, B, dtype, gpu) if with_f_ext else None
    qn, vn, ydd, ok = plan.step(q, qd, tau, dt, f_ext=fe)
    ydd2 = plan.forward_dynamics(q, qd, tau, f_ext=fe)
    qn2, vn2, ok2 = plan.integrate(q, qd, ydd2, dt)
    torch.cuda.synchronize()
    assert same_bits(ydd, ydd2) and same_bits(qn, qn2) and same_bits(vn, vn2) and torch.equal(ok, ok2)
    assert torch.isfinite(ydd).all() and not torch.equal(qn, q)
    if with_f_ext:
        assert not same_bits(ydd, plan.forward_dynamics(q, qd, tau))


@pytest.mark.parametrize("per_step_tau", [False, True])
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("model", ["urdf_mini_cheetah", "urdf_four_bar"])
def test_rollout_is_five_steps(model, dtype_name, per_step_tau, gpu):
    import torch

    T, B = 5, 65
    dtype, plan = _dtype(dtype_name), plan_of(model)
    dt = R.dt_of(model) / 5
    q, qd, tau = (dev(a, dtype, gpu) for a in R.states_of(model, B))
    taus = torch.stack([tau * (1.0 - 0.3 * k) for k in range(T)]) if per_step_tau else tau
    q0, qd0 = q.clone(), qd.clone()
    qT, vT, ok, qt, vt = plan.rollout(q, qd, taus, dt, T, record=True)
    cq, cv, all_ok = q, qd, torch.ones(B, dtype=torch.bool, device=gpu)
    for k in range(T):
        cq, cv, _, ok_k = plan.step(cq, cv, taus[k] if per_step_tau else tau, dt)
        all_ok &= ok_k
        assert same_bits(qt[k], cq) and same_bits(vt[k], cv), f"recorded state {k + 1}"
    torch.cuda.synchronize()
    assert same_bits(qT, cq) and same_bits(vT, cv) and torch.equal(ok, all_ok)
    assert same_bits(q, q0) and same_bits(qd, qd0)  # the Python layer rolls copies out
    # without the record the same end state; T = 0 leaves the state untouched
    qT2, vT2, ok2 = plan.rollout(q, qd, taus, dt, T)
    z = plan.rollout(q, qd, tau, dt, 0)
    torch.cuda.synchronize()
    assert same_bits(qT2, qT) and same_bits(vT2, vT) and torch.equal(ok2, ok)
    assert same_bits(z[0], q) and same_bits(z[1], qd) and z[2].all()


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("model", ["urdf_mini_cheetah", "urdf_four_bar"])
def test_rollout_captured_into_a_graph(model, dtype_name, gpu):
    """One eager rollout(T = 4) on a side stream, then the same call captured: two replays from the same initial state equal the eager
    result bit for bit; the graph is linear -- kernels and device-to-device copies only; gravity set after the capture does not change
    the replay (it is read at launch, i.e. at capture)."""
    import torch

    T, B = 4, 130
    dtype = _dtype(dtype_name)
    plan = G.Plan(R.blob_of(model))  # (its own plan: the gravity is changed below)
    dt = R.dt_of(model) / 5
    q, qd, tau = (dev(a, dtype, gpu) for a in R.states_of(model, B))
    fn = lambda: plan.rollout(q, qd, tau, dt, T, record=True)
    cap = GC.capture(fn)
    try:
        with torch.cuda.stream(cap.stream):
            want = fn()
        cap.stream.synchronize()
        assert cap.nodes["other"] == 0 and cap.nodes["kernel"] >= 2 * T and cap.nodes["memcpy"] >= 2 * T, cap.nodes
        for _ in range(2):
            got = cap.replay()
            assert all(same_bits(a, b) for a, b in zip(got, want))
        g = plan.get_gravity()
        plan.set_gravity((0.3, -0.2, 4.0))
        got = cap.replay()
        assert all(same_bits(a, b) for a, b in zip(got, want)), "gravity set after the capture changed the replay"
        with torch.cuda.stream(cap.stream):
            other = fn()
        cap.stream.synchronize()
        assert not same_bits(other[0], want[0]), "an eager call does follow the new gravity"
        plan.set_gravity(g)
    finally:
        cap.drop()


def test_a_capture_that_would_grow_the_scratch_slab_is_refused(gpu):
    import torch

    model = "urdf_mini_cheetah"
    plan = G.Plan(R.blob_of(model))
    small = tuple(dev(a, torch.float64, gpu) for a in R.states_of(model, 65))
    nq, nv, B = plan.nq, plan.nv, 64 * 4096
    big = (small[0][:1].repeat(B, 1).contiguous(), torch.zeros((B, nv), dtype=torch.float64, device=gpu), torch.zeros((B, nv), dtype=torch.float64, device=gpu))
    with pytest.raises(G.GrbdaError) as e:
        GC.capture(lambda: plan.rollout(*big, 1e-3, 2), warm=lambda: plan.rollout(*small, 1e-3, 2))
    assert e.value.code == EINVAL and "capture" in str(e.value)
    torch.cuda.synchronize()


def test_the_scheme_is_first_order(gpu):
    """rev_rotor_chain_3, fp64, B = 64, zero torque, T_end = 0.1 with dt = 1e-2, dt / 2 and dt / 4: |x(dt) - x(dt/2)| / |x(dt/2) - x(dt/4)|
    lies in [1.6, 2.4] (2 for a first-order scheme; the band covers the second-order remainder at these steps)."""
    import torch

    model, B = "rev_rotor_chain_3", 64
    plan = plan_of(model)
    q, qd, _ = (dev(a, torch.float64, gpu) for a in R.states_of(model, B))
    zero = torch.zeros_like(qd)
    ends = []
    for n in (10, 20, 40):
        qT, vT, ok = plan.rollout(q, qd, zero, 0.1 / n, n)
        ends.append(np.concatenate([host(qT), host(vT)], axis=1))
    torch.cuda.synchronize()
    d1, d2 = np.abs(ends[0] - ends[1]).max(), np.abs(ends[1] - ends[2]).max()
    r_norm = np.linalg.norm(ends[0] - ends[1]) / np.linalg.norm(ends[1] - ends[2])
    print(f"FIRST ORDER: max-norm ratio {d1 / d2:.4f}, 2-norm ratio {r_norm:.4f} (differences {d1:.3e}, {d2:.3e})")
    assert d2 > 1e-6
    assert 1.6 <= d1 / d2 <= 2.4 and 1.6 <= r_norm <= 2.4
