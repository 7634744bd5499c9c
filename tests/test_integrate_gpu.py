"""grbda_integrate_* on the GPU (run with -m gpu on an MI355X): one semi-implicit Euler step against the float64 CPU reference of
integrate_ref.py, at the batch sizes where a tile loop goes wrong (1, 63, 64, 65, 130), in both precisions; in place; buffer edges;
the manifold; the unit quaternion over a long rollout; the refusals.

Time steps (integrate_ref.DT): 0.25 for explicit models; implicit models 0.05, Tello 0.025 -- the largest halving of 0.05 at which the
oracle reference alone accepts >= 95 % of the stepped states (shares in tests/test_integrate_cpu.py, which asserts them on the CPU;
asserted again here on the reference before anything is compared).  Values are compared on the states the reference accepts; `ok` must
equal the reference's flag except where the reference's |phi| after the projection lies within a factor 10 of the tolerance."""
import functools

import numpy as np
import pytest

import generalized_rbda_amd as G
import guarded
import integrate_ref as R

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
MODELS = R.EXPLICIT_MODELS + R.IMPLICIT_MODELS
TOL32 = 1e-3  # the project's fp32 bound; also the projection tolerance an fp32 caller can reach
EINVAL, EUNSUPPORTED, OK = -1, -2, 0


@functools.lru_cache(maxsize=None)
def plan_of(model):
    return G.Plan(R.blob_of(model))


@functools.lru_cache(maxsize=None)
def reference(model, B, rounded):
    """(inputs, (q', qd', ok, phi)) in float64; rounded: the inputs rounded to float32 first (the fp32 comparison)"""
    s = R.states_of(model, B)
    if rounded:
        s = tuple(a.astype(np.float32).astype(np.float64) for a in s)
    ref = R.reference_step(R.blob_of(model), *s, R.dt_of(model))
    for a in s + ref:
        a.setflags(write=False)
    return s, ref


def dev(a, dtype, gpu):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64) if t.dtype.is_floating_point else t.detach().cpu().numpy()


def run(model, B, dtype, gpu, tol, rounded):
    import torch

    (q, qd, ydd), ref = reference(model, B, rounded)
    qn, vn, ok = plan_of(model).integrate(dev(q, dtype, gpu), dev(qd, dtype, gpu), dev(ydd, dtype, gpu), R.dt_of(model), tol=tol)
    torch.cuda.synchronize()
    return (q, qd, ydd), ref, host(qn), host(vn), host(ok)


def quat_sign_aligned(got, ref, kinds):
    """the quaternion is compared up to sign: flip the rows of `got` whose quaternion points the other way"""
    cols = np.nonzero(kinds == "quat")[0]
    if cols.size:
        flip = np.einsum("bi,bi->b", got[:, cols], ref[:, cols]) < 0
        got = got.copy()
        got[np.ix_(flip, cols)] *= -1
    return got


def check_flags(ok, ref_ok, phi, tol, what):
    """ok == the reference's flag, except where the reference's |phi| lies within a factor 10 of the tolerance"""
    unsure = (phi > tol / 10) & (phi < tol * 10)
    bad = (ok.astype(bool) != ref_ok) & ~unsure
    assert not bad.any(), f"{what}: ok differs from the reference on states {np.nonzero(bad)[0][:8]} (phi {phi[bad][:8]})"


@pytest.mark.parametrize("B", R.BATCHES)
@pytest.mark.parametrize("model", MODELS)
def test_fp64_matches_the_cpu_reference(model, B, gpu):
    """max over all entries of q' and qd' <= 1e-9 (the project's fp64 parity bound), quaternion up to sign"""
    import torch

    _, (rq, rv, rok, phi), qn, vn, ok = run(model, B, torch.float64, gpu, R.TOL, False)
    assert rok.mean() >= 0.95, f"the reference accepts only {rok.mean():.3f} of the states"
    kinds = R.column_kinds(R.blob_of(model))
    qn = quat_sign_aligned(qn, rq, kinds)
    eq, ev = np.abs(qn - rq)[rok].max(), np.abs(vn - rv)[rok].max()
    print(f"INTEGRATE f64 {model} B={B}: q' {eq:.2e} qd' {ev:.2e} ok {ok.mean():.3f} ref ok {rok.mean():.3f}")
    assert np.isfinite(qn[rok]).all() and max(eq, ev) <= 1e-9
    check_flags(ok, rok, phi, R.TOL, f"{model} B={B}")


@pytest.mark.parametrize("B", R.BATCHES)
@pytest.mark.parametrize("model", MODELS)
def test_fp32_matches_the_cpu_reference(model, B, gpu):
    """Against the float64 reference on the float32-rounded inputs.  qd', explicit coordinates (the independent ones of implicit
    clusters move the same way: unit rows of G) and the base position: 16 eps32 max(1, |ref|) -- a few roundings of a + dt b with entries of
    order pi; quaternion: 32 eps32; dependent coordinates of implicit clusters: 1e-3 on the states that pass the conditioning gate of
    states.accept before and after the step.  The projection runs with tol = 1e-3 -- |phi| < 1e-8 is out of fp32's reach -- and its flag
    is held against the reference's with the factor-10 band around either tolerance."""
    import torch

    blob = R.blob_of(model)
    (q, qd, _), (rq, rv, rok, phi), qn, vn, ok = run(model, B, torch.float32, gpu, TOL32, True)
    assert rok.mean() >= 0.95
    kinds = R.column_kinds(blob)
    qn = quat_sign_aligned(qn, rq, kinds)
    lin = 16 * EPS32 * np.maximum(1.0, np.abs(rv))
    ev = (np.abs(vn - rv) / lin)[rok].max()
    assert ev <= 1.0, f"qd': {ev:.2f} x the bound"
    plain = (kinds == "pos") | (kinds == "ind")
    ep = (np.abs(qn - rq) / (16 * EPS32 * np.maximum(1.0, np.abs(rq))))[np.ix_(rok, plain)]
    eqt = np.abs(qn - rq)[np.ix_(rok, kinds == "quat")]
    dep = kinds == "dep"
    msg = f"INTEGRATE f32 {model} B={B}: qd' {ev:.2f} x bound, plain q' {ep.max() if ep.size else 0:.2f} x bound"
    if eqt.size:
        msg += f", quat {eqt.max() / EPS32:.1f} eps"
        assert eqt.max() <= 32 * EPS32
    if ep.size:
        assert ep.max() <= 1.0, f"explicit q': {ep.max():.2f} x the bound"
    if dep.any():
        gated = rok & R.gate(blob, q, qd) & R.gate(blob, rq, rv)
        assert gated.any()
        ed = np.abs(qn - rq)[np.ix_(gated, dep)]
        msg += f", dependent {ed.max():.2e} on {gated.sum()} gated states"
        assert ed.max() <= TOL32
        unsure = ((phi > R.TOL / 10) & (phi < R.TOL * 10)) | ((phi > TOL32 / 10) & (phi < TOL32 * 10))
        bad = (ok.astype(bool) != rok) & ~unsure & gated
        assert not bad.any(), f"ok differs from the reference on gated states {np.nonzero(bad)[0][:8]}"
    else:
        assert ok.all()
    print(msg)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("model", ["urdf_mini_cheetah", "urdf_four_bar", "tello_with_arms"])
def test_in_place_gives_the_same_bits(model, dtype_name, gpu):
    import torch

    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    plan = plan_of(model)
    for B in (65, 130):
        q, qd, ydd = (dev(a, dtype, gpu) for a in R.states_of(model, B))
        qn, vn, ok = plan.integrate(q, qd, ydd, R.dt_of(model))
        q2, qd2 = q.clone(), qd.clone()
        a, b, ok2 = plan.integrate(q2, qd2, ydd, R.dt_of(model), out=(q2, qd2))
        torch.cuda.synchronize()
        assert a is q2 and b is qd2
        assert torch.equal(qn.view(torch.uint8), q2.view(torch.uint8)) and torch.equal(vn.view(torch.uint8), qd2.view(torch.uint8))
        assert torch.equal(ok, ok2)
        assert not torch.equal(qn, q)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("model", ["urdf_mini_cheetah", "urdf_four_bar"])
def test_outputs_keep_to_their_buffers(model, B, dtype_name, lead, gpu):
    """every input and output between two bands of a canary pattern (guarded.py): the bands of q', qd' and ok intact, every element of
    them written, the inputs (bands included) bit-identical afterwards"""
    import torch

    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    plan = plan_of(model)
    ins = [guarded.place(a, dtype, gpu, lead) for a in R.states_of(model, B)]
    before = [guarded.snapshot(t) for t in ins]
    with guarded.guarded_outputs(lead) as made:
        qn, vn, ok = plan.integrate(*ins, R.dt_of(model))
    torch.cuda.synchronize()
    assert len(made) == 3
    for t in made:
        assert guarded.check(t) == 0, "an output element was never written"
    for t, snap in zip(ins, before):
        assert guarded.same_bits(t, snap), "an input was written to"
    assert torch.isfinite(qn).all() and torch.isfinite(vn).all()
    # in place: the bands around q and qd stay as they are
    with guarded.guarded_outputs(lead) as made:
        plan.integrate(*ins, R.dt_of(model), out=(ins[0], ins[1]))
    torch.cuda.synchronize()
    for t in (ins[0], ins[1], made[0]):
        assert guarded.check(t) == 0
    assert torch.equal(ins[0], qn) and torch.equal(ins[1], vn)


@pytest.mark.parametrize("model", R.IMPLICIT_MODELS)
def test_stepped_states_are_on_the_manifold_where_ok(model, gpu):
    """state_to_independent(q') reports status 0 exactly where integrate reported ok"""
    import torch

    plan = plan_of(model)
    for B in (65, 130):
        q, qd, ydd = (dev(a, torch.float64, gpu) for a in R.states_of(model, B))
        qn, vn, ok = plan.integrate(q, qd, ydd, R.dt_of(model))
        status = plan.state_to_independent(qn, tol=R.TOL)[2]
        torch.cuda.synchronize()
        assert torch.equal(status == 0, ok), f"{model} B={B}: {int((status == 0).sum())} valid, {int(ok.sum())} ok"
        assert ok.float().mean() >= 0.9


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_quaternion_stays_unit_over_a_long_rollout(dtype_name, gpu):
    """1 000 steps of the mini cheetah in free fall (zero torque, dt = 1e-3): every step normalises, so | |quat| - 1 | carries a few
    roundings and no drift: <= 8 eps of the type (the norm is evaluated in float64 from the stored components)"""
    import torch

    dtype, eps = (torch.float64, EPS64) if dtype_name == "f64" else (torch.float32, EPS32)
    model, B = "urdf_mini_cheetah", 65
    plan = plan_of(model)
    q, qd, _ = (dev(a, dtype, gpu) for a in R.states_of(model, B))
    qT, vT, ok = plan.rollout(q, qd, torch.zeros_like(qd), 1e-3, 1000)
    torch.cuda.synchronize()
    cols = np.nonzero(R.column_kinds(R.blob_of(model)) == "quat")[0]
    norm = np.linalg.norm(host(qT)[:, cols], axis=1)
    print(f"QUAT NORM {dtype_name}: max | |quat| - 1 | = {np.abs(norm - 1).max() / eps:.2f} eps")
    assert np.isfinite(host(qT)).all() and ok.all()
    assert np.abs(norm - 1).max() <= 8 * eps
    assert np.abs(host(qT) - host(q)).max() > 1e-2  # it fell


def _raw_integrate(plan, q, qd, ydd, dt, qn, vn, B, stream=None, fn="grbda_integrate_f64"):
    return getattr(G.lib(), fn)(plan._h, q, qd, ydd, dt, qn, vn, None, 50, 1e-8, B, 0, stream)


@pytest.mark.parametrize("model", ["urdf_mini_cheetah_rpy", "parallel_chain_imp_d10_l17"])
def test_uncovered_plans_are_refused_and_enqueue_nothing(model, gpu):
    import torch

    plan = plan_of(model)
    B = 4
    q = torch.zeros((B, plan.nq), dtype=torch.float64, device=gpu)
    qd, ydd = torch.zeros((B, plan.nv), dtype=torch.float64, device=gpu), torch.zeros((B, plan.nv), dtype=torch.float64, device=gpu)
    qn, vn = torch.full_like(q, 7.0), torch.full_like(qd, 7.0)
    torch.cuda.synchronize()
    assert _raw_integrate(plan, q.data_ptr(), qd.data_ptr(), ydd.data_ptr(), 0.1, qn.data_ptr(), vn.data_ptr(), B) == EUNSUPPORTED
    assert (G.lib().grbda_last_error() or b"").decode()
    for call in (lambda: plan.integrate(q, qd, ydd, 0.1), lambda: plan.step(q, qd, ydd, 0.1), lambda: plan.rollout(q, qd, ydd, 0.1, 2)):
        with pytest.raises(G.GrbdaError) as e:
            call()
        assert e.value.code == EUNSUPPORTED and str(e.value)
    torch.cuda.synchronize()
    assert (qn == 7.0).all() and (vn == 7.0).all()  # nothing ran


@pytest.mark.parametrize("B", [65, 130])
def test_explicit_plan_on_the_spanning_tree_route_integrates(B, gpu):
    import torch

    model = "parallel_chain_exp_d10_l16"
    plan = plan_of(model)
    assert plan.info().spanning_tree_route == 1
    rng = np.random.default_rng(B)
    q, qd, ydd = rng.uniform(-1, 1, (B, plan.nq)), rng.uniform(-1, 1, (B, plan.nv)), rng.uniform(-1, 1, (B, plan.nv))
    rq, rv, rok, _ = R.reference_step(R.blob_of(model), q, qd, ydd, R.DT_EXPLICIT, big=True)
    qn, vn, ok = plan.integrate(dev(q, torch.float64, gpu), dev(qd, torch.float64, gpu), dev(ydd, torch.float64, gpu), R.DT_EXPLICIT)
    torch.cuda.synchronize()
    assert np.abs(host(qn) - rq).max() <= 1e-9 and np.abs(host(vn) - rv).max() <= 1e-9 and ok.all()
    assert np.abs(rq - q).max() > 0.1


def test_bad_arguments_are_refused(gpu):
    import torch

    plan = plan_of("urdf_mini_cheetah")
    B, T = 65, 3
    q = torch.zeros((B, plan.nq), dtype=torch.float64, device=gpu)
    q[:, 3] = 1.0
    qd, ydd, work = (torch.zeros((B, plan.nv), dtype=torch.float64, device=gpu) for _ in range(3))
    qn, vn = torch.empty_like(q), torch.empty_like(qd)
    p = lambda t: t.data_ptr()
    for dt in (float("nan"), float("inf")):
        assert _raw_integrate(plan, p(q), p(qd), p(ydd), dt, p(qn), p(vn), B) == EINVAL
    assert _raw_integrate(plan, p(q), p(qd), p(ydd), 0.1, p(q) + 8, p(vn), B) == EINVAL       # partially overlapping
    assert _raw_integrate(plan, p(q), p(qd), p(ydd), 0.1, p(qn), p(qd) + 8 * (B * plan.nv - 1), B) == EINVAL
    assert _raw_integrate(plan, p(q), p(qd), p(ydd), 0.1, p(qn), p(ydd), B) == EINVAL
    roll = G.lib().grbda_rollout_f64
    for bad in (0, 2, T + 1):
        assert roll(plan._h, p(q), p(qd), p(ydd), bad, 0.1, T, p(work), None, None, None, B, 0, None) == EINVAL
    assert roll(plan._h, p(q), p(qd), p(ydd), 1, 0.1, -1, p(work), None, None, None, B, 0, None) == EINVAL
    assert _raw_integrate(plan, p(q), p(qd), p(ydd), 0.1, p(qn), p(vn), 0) == OK
    assert roll(plan._h, p(q), p(qd), p(ydd), 1, 0.1, T, p(work), None, None, None, 0, 0, None) == OK
    torch.cuda.synchronize()
