"""Energy, centre of mass, centroidal momentum and the momentum matrix of the device against the numpy sums of centroidal_ref.py (which
test_centroidal_ref_cpu.py pins to the oracle), every state on its own scale.

fp64: plan.energy and plan.centroidal on the whole zoo and the two spanning-tree models, B = 1, 65 and 130 (one state; one tile and one
state; two tiles and a ragged third), every output per state at entry_points.TOL64; plan.centroidal_matrix at B = 1 and 65 on an
explicit model, an implicit one and one on the spanning-tree route.

fp32: every output against what single precision itself costs on the same float32-rounded inputs -- the float32 run of the reference --
times term_states.MARGIN (term_states.within_float: worst and median).  MARGINS holds the cases the kernel misses at that margin, as
test_kinematics_gpu.MARGINS does: measured on the MI355X, the allowance twice the measured worst ratio.

Momentum balance on the device (fp64, B = 65, the floating-base models): with ydd = plan.forward_dynamics(q, qd, tau[, f_ext]),
hdot - [0; M g] - (the wrenches about the centre of mass) relative to 1 + max_j |A[:, j]| |ydd|_inf is bounded by BALANCE_BOUND = ten times
test_centroidal_ref_cpu.BALANCE_WORST = 4.9e-14, BALANCE_WORST being the worst value of the same identity in the numpy reference with the
oracle's forward dynamics on the same states (4.9e-15, the larger of the values two hosts measured: that file's docstring); the factor
covers the device's own forward dynamics, which sit at TOL64 of the oracle's.  Measured on the MI355X: 7.0e-16 at worst
(tree_mixed_float), the other three models under 7e-17.  tau acts on the joints only (a generalized force on the floating base is an
external wrench).  On the same
states kinetic = 1/2 yd^T H yd with the device's mass matrix and A yd = h, each at TOL64.

Behaviour: each output asked for alone gives the bits of the call that asks for all (positions with qd = None); set_gravity between two
calls moves potential and hdot to the new reference; the momentum matrix under a GRBDA_WORK_MAX_MB that cuts B = 65 into a full and a
ragged chunk gives the bits of the single chunk; a captured replay of centroidal with all outputs at B = 130 gives the eager bits."""
import functools

import numpy as np
import pytest

import centroidal_ref as C
import entry_points as EP
import generalized_rbda_amd as G
import kinematics_ref as K
import term_states as TS
from test_centroidal_ref_cpu import BALANCE_WORST, FLOATING, balance_cases, balance_scale
from test_kinematics_gpu import BATCHES, MODELS32, MODELS64

pytestmark = pytest.mark.gpu
B_TOP = BATCHES[-1]
SEED = 67
OUTPUTS = C.OUTPUTS
BALANCE_BOUND = 10 * BALANCE_WORST
B_BALANCE = 65
# explicit, implicit, spanning-tree route
MATRIX_MODELS = ("urdf_mit_humanoid", "tello_with_arms", "parallel_chain_exp_d10_l16")
# (model, output) that is not run in fp32, with the reason (test_centroidal_ref_cpu.py asserts that every other one leaves out at most
# term_states.MAX_LEFT_OUT of its batch)
NOT_RUN = {
    ("urdf_four_bar", "potential"): "gravity along z is perpendicular to the linkage's plane: the potential energy is identically zero",
    ("urdf_four_bar", "kinetic"): "one velocity coordinate: H yd^2 / 2 of a yd in U(-1, 1) is under the floor for 1.5 % of the batch (h and com_vel are run)",
}
# (model, output): (margin = twice the measured worst ratio, measured (worst, median) ratio to the float32 run on the MI355X, cause)
# One case, the cause of test_kinematics_gpu.MARGINS: the float32 run takes G = -K_d^-1 K_i of the implicit clusters rounded from the fp64
# oracle, the device solves K_d in fp32, which costs cond(K_d) eps in the spanning velocities (tello_with_arms v there: worst 10.34), and
# the kinetic energy is quadratic in them.  The median is that of ordinary states; every other case measured at most 2.23 (worst) and 2.25
# (median), and fp64 holds this one at 1e-9.
MARGINS = {
    ("tello_with_arms", "kinetic"): (19.0, (9.50, 1.50), "G of the implicit clusters: solved in fp32 on the device, rounded from fp64 in the yardstick"),
}
CASES32 = [(m, o) for m in MODELS32 for o in OUTPUTS if (m, o) not in NOT_RUN]


@functools.lru_cache(maxsize=None)
def draw(name, rounded):
    """(q, qd, ydd) of B_TOP states of `name`, read-only; rounded: to float32-representable values"""
    q, qd, ydd = EP._states(EP._model(name), B_TOP, SEED)
    return tuple(TS._frozen(TS.fp32_rounded(a) if rounded else a) for a in (q, qd, ydd))


def _reference(name, rounded, dtype=np.float64):
    blob = EP._model(name)
    q, qd, ydd = draw(name, rounded)
    ref = C.centroidal(blob, q, qd, ydd, big=EP._big(blob), dtype=dtype)
    return {k: TS._frozen(np.asarray(ref[k], dtype=np.float64)) for k in OUTPUTS}


@functools.lru_cache(maxsize=None)
def reference64(name):
    return _reference(name, False)


@functools.lru_cache(maxsize=None)
def references32(name):
    """(fp64 reference, float32 run as fp64) of the rounded draw, computed once per process"""
    return _reference(name, True), _reference(name, True, np.float32)


def rows(a):
    return np.asarray(a).reshape(a.shape[0], -1)


def device_outputs(plan, q, qd, ydd):
    """all six outputs of the two calls as numpy arrays"""
    kinetic, potential = plan.energy(q, qd)
    out = {k: v for k, v in plan.centroidal(q, qd, ydd).items()}
    out.update(kinetic=kinetic, potential=potential)
    return {k: out[k].double().cpu().numpy() for k in OUTPUTS}


@pytest.mark.parametrize("name", MODELS64)
def test_energy_and_centroidal_fp64(name, gpu):
    import torch

    plan = EP.plan_for(name, ())
    q, qd, ydd = draw(name, False)
    ref = reference64(name)
    assert plan.total_mass() == pytest.approx(C.total_mass(EP._model(name)), rel=1e-14)
    t = lambda a, B: torch.as_tensor(np.ascontiguousarray(a[:B]), dtype=torch.float64, device=gpu)
    for B in BATCHES:
        got = device_outputs(plan, t(q, B), t(qd, B), t(ydd, B))
        err = {k: C.scale_error(got[k], ref[k][:B]) for k in OUTPUTS}
        print(f"{name} B={B}: " + "  ".join(f"{k} {e.max():.1e}" for k, e in err.items()))
        for k, e in err.items():
            assert e.max() < EP.TOL64, (B, k, int(e.argmax()), e.max())


@pytest.mark.parametrize("name", MATRIX_MODELS)
def test_momentum_matrix_fp64(name, gpu):
    import torch

    blob, plan = EP._model(name), EP.plan_for(name, ())
    q = draw(name, False)[0][:65]
    A_ref = C.momentum_matrix(blob, q, big=EP._big(blob))
    for B in (1, 65):
        A = plan.centroidal_matrix(torch.as_tensor(np.ascontiguousarray(q[:B]), dtype=torch.float64, device=gpu)).cpu().numpy()
        assert A.shape == (B, 6, plan.nv)
        e = C.scale_error(A, A_ref[:B])
        print(f"{name} B={B}: A {e.max():.1e}")
        assert e.max() < EP.TOL64, (B, int(e.argmax()), e.max())


@pytest.mark.parametrize("name,out", CASES32, ids=[f"{m}-{o}" for m, o in CASES32])
def test_fp32_within_the_float_run_of_the_reference(name, out, gpu):
    import torch

    plan = EP.plan_for(name, ())
    q, qd, ydd = draw(name, True)
    ref64, ref32 = references32(name)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)
    if out in ("kinetic", "potential"):
        got = dict(zip(("kinetic", "potential"), plan.energy(t(q), t(qd))))[out]
    else:
        got = plan.centroidal(t(q), t(qd), t(ydd), want=(out,))[out]
    got = rows(got.double().cpu().numpy())
    assert np.isfinite(got).all()
    worst, median = TS.float_ratio(got, rows(ref64[out]), rows(ref32[out]))
    print(f"{name} {out}: kernel error / float32 reference error: worst {worst:.2f}, median {median:.2f}")
    margin = MARGINS.get((name, out), (TS.MARGIN,))[0]
    TS.within_float(got, rows(ref64[out]), rows(ref32[out]), margin, what=f"{name} {out}")


@pytest.mark.parametrize("name", FLOATING)
def test_momentum_balance_and_identities_on_the_device(name, gpu):
    import torch

    blob, plan = EP._model(name), EP.plan_for(name, ())
    q, qd, tau = (a[:B_BALANCE] for a in draw(name, False))
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gpu)
    fd = lambda q, qd, tau, fe: plan.forward_dynamics(t(q), t(qd), t(tau), f_ext=t(fe)).cpu().numpy()
    A = plan.centroidal_matrix(t(q)).cpu().numpy()
    for case, want, ydd, _ in balance_cases(blob, q, qd, tau, fd):
        hdot = plan.centroidal(t(q), t(qd), t(ydd), want=("hdot",))["hdot"].cpu().numpy()
        rel = np.abs(hdot - want).max(axis=1) / balance_scale(A, ydd)
        print(f"{name} {case}: hdot - gravity - wrenches {rel.max():.1e} of 1 + max_j |A_j| |ydd| (bound {BALANCE_BOUND:.0e})")
        assert rel.max() < BALANCE_BOUND, (case, int(rel.argmax()), rel.max())
    kinetic = plan.energy(t(q), t(qd))[0].cpu().numpy()
    H = plan.mass_matrix(t(q)).cpu().numpy()
    assert C.scale_error(kinetic, 0.5 * np.einsum("bi,bij,bj->b", qd, H, qd)).max() < EP.TOL64
    h = plan.centroidal(t(q), t(qd), want=("h",))["h"].cpu().numpy()
    assert C.scale_error(np.einsum("bij,bj->bi", A, qd), h).max() < EP.TOL64


@pytest.mark.parametrize("name", ["urdf_mit_humanoid", "tello_with_arms"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_each_output_alone_gives_the_bits_of_all_together(name, dt, gpu):
    import torch

    plan = EP.plan_for(name, ())
    dtype = torch.float64 if dt == "f64" else torch.float32
    q, qd, ydd = (torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu) for a in draw(name, dt == "f32"))
    both = plan.energy(q, qd)
    all_ = plan.centroidal(q, qd, ydd)
    assert sorted(all_) == ["com", "com_vel", "h", "hdot"]
    kinetic_none, potential = plan.energy(q)  # positions only: qd = None
    assert kinetic_none is None and torch.equal(potential, both[1])
    L = G.lib()
    k_alone = torch.empty_like(both[0])
    fn = getattr(L, "grbda_energy_" + dt)
    G._check(fn(plan._h, q.data_ptr(), qd.data_ptr(), k_alone.data_ptr(), None, q.shape[0], 0, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(k_alone, both[0])
    assert torch.equal(plan.centroidal(q, want=("com",))["com"], all_["com"])  # positions only: qd = None
    for out in ("com_vel", "h"):
        assert torch.equal(plan.centroidal(q, qd, want=(out,))[out], all_[out]), out
    assert torch.equal(plan.centroidal(q, qd, ydd, want=("hdot",))["hdot"], all_["hdot"])
    assert sorted(plan.centroidal(q, qd)) == ["com", "com_vel", "h"] and sorted(plan.centroidal(q)) == ["com"]


def test_gravity_is_read_at_launch(gpu):
    import torch

    name = "urdf_mit_humanoid"
    blob = EP._model(name)
    plan = G.Plan(blob)  # (a plan of its own: set_gravity)
    q, qd, ydd = draw(name, False)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gpu)
    before = device_outputs(plan, t(q), t(qd), t(ydd))
    plan.set_gravity(TS.OBLIQUE)
    after = device_outputs(plan, t(q), t(qd), t(ydd))
    ref = C.centroidal(TS.with_gravity(blob, TS.OBLIQUE), q, qd, ydd)
    for k in OUTPUTS:
        assert C.scale_error(after[k], ref[k]).max() < EP.TOL64, k
        assert C.scale_error(before[k], reference64(name)[k]).max() < EP.TOL64, k
        changed = not np.array_equal(before[k], after[k])
        assert changed == (k in ("potential", "hdot")), k


def test_momentum_matrix_chunk_seam(gpu, monkeypatch):
    import torch

    name, B, cap_mb = "urdf_jvrc1_humanoid", 65, 1
    plan = G.Plan(EP._model(name))
    q = torch.as_tensor(np.ascontiguousarray(draw(name, False)[0][:B]), dtype=torch.float64, device=gpu)
    # the work slab of a state (include/grbda_hip.h): nv (nq + nv + 2 span_vel) scalars
    per_state = plan.nv * (plan.nq + plan.nv + 2 * plan.n_span_vel) * 8
    chunk = (cap_mb << 20) // per_state
    assert 1 <= chunk < B and B % chunk != 0 and B > chunk, "no ragged second chunk: nothing is tested"
    plan.release_work()
    whole = plan.centroidal_matrix(q).cpu().numpy()
    assert plan.release_work() >= B * per_state
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", str(cap_mb))
    chunked = plan.centroidal_matrix(q).cpu().numpy()
    assert 0 < plan.release_work() <= (cap_mb << 20) + 256
    assert np.array_equal(whole, chunked)


def test_graph_capture_replays_the_eager_bits(gpu):
    import torch

    import graph_capture

    name = "urdf_mit_humanoid"
    plan = G.Plan(EP._model(name))
    src = [torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gpu) for a in draw(name, False)]
    eager = {k: v.clone() for k, v in plan.centroidal(*src).items()}
    x = [torch.zeros_like(a) for a in src]
    x[0].copy_(src[0])  # (valid positions for the eager call inside capture())
    cap = graph_capture.capture(lambda: plan.centroidal(*x))
    try:
        assert cap.nodes["kernel"] == 2 and cap.nodes["total"] == 2, cap.nodes  # spanning rates, centroidal_kernel
        for a, b in zip(x, src):
            a.copy_(b)
        out = cap.replay()
        for k in eager:
            assert torch.equal(out[k], eager[k]), k
    finally:
        cap.drop()
