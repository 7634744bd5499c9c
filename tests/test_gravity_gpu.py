"""Gravity on the GPU (run with -m gpu on an MI355X).  grbda_plan_set_gravity changes a kernel argument (a_root = -gravity) that some
twenty kernel sites read, and the spanning-tree plan gets it by copy; the other GPU tests run at the gravity their model was built with.
Here every entry point that reads gravity is held against the oracle at four gravities -- the oracle is fed plan.blob after set_gravity --,
every entry point that must not read it gives the same bits at two, and a plan that has launched before (device tables cached) follows
set_gravity on its next call.  The later entry points -- contact dynamics, step / rollout, the inverse-dynamics derivatives, energy and the
centroidal quantities -- are held the same way with the checkers and bounds of entry_points.py; three of their kernels get the gravity as
a host-side triple of its own, added back in world axes to what the twists carry as -g in body axes.  contact_points and contact_impulse,
where gravity cancels, are held to their references at every gravity all the same: an error in the added g shows there at full size.
Each test builds its own plans: the plans of entry_points.plan_for are shared and keep their gravity."""
import functools

import numpy as np
import pytest

import entry_points as EP
import oracle_py as O
import term_states as TS
from entry_points import ENTRY, TOL32, TOL64

pytestmark = pytest.mark.gpu
B = 300
SEED = 41
GRAVITIES = {"native": None, "zero": (0.0, 0.0, 0.0), "oblique": TS.OBLIQUE, "up": (0.0, 0.0, 9.81)}

# (id, model, plan-time switches, entry point, what the fp32 kernel name holds or None)
READERS = [
    ("chain", "urdf_mini_cheetah", {"GRBDA_NO_LATENCY_MODE": "1"}, "aba", "aba_chain_kernel<float"),
    ("chain", "urdf_mini_cheetah", {"GRBDA_NO_LATENCY_MODE": "1"}, "rnea", "rnea_chain_kernel<float"),
    ("lm4", "urdf_mit_humanoid", {}, "aba", "aba_chain_lm_kernel<float, 4"),
    ("lm4", "urdf_mit_humanoid", {}, "rnea", "rnea_chain_lm_kernel<float, 4"),
    ("lm2", "tello_with_arms", {"GRBDA_LM_WAVES": "2"}, "aba", "aba_chain_lm_kernel<float, 2, true"),
    ("lm2", "tello_with_arms", {"GRBDA_LM_WAVES": "2"}, "rnea", "rnea_chain_lm_kernel<float, 2, true"),
    ("interpreter", "tree_mixed_float", {"GRBDA_NO_CHAIN": "1"}, "aba", "grbda_hip::aba_kernel<float"),
    ("interpreter", "tree_mixed_float", {"GRBDA_NO_CHAIN": "1"}, "rnea", "grbda_hip::rnea_kernel<float"),
    ("gen1", "urdf_six_bar", {}, "aba", "aba_gen1_kernel<float"),
    ("gen1", "urdf_six_bar", {}, "rnea", "rnea_gen1_kernel<float"),
    ("latency", "urdf_mini_cheetah", {}, "aba_fext", None),
    ("latency", "urdf_mini_cheetah", {}, "rnea_fext", None),
    ("interpreter", "tree_mixed_float", {"GRBDA_NO_CHAIN": "1"}, "aba_fext", None),
    ("chain", "urdf_mini_cheetah", {}, "bias", None),
    ("gen1", "urdf_six_bar", {}, "bias", None),
    ("two_parent", "two_parent", {}, "aba", None),
    ("two_parent", "two_parent", {}, "rnea", None),
    ("spanning_tree", "parallel_chain_exp_d10_l16", {}, "aba", None),
    ("spanning_tree", "parallel_chain_exp_d10_l16", {}, "rnea", None),
]
DERIVATIVE_ROUTES = [
    ("analytic", "urdf_mini_cheetah", {}),
    ("dense", "urdf_mini_cheetah", {"GRBDA_NO_MINV": "1"}),
    ("differences", "urdf_mini_cheetah", {"GRBDA_NO_ANALYTIC": "1"}),
    ("manifold", "tello", {}),
    ("manifold", "urdf_four_bar", {}),
]
SPANNING_TREE = ("two_parent", "parallel_chain_exp_d10_l16")
N_CONTACTS = {"urdf_mini_cheetah": 4, "tello_with_arms": 2, "urdf_mit_humanoid": 8}  # of entry_points.CONTACT_SETS; every other model: 1
# fp32 forward dynamics on the spanning-tree route against the float oracle, by gravity: (margin = 2 x the measured ratio, the measured
# ratio: the larger of worst state and median).  Cause: the route factorises the dense mass matrix of the spanning tree and projects onto
# the constraint; the float oracle runs the cluster recursion on fewer coordinates.  test_term_checker_cpu.py: a term wrong by 1 % still
# fails.
SPANNING_TREE_MARGINS = {("two_parent", "aba", "native"): (37.6, 18.8), ("two_parent", "aba", "zero"): (31.0, 15.5),
                         ("two_parent", "aba", "oblique"): (13.8, 6.9), ("two_parent", "aba", "up"): (14.2, 7.1)}


def own_plan(model, env, gravity=None):
    plan = TS.compile_under(EP._model(model), env)
    if model in SPANNING_TREE:
        assert plan.info().spanning_tree_route == 1
    if gravity is not None:
        plan.set_gravity(gravity)
    blob = plan.blob
    assert plan.get_gravity() == list(TS.native_gravity(EP._model(model)) if gravity is None else gravity)
    if EP._big(EP._model(model)):
        EP._BIG.add(blob)  # (the oracle with room for the big clusters)
    register(model, blob)
    return plan, blob


def register(model, blob):
    """entry_points._contacts and _dt go by the name a blob was made under, and a blob after set_gravity is another blob: without its
    name a contact row falls back to one point on the last link, and a stepping row to the default time step"""
    EP._NAMES.setdefault(bytes(blob), model)
    assert EP._name(blob) == model
    assert EP._dt(blob) == EP._dt(EP._model(model))
    bodies, offsets = EP._contacts(blob)
    assert (list(bodies), [tuple(o) for o in offsets]) == (list(EP._contacts(EP._model(model))[0]), [tuple(o) for o in EP._contacts(EP._model(model))[1]])
    if model in N_CONTACTS:
        assert len(bodies) == N_CONTACTS[model], f"{model}: {len(bodies)} contacts"


def inputs(model, plan, dtype, gpu, max_cond=None):
    """the states are drawn once, from the model as it was built: the same at every gravity"""
    return EP._inputs(EP._model(model), plan, B, SEED, dtype, gpu, max_cond)


def outputs(plan, entry, x):
    import torch

    outs = ENTRY[entry][0](plan, x)
    torch.cuda.synchronize()
    return EP._host(outs)


def dtypes():
    import torch

    return ((torch.float64, TOL64), (torch.float32, TOL32))


@pytest.mark.parametrize("gname", list(GRAVITIES))
@pytest.mark.parametrize("route,model,env,entry,kernel", READERS, ids=[f"{e}-{r}-{m}" for r, m, _, e, _ in READERS])
def test_dynamics_follow_gravity(route, model, env, entry, kernel, gname, gpu):
    """forward / inverse dynamics (with and without external forces) and the bias force against the oracle at plan.blob's gravity: fp64 at
    TOL64, fp32 at TOL32, and fp32 forward / inverse dynamics within 5 x the float oracle on the term's own scale"""
    import torch

    plan, blob = own_plan(model, env, GRAVITIES[gname])
    if kernel is not None:
        assert kernel in plan.kernel_name(entry, "f32", B)
    for dtype, tol in dtypes():
        s, x = inputs(model, plan, dtype, gpu)
        o = outputs(plan, entry, x)
        ENTRY[entry][1](blob, s, o, tol)
        if dtype == torch.float32 and entry in ("aba", "rnea") and not EP._big(blob):  # (the float oracle has no build for the big clusters)
            f64, f32 = (O.forward_dynamics, O.forward_dynamics_f32) if entry == "aba" else (O.inverse_dynamics, O.inverse_dynamics_f32)
            ref, fl = f64(blob, s["q"], s["qd"], s["tau"]), f32(blob, s["q"], s["qd"], s["tau"]).astype(np.float64)
            print(f"GRAVITY {entry} {route} {model} {gname}: {TS.float_ratio(o[0], ref, fl)}")
            TS.within_float(o[0], ref, fl, SPANNING_TREE_MARGINS.get((model, entry, gname), (TS.MARGIN,))[0], what=f"{entry} {route} {model} {gname}")


@functools.lru_cache(maxsize=2)
def derivative_references(blob, model, max_cond):
    """(d ydd / d q, d ydd / d qd, d ydd / d tau) of the oracle at the fp32-rounded states: one evaluation for both precisions and the
    three entry points"""
    import torch

    s = EP._host_inputs(EP._model(model), n_bodies_of(blob), B, SEED, torch.float32, max_cond)
    return (EP._dq_oracle(blob, s["q"], s["qd"], s["tau"]), EP._fd_columns(blob, s["q"], s["qd"], s["tau"], "dqd"),
            EP._fd_columns(blob, s["q"], s["qd"], s["tau"], "dtau"))


def n_bodies_of(blob):
    import struct

    return struct.unpack_from("<ii", blob, 8)[0]


@pytest.mark.parametrize("gname", list(GRAVITIES))
@pytest.mark.parametrize("route,model,env", DERIVATIVE_ROUTES, ids=[f"{r}-{m}" for r, m, _ in DERIVATIVE_ROUTES])
def test_derivatives_follow_gravity(route, model, env, gname, gpu):
    """fd_dq, fd_dqd and fd_derivatives on the analytic, dense, difference-batch and constraint-manifold routes: the bounds of
    entry_points (2e-5 for d / d q, against differences of the oracle; 1e-8 for the exact columns; TOL32 in fp32).  Both precisions get
    the fp32-rounded states, so the oracle differentiates once per gravity."""
    import torch

    bound = EP.draw_bound("fd_dq")
    plan, blob = own_plan(model, env, GRAVITIES[gname])
    dq, dqd, dtau = derivative_references(blob, model, bound)
    for dtype, tol in dtypes():
        s, x = inputs(model, plan, torch.float32, gpu, bound)
        x = {k: v.to(dtype) for k, v in x.items()}
        got_dq, got_dqd = outputs(plan, "fd_dq", x)[0], outputs(plan, "fd_dqd", x)[0]
        all3 = outputs(plan, "fd_derivatives", x)
        for name, got, ref, floor in (("fd_dq", got_dq, dq, 2e-5), ("fd_derivatives dq", all3[0], dq, 2e-5), ("fd_dqd", got_dqd, dqd, 1e-8),
                                      ("fd_derivatives dqd", all3[1], dqd, 1e-8), ("fd_derivatives dtau", all3[2], dtau, 1e-8)):
            err = EP._rel(got, ref)
            assert err < max(tol, floor), f"{name} {dtype}: {err:.2e}"


@pytest.mark.parametrize("gname", list(GRAVITIES))
def test_sharded_host_follows_gravity(gname, gpu):
    model = "urdf_mini_cheetah"
    plan, blob = own_plan(model, {}, GRAVITIES[gname])
    import torch

    s = EP._host_inputs(EP._model(model), plan.n_bodies, B, SEED, torch.float32)
    q, qd, x = s["q"], s["qd"], s["tau"]
    assert EP._rel(plan.sharded_host("aba", q, qd, x, 1), O.forward_dynamics(blob, q, qd, x)) < TOL64
    assert EP._rel(plan.sharded_host("rnea", q, qd, x, 1), O.inverse_dynamics(blob, q, qd, x)) < TOL64
    f32 = lambda a: a.astype(np.float32)
    assert EP._rel(plan.sharded_host("aba", f32(q), f32(qd), f32(x), 1).astype(np.float64), O.forward_dynamics(blob, q, qd, x)) < TOL32
    assert EP._rel(plan.sharded_host("rnea", f32(q), f32(qd), f32(x), 1).astype(np.float64), O.inverse_dynamics(blob, q, qd, x)) < TOL32


@pytest.mark.parametrize("gname", list(GRAVITIES))
@pytest.mark.parametrize("model", ["urdf_mini_cheetah", "tree_mixed_float", "urdf_four_bar"])
def test_bodies_at_rest_accelerate_against_gravity(model, gname, gpu):
    """body_twists at qd = 0, ydd = 0: every body's spatial acceleration is the base's -gravity in its own coordinates -- no angular
    part, the linear part E_i (-g) with E_i the rotation of body_poses (the oracle's)."""
    import torch

    plan, blob = own_plan(model, {}, GRAVITIES[gname])
    g = np.array(plan.get_gravity())
    for dtype, tol in dtypes():
        s, x = inputs(model, plan, dtype, gpu)
        zero = torch.zeros_like(x["qd"])
        V = plan.body_twists(x["q"], zero, zero)
        torch.cuda.synchronize()
        V = V.double().cpu().numpy()
        E = O.body_poses(blob, s["q"], plan.n_bodies)[:, :, :9].reshape(B, plan.n_bodies, 3, 3)
        want = np.einsum("bnij,j->bni", E, -g)
        assert not V[:, :, :6].any(), "velocity of a model at rest"
        assert np.abs(V[:, :, 6:9]).max() < tol * (1 + np.abs(g).max())
        assert np.abs(V[:, :, 9:12] - want).max() < tol * (1 + np.abs(g).max())


# ---- the later entry points: (route, model, plan-time switches, entry point), the rows of entry_points.CASES ---------------------------
# (the four-bar's draw at SEED: test_entry_draws_cpu.py holds the table's condition on it -- the reference step accepts at least 95 % of
# the states at dt = 0.05 -- at every gravity of this file; measured 100 %)
LATER = [
    ("efpa", "urdf_mini_cheetah", {}, "contact_dynamics"), ("no_efpa", "urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, "contact_dynamics"),
    ("feet", "tello_with_arms", {}, "contact_dynamics"), ("soles", "urdf_mit_humanoid", {}, "contact_dynamics_damped_fext"),
    ("explicit", "urdf_mini_cheetah", {}, "step"), ("interpreter", "urdf_mini_cheetah", {}, "step_fext"), ("newton", "urdf_four_bar", {}, "step"),
    ("explicit", "urdf_mini_cheetah", {}, "rollout"),
    ("analytic", "urdf_mini_cheetah", {}, "id_derivatives"), ("manifold", "urdf_four_bar", {}, "id_derivatives"),
    ("differences", "urdf_mini_cheetah", {"GRBDA_NO_ANALYTIC": "1"}, "id_derivatives"),
]
LATER += [(r, m, {}, e) for e in ("energy", "centroidal") for r, m in (("explicit", "urdf_mit_humanoid"), ("implicit", "tello_with_arms"),
                                                                      ("spanning_tree", "parallel_chain_exp_d10_l16"))]
# where gravity cancels: contact_points adds g to twists that carry -g; contact_impulse subtracts two forward dynamics that both hold it
CANCELS = [("feet", "urdf_mini_cheetah", {}, "contact_points"), ("feet", "tello_with_arms", {}, "contact_points"),
           ("spanning_tree", "parallel_chain_exp_d10_l16", {}, "contact_points"),
           ("efpa", "urdf_mini_cheetah", {}, "contact_impulse"), ("feet", "tello_with_arms", {}, "contact_impulse"),
           ("no_efpa", "urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, "contact_impulse")]
assert all((r, m, env, B, e) in EP.CASES for r, m, env, e in LATER + CANCELS if r != "differences")
# (No fp32 row needs an allowance against the float32 run of its reference: measured on the MI355X, every row below holds TOL32 -- and the
# 16-eps / 32-eps bounds of the stepping rows -- at all four gravities.)


@functools.lru_cache(maxsize=2)
def id_derivative_references(blob, model, max_cond):
    """id_derivative_refs.oracle_refs at the fp32-rounded states: one evaluation per (model, gravity) for both precisions"""
    import torch

    from id_derivative_refs import oracle_refs

    s = EP._host_inputs(EP._model(model), n_bodies_of(blob), B, SEED, torch.float32, max_cond)
    return oracle_refs(blob, {"q": s["q"], "qd": s["qd"], "ydd": s["tau"]})


def hold(route, model, env, entry, gname, gpu):
    """the row's outputs at gravity `gname`, fp64 and fp32 (less entry_points.NOT_RUN), through the table's checker on plan.blob"""
    import torch

    plan, blob = own_plan(model, env, GRAVITIES[gname])
    if entry == "id_derivatives" and model == "urdf_mini_cheetah":
        assert plan.info().analytic_derivatives == (0 if route == "differences" else 1)
    bound, got = EP.draw_bound(entry), {}
    for dtype, tol in dtypes():
        if (entry, model, "f64" if dtype == torch.float64 else "f32") in EP.NOT_RUN:
            continue
        if entry == "id_derivatives":  # (both precisions get the fp32-rounded states, as test_derivatives_follow_gravity's do)
            s, x = inputs(model, plan, torch.float32, gpu, bound)
            o = outputs(plan, entry, {k: v.to(dtype) for k, v in x.items()})
            EP._chk_id_derivs(blob, s, o, tol, id_derivative_references(blob, model, bound))
        else:
            s, x = inputs(model, plan, dtype, gpu, bound)
            o = outputs(plan, entry, x)
            ENTRY[entry][1](blob, s, o, tol)
        got[dtype] = o
    return got


@pytest.mark.parametrize("gname", list(GRAVITIES))
@pytest.mark.parametrize("route,model,env,entry", LATER + CANCELS, ids=[f"{e}-{r}-{m}" for r, m, _, e in LATER + CANCELS])
def test_later_entry_points_follow_gravity(route, model, env, entry, gname, gpu):
    """contact dynamics, step / rollout, the inverse-dynamics derivatives, energy and the centroidal quantities against their references
    on plan.blob at four gravities, by the checkers and bounds of entry_points.py (HELD lines: error of bound); contact points and contact
    impulses, which gravity must leave alone, the same way"""
    hold(route, model, env, entry, gname, gpu)


@pytest.mark.parametrize("route,model,env,entry", CANCELS, ids=[f"{e}-{r}-{m}" for r, m, _, e in CANCELS])
def test_gravity_cancels_bit_for_bit_where_nothing_reads_it(route, model, env, entry, gpu):
    """contact_points: position and velocity read no gravity -- the same bits at the native and the oblique one.  contact_impulse: poses,
    twists' velocity halves, the inverse OSIM and the solve read none, so the impulse has the same bits; qd_next comes from y1 - y0 of two
    forward dynamics that both hold gravity, and what that cancellation costs is printed (CANCELLATION ...), not bounded beyond the
    checker's own bound (test_later_entry_points_follow_gravity).

    Measured on the MI355X, max |qd_next(oblique) - qd_next(zero)|, fp64 / fp32: Mini Cheetah 2.3e-15 / 1.4e-6 of 34, tello_with_arms
    2.2e-15 / 1.3e-6 of 66, Mini Cheetah under GRBDA_NO_EFPA 2.7e-15 / 1.4e-6 of 34 (5.7e-13 / 1.5e-4 before the change below).

    The GRBDA_NO_EFPA row is what found that the unit-wrench route of the inverse OSIM (capi.cpp, inv_osim_unit) ran its 6 n + 1 rows of
    forward and inverse dynamics at the plan's gravity and left the cancellation to the subtraction: the impulse then differed between the
    native and the oblique gravity by 1.5e-13 of 10.4 in fp64 and 8.5e-5 of 10.4 in fp32.  Those rows now run without gravity."""
    plans = {g: own_plan(model, env, GRAVITIES[g])[0] for g in ("native", "oblique", "zero")}
    changed = []  # (asserted after both types have printed their figures)
    for dtype, _ in dtypes():
        _, x = inputs(model, plans["native"], dtype, gpu)
        o = {g: outputs(p, entry, x) for g, p in plans.items()}
        same = (0, 1) if entry == "contact_points" else (1,)
        for i in same:
            print(f"SAME BITS {entry} {route} {model} {dtype} output {i}: max |oblique - native| = {np.abs(o['oblique'][i] - o['native'][i]).max():.2e}"
                  f" of max {np.abs(o['native'][i]).max():.2e}")
        if entry == "contact_impulse":
            print(f"CANCELLATION {entry} {route} {model} {dtype}: max |qd_next(oblique) - qd_next(zero)| = {np.abs(o['oblique'][0] - o['zero'][0]).max():.2e}"
                  f" of max |qd_next| = {np.abs(o['zero'][0]).max():.2e}")
        changed += [f"{entry} {dtype}: output {i} changes with gravity" for i in same if not np.array_equal(o["native"][i], o["oblique"][i])]
    assert not changed, changed


BLIND = [("urdf_mini_cheetah", e) for e in ("mass_matrix", "fd_dtau", "inv_osim", "apply_test_force", "body_poses")] + \
        [("urdf_four_bar", e) for e in ("mass_matrix", "fd_dtau", "body_poses", "project_positions", "spanning")] + \
        [("two_parent", "mass_matrix")] + \
        [("urdf_mini_cheetah", "integrate"), ("urdf_four_bar", "integrate"), ("urdf_mit_humanoid", "centroidal_matrix"), ("tello_with_arms", "centroidal_matrix")]


@pytest.mark.parametrize("model,entry", BLIND, ids=[f"{e}-{m}" for m, e in BLIND])
def test_what_must_not_read_gravity_gives_the_same_bits(model, entry, gpu):
    native, _ = own_plan(model, {})
    oblique, _ = own_plan(model, {}, TS.OBLIQUE)
    for dtype, _ in dtypes():
        _, x = inputs(model, native, dtype, gpu)
        a, b = outputs(native, entry, x), outputs(oblique, entry, x)
        if entry == "spanning":
            a, b = a[:1], b[:1]  # (qd_span)
        assert EP.same_bits_np(a, b), f"{entry} {dtype} changes with gravity"


ORDER = [("urdf_mini_cheetah", e) for e in ("aba", "aba_fext", "rnea", "rnea_fext", "bias", "fd_dq", "fd_dqd", "fd_derivatives", "body_twists",
                                            "mass_matrix", "fd_dtau", "inv_osim", "apply_test_force", "body_poses")] + \
        [("urdf_four_bar", e) for e in ("aba", "rnea", "fd_dq", "project_positions", "spanning")] + \
        [("two_parent", e) for e in ("aba", "rnea", "fd_derivatives")] + \
        [("urdf_mini_cheetah", e) for e in ("contact_dynamics", "contact_points", "step", "id_derivatives", "energy", "centroidal")] + \
        [("parallel_chain_exp_d10_l16", e) for e in ("contact_points", "centroidal")]  # (the sub-plan the first launch made follows too)
# (where another gravity cannot give the same bits; contact_points and centroidal are not among them: the acceleration of a point and the
# rate of the momentum at a given ydd are kinematic, the gravity added at the end answers the -g the twists carry)
CHANGES = ("aba", "aba_fext", "rnea", "rnea_fext", "bias", "fd_dq", "body_twists", "contact_dynamics", "step", "id_derivatives", "energy")


@pytest.mark.parametrize("model,entry", ORDER, ids=[f"{e}-{m}" for m, e in ORDER])
def test_set_gravity_after_a_launch(model, entry, gpu):
    """A plan that has launched at its native gravity (device tables uploaded, work buffers cached; the spanning-tree plan of two_parent
    made) follows set_gravity on the next call: the bits of a fresh plan built at the oblique gravity, which the tests above hold against
    the oracle.  The native gravity again: the first result bit for bit."""
    plan, _ = own_plan(model, {})
    fresh, _ = own_plan(model, {}, TS.OBLIQUE)
    native = TS.native_gravity(EP._model(model))
    for dtype, _ in dtypes():
        _, x = inputs(model, plan, dtype, gpu, EP.draw_bound(entry))
        first = outputs(plan, entry, x)
        plan.set_gravity(TS.OBLIQUE)
        register(model, plan.blob)
        second = outputs(plan, entry, x)
        assert EP.same_bits_np(second, outputs(fresh, entry, x)), f"{entry} {dtype}: set_gravity after a launch is not a plan built at that gravity"
        if entry in CHANGES:
            assert not EP.same_bits_np(second, first), f"{entry} {dtype}: the oblique gravity changed nothing"
        plan.set_gravity(native)
        register(model, plan.blob)
        assert EP.same_bits_np(outputs(plan, entry, x), first), f"{entry} {dtype}: the native gravity set again gives other bits"
