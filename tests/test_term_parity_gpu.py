"""The fp32 kernels held to single precision term by term (run with -m gpu on an MI355X).

Every fp32 route of the library -- the one-wavefront chain kernels, latency mode on four and on two wavefronts, the interpreter, the
single-cluster kernels -- computes the sets of term_states.py: velocity-product terms alone (V), gravity alone at the model's own and at an
oblique gravity (G, Gobl), H^-1 tau / H ydd alone (T), nothing (Z) and everything (all).  The error is measured on the term's own scale and
bounded by MARGIN x what the oracle compiled in `float` loses on the same inputs (term_states.within_float); fp64 keeps TOL64 on the same
scale.  test_term_checker_cpu.py shows that a term wrong by 1 % fails these bounds and passes the norm-wise TOL32 of the other tests."""
import functools

import numpy as np
import pytest

import oracle_py as O
import term_states as TS
from term_states import model_blob, references, term_error, term_set

pytestmark = pytest.mark.gpu
TOL64 = 1e-9

# Cases in which a kernel is honestly less accurate than the float oracle: (route, model, set, entry point) ->
# (margin = 2 x the measured ratio, the measured ratio, the cause).  test_term_checker_cpu.py proves that the seeded 1 % defect of
# every case still fails at its margin.
_NEAR_SINGULAR = ("one pose of 500 next to a singular configuration of the loop: the fp64 kernel itself loses 2.4e-10 there (1e-15 elsewhere), a condition "
                  "number near 1e6, and eps32 x 1e6 is the 9e-2 measured; the float oracle's 5e-3 on that state is its operation order's luck.  "
                  "The median over the batch is 0.91 x the float oracle's")
MARGINS = {
    ("gen1", "urdf_planar_leg_linkage", "V", "rnea"): (35.4, 17.7, _NEAR_SINGULAR),
    ("gen1", "urdf_planar_leg_linkage", "V", "bias"): (35.4, 17.7, _NEAR_SINGULAR),
}

# fp64 cases that legitimately exceed TOL64 on the term's own scale: held at 5 x the error of the fp64 oracle against the long double one
FP64_AGAINST_LONG_DOUBLE = set()


def margin_of(route, model, s, which):
    return MARGINS.get((route, model, s, which), (TS.MARGIN,))[0]


@functools.lru_cache(maxsize=8)
def plan_at(route, gblob):
    """a plan of the description gblob (a set's gravity is in it) compiled under the route's switches"""
    return TS.compile_under(gblob, ROUTES[route][0])


ROUTES = TS.ROUTES
KERNEL = {  # route -> what the fp32 kernel names hold
    "chain": "{}_chain_kernel<float", "lm4": "{}_chain_lm_kernel<float, 4", "lm2": "{}_chain_lm_kernel<float, 2",
    "interpreter": "grbda_hip::{}_kernel<float", "gen1": "{}_gen1_kernel<float",
}
# The planar leg linkage is two clusters, not one: it does not take the single-cluster kernels but the generic segments of the fp32 chain
# program.  It stays with the loop mechanisms it belongs to, under the name of the kernel it runs.
KERNEL_OF = {("gen1", "urdf_planar_leg_linkage"): "{}_chain_kernel<float"}


def assert_route(route, model, plan, B):
    """fp32: the route's kernel.  fp64 has fewer programs (no latency mode for some models, the interpreter for trees with generic clusters):
    held to what distinguishes the route where fp64 has it."""
    for algo in ("aba", "rnea"):
        n32, n64 = plan.kernel_name(algo, "f32", B), plan.kernel_name(algo, "f64", B)
        assert KERNEL_OF.get((route, model), KERNEL[route]).format(algo) in n32, (route, n32)
        if route == "chain":
            assert "lm_kernel" not in n64, (route, n64)
        elif route == "interpreter":
            assert f"grbda_hip::{algo}_kernel<double" in n64, (route, n64)
        elif route == "gen1" and (route, model) not in KERNEL_OF:
            assert f"{algo}_gen1_kernel<double" in n64, (route, n64)


def run(plan, which, q, qd, x, dtype, gpu):
    import torch

    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=gpu)
    if which == "bias":
        out = plan.bias_force(t(q), t(qd))
    else:
        out = (plan.forward_dynamics if which == "aba" else plan.inverse_dynamics)(t(q), t(qd), t(x))
    torch.cuda.synchronize()
    return out.double().cpu().numpy()


ROUTE_MODELS = [(r, m) for r, (_, models) in ROUTES.items() for m in models]
TERM_CASES = [(r, m, s) for r, m in ROUTE_MODELS for s in TS.sets_of(m, "aba")]


@pytest.mark.parametrize("route,model,s", TERM_CASES, ids=[f"{r}-{m}-{s}" for r, m, s in TERM_CASES])
def test_every_term_within_single_precision(route, model, s, gpu):
    """fp32: forward dynamics, inverse dynamics and (sets without a third input) the bias force within MARGIN x the float oracle's own
    term error, worst state and median; fp64: TOL64 on the term's own scale."""
    import torch

    blob = model_blob(model)
    gblob, q, qd, x = term_set(blob, s)
    plan = plan_at(route, gblob)
    assert_route(route, model, plan, len(q))
    failures = []
    for which in ("aba", "rnea", "bias"):
        if s not in TS.sets_of(model, which):
            continue
        ref, fl = references(blob, s, which)
        got32 = run(plan, which, q, qd, x, torch.float32, gpu)
        got64 = run(plan, which, q, qd, x, torch.float64, gpu)
        worst, median = TS.float_ratio(got32, ref, fl)
        e64 = float(term_error(got64, ref).max())
        print(f"TERM {route} {model} {s} {which}: fp32 {term_error(got32, ref).max():.2e} = {worst:.2f} x float oracle (median {median:.2f} x), fp64 {e64:.2e}")
        try:
            TS.within_float(got32, ref, fl, margin_of(route, model, s, which), what=f"{route} {model} {s} {which}")
        except AssertionError as e:
            failures.append(str(e))
        bound64 = TOL64
        if (route, model, s, which) in FP64_AGAINST_LONG_DOUBLE:
            assert which == "aba"
            bound64 = 5.0 * float(term_error(ref, O.forward_dynamics_ld(gblob, q, qd, x).astype(np.float64)).max())
        if not e64 < bound64:
            failures.append(f"{route} {model} {s} {which}: fp64 term error {e64:.2e} against {bound64:.2e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("route,model", ROUTE_MODELS, ids=[f"{r}-{m}" for r, m in ROUTE_MODELS])
def test_nothing_in_gives_exactly_zero(route, model, gpu):
    """Z: zero gravity, velocity and third input.  Forward dynamics, inverse dynamics and the bias are zero in every bit but the sign,
    in both precisions, as in the oracle."""
    import torch

    gblob, q, qd, x = term_set(model_blob(model), "Z")
    assert not qd.any() and not x.any()
    plan = plan_at(route, gblob)
    assert_route(route, model, plan, len(q))
    for dtype in (torch.float32, torch.float64):
        for which in ("aba", "rnea", "bias"):
            got = run(plan, which, q, qd, x, dtype, gpu)
            assert (got == 0).all(), f"{which} {dtype}: {int((got != 0).sum())} non-zero values, largest {np.abs(got).max():.2e}"


@pytest.mark.parametrize("name", TS.COMPONENT_MODELS)
def test_componentwise_parity_fp32(name, gpu):
    """test_componentwise_parity_fp64 for single precision, on the `all` set: every component on its own,
    |got_i - ref_i| / (|ref_i| + 1e-3 |ref|_inf), at most MARGIN x the worst of the float oracle (1.2e-5 to 3.8e-4 on these models and states).  The
    plan is the default one: latency mode for the robots at this batch size, the single-cluster kernels for the six-bar."""
    import torch
    import generalized_rbda_amd as G

    blob = model_blob(name)
    gblob, q, qd, x = term_set(blob, "all")
    plan = G.Plan(gblob)
    failures = []
    for which in ("aba", "rnea"):
        ref, fl = references(blob, "all", which)
        got = run(plan, which, q, qd, x, torch.float32, gpu)
        e, f = TS.component_error(got, ref), TS.component_error(fl, ref)
        print(f"COMPONENT {name} {which}: {e:.2e} = {e / f:.2f} x float oracle ({f:.2e}), kernel {plan.kernel_name(which, 'f32', len(q))}")
        if not e <= TS.MARGIN * f:
            failures.append(f"{which}: worst component error {e:.2e} against {f:.2e} of the float oracle ({e / f:.1f} x)")
    assert not failures, "\n".join(failures)
