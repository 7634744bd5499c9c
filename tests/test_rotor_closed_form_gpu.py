"""The closed-form axisymmetric rotor of the chain ABA against the oracle, on states where it is the whole answer (run with -m gpu).

chain_kernels.hip evaluates an axisymmetric rotor as tp = om (vp x* X0^T h) and leaves vp x* (X0^T I X0) vp to the bias force of the body
the rotor hangs off (tests/test_rotor_identity_cpu.py proves the identity).  With tau = 0 and gravity zero the forward dynamics is made of
velocity-product terms alone, so a rotor term that is missing, doubled or evaluated with the wrong parent shows at full size:

* the fixed-base chain of links with rotors (the first rotor hangs off the ground: vp = 0), Mini Cheetah, and the MIT Humanoid (leaf pairs
  with two rotors each, rotors on the floating base's children);
* the one-wavefront kernel on 193 states (three full tiles and a ragged tail), latency mode on four and on two wavefronts on 70;
* joint rates of the reference's sampling law times 1, 10 and 30 (the base as drawn), the joints moving with the base at rest (every
  rotor of a limb's first cluster then has vp = 0 and the linear term alone is left below it), and the base moving with the joints at rest
  (om = 0: only the quadratic terms, all of them produced by the parents' bias forces; floating bases only -- a fixed-base model at rest
  has no state of this kind).

fp64 keeps TOL64 on the term's own scale; fp32 is bounded by MARGIN x what the oracle compiled in `float` loses on the same inputs
(term_states.within_float)."""
import functools

import numpy as np
import pytest

import oracle_py as O
import term_states as TS
from generalized_rbda_amd.modeldesc import C_FREE
from generalized_rbda_amd.states import parse_clusters

pytestmark = pytest.mark.gpu
TOL64 = 1e-9
B_CHAIN, B_LM = 193, 70
MODELS = ("urdf_revolute_rotor_chain", "urdf_mini_cheetah", "urdf_mit_humanoid")
ROUTES = ("chain", "lm4", "lm2")
KERNEL = {"chain": "aba_chain_kernel<float", "lm4": "aba_chain_lm_kernel<float, 4", "lm2": "aba_chain_lm_kernel<float, 2"}
STATES = ("rate1", "rate10", "rate30", "joints_only", "base_only")


def base_rates(blob):
    """the velocity coordinates of the floating base (empty: fixed base)"""
    return [j for c in parse_clusters(blob)["clusters"] if c[9] == C_FREE for j in range(c[5], c[5] + c[6])]


def has_case(model, state):
    return state != "base_only" or bool(base_rates(TS.model_blob(model)))


CASES = [(r, m, s) for r in ROUTES for m in MODELS for s in STATES if has_case(m, s)]


@functools.lru_cache(maxsize=None)
def inputs(model, state, B):
    """(zero-gravity blob, q, qd, tau = 0, fp64 oracle, float oracle): fp32-representable, computed once, read-only"""
    blob = TS.model_blob(model)
    gblob = TS._blob_at(blob, "zero")
    q, qd, _ = TS._draw(blob, B, TS.SEED)
    base = base_rates(blob)
    joints = [j for j in range(qd.shape[1]) if j not in base]
    qd = np.array(qd)
    if state.startswith("rate"):
        qd[:, joints] *= float(state[4:])
    elif state == "joints_only":
        qd[:, joints] *= 10.0
        qd[:, base] = 0.0
    else:
        qd[:, joints] = 0.0
    qd = TS._frozen(TS.fp32_rounded(qd))
    tau = TS._frozen(np.zeros_like(qd))
    ref = TS._frozen(O.forward_dynamics(gblob, q, qd, tau))
    fl = TS._frozen(O.forward_dynamics_f32(gblob, q, qd, tau).astype(np.float64))
    return gblob, q, qd, tau, ref, fl


@functools.lru_cache(maxsize=None)
def plan_at(route, model):
    return TS.compile_under(TS._blob_at(TS.model_blob(model), "zero"), TS.ROUTES[route][0])


@pytest.mark.parametrize("route,model,state", CASES, ids=[f"{r}-{m}-{s}" for r, m, s in CASES])
def test_velocity_products_with_closed_form_rotors(route, model, state, gpu):
    import torch

    B = B_CHAIN if route == "chain" else B_LM
    gblob, q, qd, tau, ref, fl = inputs(model, state, B)
    plan = plan_at(route, model)
    name = plan.kernel_name("aba", "f32", B)
    if model in TS.ROUTES[route][1]:
        assert KERNEL[route] in name, (route, name)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=gpu)
    got32 = plan.forward_dynamics(t(q, torch.float32), t(qd, torch.float32), t(tau, torch.float32))
    got64 = plan.forward_dynamics(t(q, torch.float64), t(qd, torch.float64), t(tau, torch.float64))
    torch.cuda.synchronize()
    got32, got64 = got32.double().cpu().numpy(), got64.cpu().numpy()
    e64 = float(TS.term_error(got64, ref).max())
    worst, median = TS.float_ratio(got32, ref, fl)
    print(f"ROTOR {route} {model} {state} B={B} {name}: |ydd| median {np.median(np.abs(ref).max(axis=1)):.2e}, fp32 "
          f"{TS.term_error(got32, ref).max():.2e} = {worst:.2f} x float oracle (median {median:.2f} x), fp64 {e64:.2e}")
    assert e64 < TOL64, f"fp64 term error {e64:.2e}"
    TS.within_float(got32, ref, fl, what=f"{route} {model} {state}")
