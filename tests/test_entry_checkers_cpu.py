"""The checkers of the later rows of the entry-point table have teeth (no GPU): each is fed the reference's own output, which it must
pass at the fp64 and at the fp32 tolerance, and then the same output with one deliberate fault, which it must refuse at both:
state B - 1 replaced by state B - 2 (every checker); one contact's offset dropped (the contact checkers); one sign flipped in hdot
(centroidal); ok inverted on one state (integrate, step, rollout)."""
import numpy as np
import pytest

import centroidal_ref as CR
import contact_ref as C
import generalized_rbda_amd as G
import integrate_ref as R
import oracle_py as O
from entry_points import CASES, DAMPING, ENTRY, T_ROLL, TOL32, TOL64, _big, _contacts, _dt, _host_inputs, _model, draw_bound
from generalized_rbda_amd.states import parse_clusters
from id_derivative_refs import oracle_refs

B = 6
SEED = 11
NEW = ("id_derivatives", "integrate", "step", "step_fext", "rollout", "contact_points", "contact_dynamics", "contact_dynamics_damped_fext", "energy",
       "centroidal", "centroidal_matrix")
ROWS = sorted({(c[4], c[1]) for c in CASES if c[4] in NEW})
assert {e for e, _ in ROWS} == set(NEW)
# rows whose outputs do not depend on the state beyond their bounds, so that a swapped state is no fault: the four-bar is a parallelogram
# with one coordinate -- H is constant and the velocity-product term 1e-17 (term_states.NOT_RUN), so d tau / d ydd is one number and the
# other two derivatives vanish.  Held instead: d tau / d ydd off by 1e-6 of itself is refused in fp64.
SAME_IN_EVERY_STATE = {("id_derivatives", "urdf_four_bar")}


def reference_outputs(entry, blob, s, offsets=None):
    """what the entry point's call returns, from the references alone; offsets: other contact offsets than the table's"""
    q, qd, tau, big = s["q"], s["qd"], s["tau"], _big(blob)
    bodies, table_offsets = _contacts(blob)
    offsets = table_offsets if offsets is None else offsets
    if entry == "id_derivatives":
        ref = oracle_refs(blob, {"q": q, "qd": qd, "ydd": tau})
        return [ref["dq"], ref["dqd"], ref["dydd"]]
    if entry == "integrate":
        qn, vn, ok, _ = R.reference_step(blob, q, qd, tau, _dt(blob), big=big)
        return [qn, vn, ok]
    if entry in ("step", "step_fext"):
        ydd = O.forward_dynamics(blob, q, qd, tau, s["fext"] if entry == "step_fext" else None, big=big)
        qn, vn, ok, _ = R.reference_step(blob, q, qd, ydd, _dt(blob), big=big)
        return [qn, vn, ydd, ok]
    if entry == "rollout":
        qt, vt, ok = [], [], np.ones(len(q), dtype=bool)
        for k in range(T_ROLL):
            q, qd, ok_k, _ = R.reference_step(blob, q, qd, O.forward_dynamics(blob, q, qd, s["tau_T"][:, k], big=big), _dt(blob), big=big)
            qt.append(q), vt.append(qd)
            ok = ok & ok_k
        return [np.stack(qt, axis=1), np.stack(vt, axis=1), ok]
    if entry == "contact_points":
        return list(C.contact_points(blob, q, bodies, offsets, qd, tau))
    if entry.startswith("contact_dynamics"):
        damped = entry.endswith("damped_fext")
        ref = C.contact_dynamics(blob, q, qd, tau, bodies, offsets, s["a_des"], DAMPING if damped else 0.0, s["fext"] if damped else None)
        return [ref["ydd"], ref["lam"], ref["ydd_free"]]
    if entry == "energy":
        ref = CR.centroidal(blob, q, qd, big=big)
        return [ref["kinetic"], ref["potential"]]
    if entry == "centroidal":
        ref = CR.centroidal(blob, q, qd, tau, big=big)
        return [ref[k] for k in ("com", "com_vel", "h", "hdot")]
    assert entry == "centroidal_matrix"
    return [CR.momentum_matrix(blob, q, big=big)]


def refused(check, blob, s, outs):
    for tol in (TOL64, TOL32):
        with pytest.raises(AssertionError):
            check(blob, s, outs, tol)


@pytest.mark.parametrize("entry,model", ROWS, ids=[f"{e}-{m}" for e, m in ROWS])
def test_checker_passes_the_reference_and_refuses_each_fault(entry, model):
    blob = _model(model)
    check = ENTRY[entry][1]
    s = _host_inputs(blob, G.Plan(blob).n_bodies, B, SEED, __import__("torch").float64, draw_bound(entry))
    good = reference_outputs(entry, blob, s)
    for tol in (TOL64, TOL32):
        check(blob, s, [np.array(o) for o in good], tol)
    # state B - 1 replaced by state B - 2, in every output that differs between the two
    moved = [np.array(o) for o in good]
    for o in moved:
        o[B - 1] = o[B - 2]
    assert any(not np.array_equal(a, b) for a, b in zip(moved, good))
    if (entry, model) in SAME_IN_EVERY_STATE:
        scaled = [np.array(o) for o in good]
        scaled[2] *= 1.0 + 1e-6
        with pytest.raises(AssertionError):
            check(blob, s, scaled, TOL64)
    else:
        refused(check, blob, s, moved)
    if entry.startswith("contact"):
        bodies, offsets = _contacts(blob)
        dropped = [tuple(o) for o in offsets]
        dropped[-1] = (0.0, 0.0, 0.0)
        refused(check, blob, s, reference_outputs(entry, blob, s, dropped))
    if entry == "centroidal":
        flipped = [np.array(o) for o in good]
        flipped[3][B // 2, 4] *= -1.0
        refused(check, blob, s, flipped)
    if entry in ("integrate", "step", "step_fext", "rollout"):
        inverted = [np.array(o) for o in good]
        inverted[-1][B // 2] = ~inverted[-1][B // 2]
        with pytest.raises(AssertionError):
            check(blob, s, inverted, TOL64)
        # (step's fp32 flag of a model with implicit clusters is not held: entry_points._hold_dynamics_step)
        if entry == "integrate" or not any(c[9] in (2, 3) for c in parse_clusters(blob)["clusters"]):
            with pytest.raises(AssertionError):
                check(blob, s, inverted, TOL32)
