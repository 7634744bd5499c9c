"""The checkers of the later rows of the entry-point table have teeth (no GPU): each is fed the reference's own output, which it must
pass at the fp64 and at the fp32 tolerance, and then the same output with one deliberate fault, which it must refuse at both:
state B - 1 replaced by state B - 2 (every checker); one contact's offset dropped (the contact checkers); one sign flipped in hdot
(centroidal); ok inverted on one state (integrate, step, rollout); the impulse with the wrong sign (contact_impulse).

Then the gravity rows of test_gravity_gpu.py: at the oblique gravity, on the states that file runs, every checker refuses the
reference's own outputs computed at another gravity -- x and y swapped, the sign of x flipped, the native gravity -- output by output
at the fp32 tolerance, so the oblique gravity moves every held output by more than TOL32; NOT_MOVED names the outputs gravity does not
move and NOT_MOVED_ENOUGH those it moves by less than the row's bound, with the reasons, and what is listed is asserted to pass.
contact_points' acceleration with swap(g) - g added, and centroidal's hdot with M (swap(g) - g), are refused."""
import numpy as np
import pytest

import centroidal_ref as CR
import contact_ref as C
import impulse_ref as I
import generalized_rbda_amd as G
import integrate_ref as R
import oracle_py as O
from entry_points import CASES, DAMPING, ENTRY, RESTITUTION, T_ROLL, TOL32, TOL64, _big, _contacts, _dt, _host_inputs, _model, draw_bound
from generalized_rbda_amd.states import parse_clusters
from id_derivative_refs import oracle_refs

B = 6
SEED = 11
NEW = ("id_derivatives", "integrate", "step", "step_fext", "rollout", "contact_points", "contact_dynamics", "contact_dynamics_damped_fext", "energy",
       "centroidal", "centroidal_matrix", "contact_impulse")
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
    if entry == "contact_impulse":
        ref = I.contact_impulse(blob, q, qd, bodies, offsets, s["v_des"], RESTITUTION, 0.0)
        return [ref["qd_next"], ref["impulse"]]
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
    if entry == "contact_impulse":
        flipped = [np.array(o) for o in good]
        flipped[1] *= -1.0
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


# ---- the gravity rows of test_gravity_gpu.py can fail ------------------------------------------------------------------------------------
OUTPUTS = {"contact_dynamics": ("ydd", "lambda", "ydd_free"), "contact_dynamics_damped_fext": ("ydd", "lambda", "ydd_free"),
           "step": ("q'", "qd'", "ydd", "ok"), "step_fext": ("q'", "qd'", "ydd", "ok"), "rollout": ("q_t", "qd_t", "ok"),
           "id_derivatives": ("dq", "dqd", "dydd"), "energy": ("kinetic", "potential"), "centroidal": ("com", "com_vel", "h", "hdot")}
# (entry point, output) that no gravity moves, on every model: the checker cannot tell one gravity from another there, and need not
NOT_MOVED = {
    ("step", "ok"): "the flag of the projection: explicit models accept every state, the four-bar's reference every state of the draw",
    ("step_fext", "ok"): "as step",
    ("rollout", "ok"): "as step",
    ("id_derivatives", "dqd"): "d tau / d qd is made of velocity-product terms: gravity does not enter",
    ("id_derivatives", "dydd"): "d tau / d ydd is the mass matrix",
    ("energy", "kinetic"): "1/2 yd^T H yd",
    ("centroidal", "com"): "the centre of mass is kinematic",
    ("centroidal", "com_vel"): "as com",
    ("centroidal", "h"): "the momentum is A(q) yd",
    ("centroidal", "hdot"): "the rate of A(q) yd at the ydd given: the M g added at the end answers the -g the twists carry, as in contact_points "
                            "(test_centroidal_rate_refuses_another_g_added_back: the kernel's own M g can be wrong, and then shows)",
}
# (entry point, model, output): (the wrong gravities that pass at TOL32 on these states, the reason)
NOT_MOVED_ENOUGH = {
    ("step_fext", "urdf_mini_cheetah", "q'"): (("x and y swapped", "x flipped", "native"),
                                               "f_ext in U(-1, 1) on every body, rotors included, gives max |ydd| = 3.6e3 (2.7e2 without), and the step is held on the scale "
                                               "1 + |ref| + dt max |ydd| = 1.8e3: dt^2 |dg| = 0.5 is 2.7e-4 of it.  The row's ydd, on its own scale, refuses "
                                               "all three, and the step row without f_ext refuses q' and qd'."),
    ("step_fext", "urdf_mini_cheetah", "qd'"): (("x flipped", "native"), "as q': dt |dg| = 1.6 is 8.8e-4 of that scale; x and y swapped (2.0) is refused"),
}


def wrong_gravities(blob):
    import term_states as TS

    g = TS.OBLIQUE
    return {"x and y swapped": (g[1], g[0], g[2]), "x flipped": (-g[0], g[1], g[2]), "native": TS.native_gravity(blob)}


def _gravity_rows():
    import test_gravity_gpu as TG

    return TG, sorted({(e, m) for _, m, _, e in TG.LATER})


def _at(TG, model, g):
    """the description of `model` at gravity g, known to entry_points under the model's name as test_gravity_gpu.own_plan leaves it"""
    import entry_points as EP
    import term_states as TS

    blob = TS.with_gravity(_model(model), g)
    if _big(_model(model)):
        EP._BIG.add(blob)
    TG.register(model, blob)
    return blob


def _check(entry, blob, s, outs, tol, good):
    """the table's checker; id_derivatives with the references already at hand (its oracle differentiates state by state)"""
    if entry == "id_derivatives":
        import entry_points as EP

        return EP._chk_id_derivs(blob, s, outs, tol, dict(zip(("dq", "dqd", "dydd"), good)))
    return ENTRY[entry][1](blob, s, outs, tol)


@pytest.mark.parametrize("entry,model", _gravity_rows()[1], ids=[f"{e}-{m}" for e, m in _gravity_rows()[1]])
def test_gravity_rows_refuse_the_outputs_of_another_gravity(entry, model):
    import term_states as TS

    TG, _ = _gravity_rows()
    blob = _at(TG, model, TS.OBLIQUE)
    s = _host_inputs(_model(model), G.Plan(_model(model)).n_bodies, TG.B, TG.SEED, __import__("torch").float32, draw_bound(entry))
    good = reference_outputs(entry, blob, s)
    _check(entry, blob, s, [np.array(o) for o in good], TOL32, good)
    for what, g in wrong_gravities(_model(model)).items():
        wrong = reference_outputs(entry, _at(TG, model, g), s)
        for i, name in enumerate(OUTPUTS[entry]):
            outs = [np.array(o) for o in good]
            outs[i] = np.array(wrong[i])
            moved = np.abs(np.asarray(wrong[i], dtype=float) - np.asarray(good[i], dtype=float)).max()
            print(f"MOVED {entry} {model} {name}, {what}: {moved:.2e}")
            if (entry, name) in NOT_MOVED or what in NOT_MOVED_ENOUGH.get((entry, model, name), ((),))[0]:
                _check(entry, blob, s, outs, TOL32, good)  # (listed: then it does pass)
                continue
            with pytest.raises(AssertionError):
                _check(entry, blob, s, outs, TOL32, good)


@pytest.mark.parametrize("model", ["urdf_mini_cheetah", "tello_with_arms", "parallel_chain_exp_d10_l16"])
def test_contact_points_refuse_an_acceleration_with_another_g_added(model):
    """gravity cancels in contact_points, so the reference at another gravity is the same; what the kernel can get wrong is the g it adds
    back: swap(g) - g on every point's acceleration"""
    import term_states as TS

    TG, _ = _gravity_rows()
    blob = _at(TG, model, TS.OBLIQUE)
    s = _host_inputs(_model(model), G.Plan(_model(model)).n_bodies, TG.B, TG.SEED, __import__("torch").float32)
    good = reference_outputs("contact_points", blob, s)
    check = ENTRY["contact_points"][1]
    check(blob, s, [np.array(o) for o in good], TOL32)
    g = np.array(TS.OBLIQUE)
    for what, w in wrong_gravities(_model(model)).items():
        outs = [np.array(o) for o in good]
        outs[2] = outs[2] + (np.array(w) - g)[None, None]
        with pytest.raises(AssertionError):
            check(blob, s, outs, TOL32)


@pytest.mark.parametrize("model", ["urdf_mit_humanoid", "tello_with_arms", "parallel_chain_exp_d10_l16"])
def test_centroidal_rate_refuses_another_g_added_back(model):
    """hdot's linear part with M (w - g) added, w each wrong gravity: what centroidal_kernel gives if its own copy of g is wrong"""
    import term_states as TS

    TG, _ = _gravity_rows()
    blob = _at(TG, model, TS.OBLIQUE)
    s = _host_inputs(_model(model), G.Plan(_model(model)).n_bodies, TG.B, TG.SEED, __import__("torch").float32)
    good = reference_outputs("centroidal", blob, s)
    check = ENTRY["centroidal"][1]
    check(blob, s, [np.array(o) for o in good], TOL32)
    for what, w in wrong_gravities(_model(model)).items():
        outs = [np.array(o) for o in good]
        outs[3][:, 3:] += CR.total_mass(blob) * (np.array(w) - np.array(TS.OBLIQUE))[None]
        with pytest.raises(AssertionError):
            check(blob, s, outs, TOL32)
