"""Which rule wins when a call of the product family breaks two at once -- every entry point of include/grbda_hip_vjp.h,
grbda_hip_step_vjp.h and grbda_hip_jvp.h, device (f64, f32) and host variants alike, bound as test_jvp_args_cpu.py binds them.  All of them
go through one rule function (capi.cpp, product_rules) that applies one ordered list: S a state input is missing, T every optional
(co)tangent is, O every output that counts is, D dt is not finite, V two arrays overlap, P the plan is outside the contract of the step,
Q the step is not positive where differences in q are taken.  A case is a pair of these letters; the models are four_bar (implicit
clusters) and mini_cheetah_rpy (roll-pitch-yaw base), which the stepping entry points refuse (P) and the dynamics products accept, and
tree65_fixed (65 velocities: every entry point accepts it, and it is off the analytic route) for the pairs without P.

WHERE THE TABLE COMES FROM.  The rows of EXPECTED were recorded from the library of the commit before the rule functions of the three
headers were folded into one (its vjp_args, step_vjp_rules and jvp_rules), built on a machine without a device, by running exactly the
calls below against it -- not from the code under test.  The f64, f32 and host variants of an entry point agreed on every row there, so a
row stands for all of them.  The rules never read the arrays and are decided before a device is looked at, so the host buffers that stand
in for device arrays are never touched."""
import numpy as np
import pytest

import generalized_rbda_amd as G
from id_derivative_refs import blob_of

T = 3
MESSAGES = {
    "null": "null argument",
    "cotangent": "both cotangents are null",
    "tangent": "all tangents are null",
    "output": "no output asked for",
    "dt": "dt is not finite",
    "in_out": "an output array overlaps an input array",
    "out_out": "two output arrays overlap",
    "rpy": "time stepping covers the quaternion floating base only: the rate map of a roll-pitch-yaw base is not built",
    "implicit": "the vector-Jacobian products of integrate, step and rollout do not cover implicit clusters: the Jacobian of the Newton "
                "re-projection is not built",
    "step": "step must be positive",
}
# group: (variants, the arguments in order, state inputs, optional (co)tangents, outputs that count, all outputs)
VJP_ARGS = ["q", "qd", "x", "g", "STEP", "o0", "o1", "o2"]
JVP_ARGS = ["q", "qd", "x", "dq", "dqd", "dx", "STEP", "o0"]
GROUPS = {
    "rnea_vjp": (("f64", "f32", "host_f64"), VJP_ARGS, ("q", "qd", "x", "g"), (), ("o0", "o1", "o2"), 3),
    "aba_vjp": (("f64", "f32", "host_f64"), VJP_ARGS + ["o3"], ("q", "qd", "x", "g"), (), ("o0", "o1", "o2"), 4),
    "integrate_vjp": (("f64", "f32"), ["qd_next", "DT", "g_q", "g_qd", "o0", "o1", "o2"], ("qd_next",), ("g_q", "g_qd"), ("o0", "o1", "o2"), 3),
    "step_vjp": (("f64", "f32", "host_f64"), ["q", "qd", "x", "qd_next", "DT", "g_q", "g_qd", "STEP", "o0", "o1", "o2"], ("q", "qd", "x", "qd_next"),
                 ("g_q", "g_qd"), ("o0", "o1", "o2"), 3),
    "rollout_vjp": (("f64", "f32"), ["q", "qd", "q_traj", "qd_traj", "x", "ONE", "DT", "T", "g_q", "g_qd", "ONE", "STEP", "o0", "o1", "o2"],
                    ("q", "qd", "q_traj", "qd_traj", "x"), ("g_q", "g_qd"), ("o0", "o1", "o2"), 3),
    "rnea_jvp": (("f64", "f32", "host_f64"), JVP_ARGS, ("q", "qd", "x"), ("dq", "dqd", "dx"), ("o0",), 1),
    "aba_jvp": (("f64", "f32", "host_f64"), JVP_ARGS + ["o1"], ("q", "qd", "x"), ("dq", "dqd", "dx"), ("o0",), 2),
    "integrate_jvp": (("f64", "f32"), ["qd_next", "DT", "dq", "dqd", "dx", "o0", "o1"], ("qd_next",), ("dq", "dqd", "dx"), ("o0", "o1"), 2),
    "step_jvp": (("f64", "f32", "host_f64"), ["q", "qd", "x", "qd_next", "DT", "dq", "dqd", "dx", "STEP", "o0", "o1"], ("q", "qd", "x", "qd_next"),
                 ("dq", "dqd", "dx"), ("o0", "o1"), 2),
}
ENTRY_POINTS = tuple(f"grbda_{g}_{v}" for g, spec in GROUPS.items() for v in spec[0])
UNSUPPORTED = ("four_bar", "mini_cheetah_rpy")


def rules_of(group):
    """the letters of the rules the entry points of a group have, in the order they are applied"""
    _, args, _, tangents, _, _ = GROUPS[group]
    return "S" + ("T" if tangents else "") + "O" + ("D" if "DT" in args else "") + "V" + ("P" if "DT" in args else "") + ("Q" if "STEP" in args else "")


def cases_of(group):
    """(pair, model) for every pair of rules of the group that one call can break together (no output asked for leaves nothing to overlap)"""
    r = rules_of(group)
    for i in range(len(r)):
        for j in range(i + 1, len(r)):
            if (r[i], r[j]) == ("O", "V"):
                continue
            models = UNSUPPORTED if "P" in (r[i], r[j]) or "P" not in r else ("tree65_fixed",)
            for model in models:
                yield r[i] + "+" + r[j], model


class _Call:
    """one plan and host buffers of B states (T steps where the rollout wants them) standing in for the arrays"""

    def __init__(self, model, B=3):
        self.plan = G.Plan(blob_of(model))
        nq, nv = self.plan.nq, self.plan.nv
        self.B = B
        z = lambda *shape: np.zeros(shape)
        self.buf = dict(q=z(B, nq), qd=z(B, nv), x=z(T, B, nv), g=z(B, nv), qd_next=z(B, nv), g_q=z(T, B, nv), g_qd=z(T, B, nv), dq=z(B, nv),
                        dqd=z(B, nv), dx=z(B, nv), q_traj=z(T, B, nq), qd_traj=z(T, B, nv), o0=z(T, B, nv), o1=z(T, B, nv), o2=z(T, B, nv), o3=z(B, nv))

    def __call__(self, group, variant, broken):
        _, args, state, tangents, counted, n_out = GROUPS[group]
        at = {name: name for name in self.buf}  # argument -> the buffer it points to (None: a null pointer)
        dt, step = 0.01, 1e-6
        if "S" in broken:
            at[state[0]] = None
        if "T" in broken:
            at.update({name: None for name in tangents})
        if "O" in broken:
            at.update({name: None for name in counted})
        if "D" in broken:
            dt = float("nan")
        if "V" in broken:  # the second output on the first; the one output of grbda_rnea_jvp_* on an input
            at.update({"o1": "o0"} if n_out > 1 else {"o0": "qd"})
        if "Q" in broken:
            step = 0.0
        scalars = dict(STEP=step, DT=dt, ONE=1, T=T)
        ptr = lambda name: None if at[name] is None else self.buf[at[name]].ctypes.data
        call = [self.plan._h] + [scalars[a] if a in scalars else ptr(a) for a in args] + [self.B, 0] + ([] if variant.startswith("host") else [None])
        code = getattr(G.lib(), f"grbda_{group}_{variant}")(*call)
        return code, G.lib().grbda_last_error().decode()


_calls = {}


def outcome(group, variant, case, model):
    if model not in _calls:
        _calls[model] = _Call(model)
    return _calls[model](group, variant, case.split("+"))


# group  case  model  code  message (a key of MESSAGES) -- recorded from the parent commit's library, see the docstring
EXPECTED = """
rnea_vjp       S+O four_bar          -1 null
rnea_vjp       S+O mini_cheetah_rpy  -1 null
rnea_vjp       S+V four_bar          -1 null
rnea_vjp       S+V mini_cheetah_rpy  -1 null
rnea_vjp       S+Q four_bar          -1 null
rnea_vjp       S+Q mini_cheetah_rpy  -1 null
rnea_vjp       O+Q four_bar          -1 output
rnea_vjp       O+Q mini_cheetah_rpy  -1 output
rnea_vjp       V+Q four_bar          -1 out_out
rnea_vjp       V+Q mini_cheetah_rpy  -1 out_out
aba_vjp        S+O four_bar          -1 null
aba_vjp        S+O mini_cheetah_rpy  -1 null
aba_vjp        S+V four_bar          -1 null
aba_vjp        S+V mini_cheetah_rpy  -1 null
aba_vjp        S+Q four_bar          -1 null
aba_vjp        S+Q mini_cheetah_rpy  -1 null
aba_vjp        O+Q four_bar          -1 output
aba_vjp        O+Q mini_cheetah_rpy  -1 output
aba_vjp        V+Q four_bar          -1 out_out
aba_vjp        V+Q mini_cheetah_rpy  -1 out_out
integrate_vjp  S+T tree65_fixed      -1 null
integrate_vjp  S+O tree65_fixed      -1 null
integrate_vjp  S+D tree65_fixed      -1 null
integrate_vjp  S+V tree65_fixed      -1 null
integrate_vjp  S+P four_bar          -1 null
integrate_vjp  S+P mini_cheetah_rpy  -1 null
integrate_vjp  T+O tree65_fixed      -1 cotangent
integrate_vjp  T+D tree65_fixed      -1 cotangent
integrate_vjp  T+V tree65_fixed      -1 cotangent
integrate_vjp  T+P four_bar          -1 cotangent
integrate_vjp  T+P mini_cheetah_rpy  -1 cotangent
integrate_vjp  O+D tree65_fixed      -1 output
integrate_vjp  O+P four_bar          -1 output
integrate_vjp  O+P mini_cheetah_rpy  -1 output
integrate_vjp  D+V tree65_fixed      -1 dt
integrate_vjp  D+P four_bar          -1 dt
integrate_vjp  D+P mini_cheetah_rpy  -1 dt
integrate_vjp  V+P four_bar          -1 out_out
integrate_vjp  V+P mini_cheetah_rpy  -1 out_out
step_vjp       S+T tree65_fixed      -1 null
step_vjp       S+O tree65_fixed      -1 null
step_vjp       S+D tree65_fixed      -1 null
step_vjp       S+V tree65_fixed      -1 null
step_vjp       S+P four_bar          -1 null
step_vjp       S+P mini_cheetah_rpy  -1 null
step_vjp       S+Q tree65_fixed      -1 null
step_vjp       T+O tree65_fixed      -1 cotangent
step_vjp       T+D tree65_fixed      -1 cotangent
step_vjp       T+V tree65_fixed      -1 cotangent
step_vjp       T+P four_bar          -1 cotangent
step_vjp       T+P mini_cheetah_rpy  -1 cotangent
step_vjp       T+Q tree65_fixed      -1 cotangent
step_vjp       O+D tree65_fixed      -1 output
step_vjp       O+P four_bar          -1 output
step_vjp       O+P mini_cheetah_rpy  -1 output
step_vjp       O+Q tree65_fixed      -1 output
step_vjp       D+V tree65_fixed      -1 dt
step_vjp       D+P four_bar          -1 dt
step_vjp       D+P mini_cheetah_rpy  -1 dt
step_vjp       D+Q tree65_fixed      -1 dt
step_vjp       V+P four_bar          -1 out_out
step_vjp       V+P mini_cheetah_rpy  -1 out_out
step_vjp       V+Q tree65_fixed      -1 out_out
step_vjp       P+Q four_bar          -2 implicit
step_vjp       P+Q mini_cheetah_rpy  -2 rpy
rollout_vjp    S+T tree65_fixed      -1 null
rollout_vjp    S+O tree65_fixed      -1 null
rollout_vjp    S+D tree65_fixed      -1 null
rollout_vjp    S+V tree65_fixed      -1 null
rollout_vjp    S+P four_bar          -1 null
rollout_vjp    S+P mini_cheetah_rpy  -1 null
rollout_vjp    S+Q tree65_fixed      -1 null
rollout_vjp    T+O tree65_fixed      -1 cotangent
rollout_vjp    T+D tree65_fixed      -1 cotangent
rollout_vjp    T+V tree65_fixed      -1 cotangent
rollout_vjp    T+P four_bar          -1 cotangent
rollout_vjp    T+P mini_cheetah_rpy  -1 cotangent
rollout_vjp    T+Q tree65_fixed      -1 cotangent
rollout_vjp    O+D tree65_fixed      -1 output
rollout_vjp    O+P four_bar          -1 output
rollout_vjp    O+P mini_cheetah_rpy  -1 output
rollout_vjp    O+Q tree65_fixed      -1 output
rollout_vjp    D+V tree65_fixed      -1 dt
rollout_vjp    D+P four_bar          -1 dt
rollout_vjp    D+P mini_cheetah_rpy  -1 dt
rollout_vjp    D+Q tree65_fixed      -1 dt
rollout_vjp    V+P four_bar          -1 out_out
rollout_vjp    V+P mini_cheetah_rpy  -1 out_out
rollout_vjp    V+Q tree65_fixed      -1 out_out
rollout_vjp    P+Q four_bar          -2 implicit
rollout_vjp    P+Q mini_cheetah_rpy  -2 rpy
rnea_jvp       S+T four_bar          -1 null
rnea_jvp       S+T mini_cheetah_rpy  -1 null
rnea_jvp       S+O four_bar          -1 null
rnea_jvp       S+O mini_cheetah_rpy  -1 null
rnea_jvp       S+V four_bar          -1 null
rnea_jvp       S+V mini_cheetah_rpy  -1 null
rnea_jvp       S+Q four_bar          -1 null
rnea_jvp       S+Q mini_cheetah_rpy  -1 null
rnea_jvp       T+O four_bar          -1 tangent
rnea_jvp       T+O mini_cheetah_rpy  -1 tangent
rnea_jvp       T+V four_bar          -1 tangent
rnea_jvp       T+V mini_cheetah_rpy  -1 tangent
rnea_jvp       T+Q four_bar          -1 tangent
rnea_jvp       T+Q mini_cheetah_rpy  -1 tangent
rnea_jvp       O+Q four_bar          -1 output
rnea_jvp       O+Q mini_cheetah_rpy  -1 output
rnea_jvp       V+Q four_bar          -1 in_out
rnea_jvp       V+Q mini_cheetah_rpy  -1 in_out
aba_jvp        S+T four_bar          -1 null
aba_jvp        S+T mini_cheetah_rpy  -1 null
aba_jvp        S+O four_bar          -1 null
aba_jvp        S+O mini_cheetah_rpy  -1 null
aba_jvp        S+V four_bar          -1 null
aba_jvp        S+V mini_cheetah_rpy  -1 null
aba_jvp        S+Q four_bar          -1 null
aba_jvp        S+Q mini_cheetah_rpy  -1 null
aba_jvp        T+O four_bar          -1 tangent
aba_jvp        T+O mini_cheetah_rpy  -1 tangent
aba_jvp        T+V four_bar          -1 tangent
aba_jvp        T+V mini_cheetah_rpy  -1 tangent
aba_jvp        T+Q four_bar          -1 tangent
aba_jvp        T+Q mini_cheetah_rpy  -1 tangent
aba_jvp        O+Q four_bar          -1 output
aba_jvp        O+Q mini_cheetah_rpy  -1 output
aba_jvp        V+Q four_bar          -1 out_out
aba_jvp        V+Q mini_cheetah_rpy  -1 out_out
integrate_jvp  S+T tree65_fixed      -1 null
integrate_jvp  S+O tree65_fixed      -1 null
integrate_jvp  S+D tree65_fixed      -1 null
integrate_jvp  S+V tree65_fixed      -1 null
integrate_jvp  S+P four_bar          -1 null
integrate_jvp  S+P mini_cheetah_rpy  -1 null
integrate_jvp  T+O tree65_fixed      -1 tangent
integrate_jvp  T+D tree65_fixed      -1 tangent
integrate_jvp  T+V tree65_fixed      -1 tangent
integrate_jvp  T+P four_bar          -1 tangent
integrate_jvp  T+P mini_cheetah_rpy  -1 tangent
integrate_jvp  O+D tree65_fixed      -1 output
integrate_jvp  O+P four_bar          -1 output
integrate_jvp  O+P mini_cheetah_rpy  -1 output
integrate_jvp  D+V tree65_fixed      -1 dt
integrate_jvp  D+P four_bar          -1 dt
integrate_jvp  D+P mini_cheetah_rpy  -1 dt
integrate_jvp  V+P four_bar          -1 out_out
integrate_jvp  V+P mini_cheetah_rpy  -1 out_out
step_jvp       S+T tree65_fixed      -1 null
step_jvp       S+O tree65_fixed      -1 null
step_jvp       S+D tree65_fixed      -1 null
step_jvp       S+V tree65_fixed      -1 null
step_jvp       S+P four_bar          -1 null
step_jvp       S+P mini_cheetah_rpy  -1 null
step_jvp       S+Q tree65_fixed      -1 null
step_jvp       T+O tree65_fixed      -1 tangent
step_jvp       T+D tree65_fixed      -1 tangent
step_jvp       T+V tree65_fixed      -1 tangent
step_jvp       T+P four_bar          -1 tangent
step_jvp       T+P mini_cheetah_rpy  -1 tangent
step_jvp       T+Q tree65_fixed      -1 tangent
step_jvp       O+D tree65_fixed      -1 output
step_jvp       O+P four_bar          -1 output
step_jvp       O+P mini_cheetah_rpy  -1 output
step_jvp       O+Q tree65_fixed      -1 output
step_jvp       D+V tree65_fixed      -1 dt
step_jvp       D+P four_bar          -1 dt
step_jvp       D+P mini_cheetah_rpy  -1 dt
step_jvp       D+Q tree65_fixed      -1 dt
step_jvp       V+P four_bar          -1 out_out
step_jvp       V+P mini_cheetah_rpy  -1 out_out
step_jvp       V+Q tree65_fixed      -1 out_out
step_jvp       P+Q four_bar          -2 implicit
step_jvp       P+Q mini_cheetah_rpy  -2 rpy
"""
ROWS = [tuple(line.split()) for line in EXPECTED.strip().splitlines()]


def test_the_table_covers_every_pair_of_every_entry_point():
    assert len(ENTRY_POINTS) == 24 and all(hasattr(G.lib(), name) for name in ENTRY_POINTS)
    assert [(g, c, m) for g, c, m, _, _ in ROWS] == [(g, c, m) for g in GROUPS for c, m in cases_of(g)]
    assert all(int(code) in (-1, -2) for _, _, _, code, _ in ROWS)  # (every call is refused: none reaches a device with these buffers)
    named = {"S+O", "T+D", "D+V", "V+P", "P+Q"}  # the pairs the order was argued from
    for group in GROUPS:
        have = {c for g, c, _, _, _ in ROWS if g == group}
        assert {c for c in named if set(c.split("+")) <= set(rules_of(group))} <= have, group
    assert rules_of("step_vjp") == rules_of("step_jvp") == "STODVPQ" and rules_of("rnea_vjp") == "SOVQ" and rules_of("integrate_jvp") == "STODVP"


def test_the_plan_and_the_step_meet_on_a_plan_off_the_analytic_route():
    """P+Q needs a plan that the step refuses AND that would need the step: four_bar is one (the dynamics products, which take it, refuse
    a zero step on it, as on tree65_fixed).  mini_cheetah_rpy is on the analytic route: a zero step breaks no rule there, so that call
    is not made -- every call of this file is one the rules refuse."""
    assert ("step_vjp", "P+Q", "four_bar") in {(g, c, m) for g, c, m, _, _ in ROWS}
    for variant in GROUPS["aba_jvp"][0]:
        assert outcome("aba_jvp", variant, "Q", "four_bar") == (-1, MESSAGES["step"])
        assert outcome("aba_jvp", variant, "Q", "tree65_fixed") == (-1, MESSAGES["step"])


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_the_rule_that_wins(entry):
    group, variant = next((g, v) for g, spec in GROUPS.items() for v in spec[0] if entry == f"grbda_{g}_{v}")
    rows = [r for r in ROWS if r[0] == group]
    assert rows
    for _, case, model, code, message in rows:
        assert outcome(group, variant, case, model) == (int(code), MESSAGES[message]), (entry, case, model)
