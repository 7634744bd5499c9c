"""The term-by-term checker of term_states.py has teeth (no GPU): defective outputs synthesised from the fp64 oracle -- one term wrong by
1 %, one gravity component dropped -- are rejected by within_float on the set that isolates the term, the oracle's own output rounded to
fp32 is accepted, and the metric of the other fp32 tests (rel_err < TOL32 on states with random torques) accepts the same defect: the gap
these sets close."""
import numpy as np
import pytest

import oracle_py as O
import term_states as TS
from term_states import OBLIQUE, fp32_rounded, model_blob, passes_float, references, term_set, with_gravity

TOL32 = 1e-3
MODELS = ("urdf_mini_cheetah", "urdf_mit_humanoid", "urdf_jvrc1_humanoid", "tello_with_arms", "urdf_six_bar", "tree_triple_fixed")
FN = {"aba": O.forward_dynamics, "rnea": O.inverse_dynamics}


def velocity_defect(blob, name, which, scale=0.99):
    """the velocity-product part of set `name` scaled: f(q, 0, x) + scale (f(q, qd, x) - f(q, 0, x)), rounded to fp32"""
    g, q, qd, x = term_set(blob, name)
    still = FN[which](g, q, np.zeros_like(qd), x)
    return fp32_rounded(still + scale * (FN[which](g, q, qd, x) - still))


def gravity_defect(blob, name, which, change):
    """set `name` evaluated at the gravity change(g), rounded to fp32"""
    g, q, qd, x = term_set(blob, name)
    import generalized_rbda_amd as G

    wrong = with_gravity(g, change(np.array(G.Plan(g).get_gravity())))
    return fp32_rounded(FN[which](wrong, q, qd, x))


def dropped_axis(name):
    """the oblique component that is dropped: z, and for the six-bar x -- z is perpendicular to its plane and moves nothing"""
    return 0 if name == "urdf_six_bar" else 2


def drop(axis):
    def change(g):
        g = g.copy()
        g[axis] = 0.0
        return g
    return change


@pytest.mark.parametrize("which", ["aba", "rnea"])
@pytest.mark.parametrize("name", MODELS)
def test_seeded_defects_are_rejected_and_the_oracle_is_accepted(name, which):
    blob = model_blob(name)
    for s in TS.sets_of(name, which):
        ref, fl = references(blob, s, which)
        assert passes_float(fp32_rounded(ref), ref, fl), f"{s}: the oracle rounded to fp32 is refused"
        TS.within_float(fp32_rounded(ref), ref, fl, what=s)
    ref, fl = references(blob, "V", which)
    assert not passes_float(velocity_defect(blob, "V", which), ref, fl), "velocity-product terms at 99 % pass on V"
    with pytest.raises(AssertionError):
        TS.within_float(velocity_defect(blob, "V", which), ref, fl)
    for s in ("G", "Gobl"):
        if (name, s) in TS.NOT_RUN:
            continue
        ref, fl = references(blob, s, which)
        assert not passes_float(gravity_defect(blob, s, which, lambda g: 0.99 * g), ref, fl), f"gravity at 99 % passes on {s}"
    ref, fl = references(blob, "Gobl", which)
    assert not passes_float(gravity_defect(blob, "Gobl", which, drop(dropped_axis(name))), ref, fl), "a dropped gravity component passes on Gobl"


def test_the_six_bar_does_not_feel_gravity_across_its_plane():
    """why dropped_axis picks x there"""
    blob = model_blob("urdf_six_bar")
    ref, _ = references(blob, "Gobl", "aba")
    g, q, qd, x = term_set(blob, "Gobl")
    assert np.array_equal(O.forward_dynamics(with_gravity(g, (OBLIQUE[0], OBLIQUE[1], 0.0)), q, qd, x), ref)


def test_the_norm_wise_metric_accepts_the_velocity_defect():
    """The gap on record: every velocity-product term of Mini Cheetah wrong by 1 % passes rel_err < TOL32 on the `all` set in more than
    half of the states (and a defect of 10 % still passes in most), while within_float refuses it on `all` itself and on V."""
    blob = model_blob("urdf_mini_cheetah")
    ref, fl = references(blob, "all", "aba")
    for scale, least in ((0.99, 0.5), (0.9, 0.5)):
        bad = velocity_defect(blob, "all", "aba", scale)
        per_state = np.abs(bad - ref).max(axis=1) / (1.0 + np.abs(ref).max(axis=1))
        assert (per_state < TOL32).mean() > least, (scale, (per_state < TOL32).mean())
    assert not passes_float(velocity_defect(blob, "all", "aba"), ref, fl)


def test_at_most_one_per_cent_of_a_batch_is_left_out():
    """of every (model, set, direction) test_term_parity_gpu.py runs; and what NOT_RUN lists would exceed the cap"""
    seen = set()
    for _, name, s, which in TS.gpu_cases():
        if (name, s, which) in seen:
            continue
        seen.add((name, s, which))
        ref, fl = references(model_blob(name), s, which)
        assert TS.left_out(ref) <= TS.MAX_LEFT_OUT, (name, s, which, TS.left_out(ref))
        assert TS.term_error(fl, ref).max() > 0
    for (name, s) in TS.NOT_RUN:
        if s == "all":
            continue
        g, q, qd, x = term_set(model_blob(name), s)
        assert TS.left_out(O.forward_dynamics(g, q, qd, x)) > TS.MAX_LEFT_OUT, (name, s)


def test_nothing_is_left_of_the_empty_set():
    """Z: zero gravity, velocity and third input give exactly zero in the oracle, on every model of the GPU file"""
    for name in sorted({m for _, models in TS.ROUTES.values() for m in models}):
        g, q, qd, x = term_set(model_blob(name), "Z")
        assert not O.forward_dynamics(g, q, qd, x).any() and not O.inverse_dynamics(g, q, qd, x).any(), name


def test_per_case_margins_still_refuse_the_seeded_defects():
    """A case of test_term_parity_gpu.MARGINS holds the kernel at more than 5 x the float oracle: its seeded 1 % defect must still fail at
    that margin."""
    from test_term_parity_gpu import MARGINS

    for (route, name, s, which), (margin, _ratio, _cause) in MARGINS.items():
        assert margin > TS.MARGIN and name in ROUTE_MODELS[route]
        blob = model_blob(name)
        w = "rnea" if which == "bias" else which
        ref, fl = references(blob, s, which)
        bad = []
        if s in ("V", "all"):
            bad.append(velocity_defect(blob, s, w))
        if s in ("G", "Gobl", "all"):
            bad.append(gravity_defect(blob, s, w, lambda g: 0.99 * g))
        if s == "T":
            bad.append(fp32_rounded(0.99 * ref))
        for b in bad:
            assert not passes_float(b, ref, fl, margin), (route, name, s, which, margin)


def test_spanning_tree_margins_still_refuse_the_seeded_defects():
    """test_gravity_gpu.SPANNING_TREE_MARGINS (two_parent's forward dynamics, up to 37.6 x the float oracle): on the states of that file,
    velocity-product terms or gravity wrong by 1 % fail at the margin."""
    import torch

    import entry_points as EP
    import test_gravity_gpu as TG

    for (model, entry, gname), (margin, _ratio) in TG.SPANNING_TREE_MARGINS.items():
        assert entry == "aba"
        blob = EP._model(model)
        g = TS.native_gravity(blob) if TG.GRAVITIES[gname] is None else TG.GRAVITIES[gname]
        gblob = with_gravity(blob, g)
        s = EP._host_inputs(blob, TS.G.Plan(blob).n_bodies, TG.B, TG.SEED, torch.float32)
        q, qd, x = s["q"], s["qd"], s["tau"]
        ref, fl = O.forward_dynamics(gblob, q, qd, x), O.forward_dynamics_f32(gblob, q, qd, x).astype(np.float64)
        still = O.forward_dynamics(gblob, q, np.zeros_like(qd), x)
        assert not passes_float(fp32_rounded(still + 0.99 * (ref - still)), ref, fl, margin), (gname, "velocity")
        if any(g):
            weak = O.forward_dynamics(with_gravity(blob, [0.99 * c for c in g]), q, qd, x)
            assert not passes_float(fp32_rounded(weak), ref, fl, margin), (gname, "gravity")


ROUTE_MODELS = {r: models for r, (_, models) in TS.ROUTES.items()}
