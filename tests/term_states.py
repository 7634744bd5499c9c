"""Term-by-term states and the single-precision yardstick.  A plain module, not a test file: test_term_checker_cpu.py (no GPU: the checker
has teeth), test_term_parity_gpu.py and test_gravity_gpu.py go through it.

The suite's fp32 metric, max|got - ref| / (1 + |ref|_inf) < 1e-3 on states with random torques, sees H^-1 tau and little else: the
velocity-product terms are about 1 % of such a result and gravity less.  Here one draw (q, qd, x) of a model is taken apart into SETS that
leave one term standing each, the error is measured on that term's own scale (term_error), and the bound is what single precision itself
costs on the same inputs: the oracle compiled in `float` (oracle_py.forward_dynamics_f32), times a margin (within_float)."""
import functools
import os

import numpy as np

import oracle_py as O
import generalized_rbda_amd as G
from models import valid_states, zoo

OBLIQUE = (3.1, -4.7, -6.9)  # no component zero, none equal: a dropped, swapped or sign-flipped axis shows
SETS = ("V", "G", "Gobl", "T", "Z", "all")
# set: (gravity, qd drawn, third input drawn) -- what is left of the equations of motion
_SET = {
    "V": ("zero", True, False),       # velocity-product terms only
    "G": ("native", False, False),    # gravity only
    "Gobl": ("oblique", False, False),  # oblique gravity only
    "T": ("zero", False, True),       # H^-1 tau (forward), H ydd (inverse)
    "Z": ("zero", False, False),      # nothing
    "all": ("native", True, True),    # the states of the other tests
}
MAX_LEFT_OUT = 0.01  # of a batch
FLOOR = 1e-3         # of the batch median of |ref|_inf
MARGIN = 5.0         # the project's margin for this yardstick (test_fp32_joint_angles_of_a_hundred_radians)
B_TERMS = 500
SEED = 22

# (model, set) that are not run, with the reason (measured on the CPU with the oracle; every other (model, set, direction) of ROUTES leaves
# out at most 0.2 % of its batch)
NOT_RUN = {
    ("urdf_four_bar", "G"): "gravity along z is perpendicular to the linkage's plane: the gravity term is identically zero (Gobl is run)",
    ("urdf_six_bar", "G"): "gravity along z is perpendicular to the linkage's plane: the gravity term is identically zero (Gobl is run)",
    ("urdf_planar_leg_linkage", "G"): "gravity along z is perpendicular to the linkage's plane: the gravity term is identically zero (Gobl is run)",
    ("urdf_four_bar", "V"): "a parallelogram: H is constant and the velocity-product term is 1e-17 in the oracle (six-bar and planar leg linkage run V)",
    ("urdf_four_bar", "all"): "with V and G empty, `all` on the four-bar is T again",
}

# route: (plan-time switches, models) -- the fp32 paths of the library
ROUTES = {
    "chain": ({"GRBDA_NO_LATENCY_MODE": "1"}, ("urdf_mini_cheetah", "urdf_mit_humanoid", "urdf_jvrc1_humanoid", "tello_with_arms", "tree_mixed_float",
                                               "tree_triple_fixed", "rev_rotor_chain_4", "chain_tree_b")),
    "lm4": ({}, ("urdf_mini_cheetah", "urdf_mit_humanoid", "tello_with_arms")),
    "lm2": ({"GRBDA_LM_WAVES": "2"}, ("urdf_mini_cheetah", "urdf_mit_humanoid", "tello_with_arms")),
    "interpreter": ({"GRBDA_NO_CHAIN": "1"}, ("urdf_mit_humanoid", "tree_mixed_float")),
    "gen1": ({}, ("urdf_six_bar", "urdf_planar_leg_linkage", "urdf_four_bar")),
}
COMPONENT_MODELS = ("urdf_mini_cheetah", "urdf_mit_humanoid", "urdf_jvrc1_humanoid", "tello_with_arms", "urdf_six_bar", "rev_rotor_chain_4")


def sets_of(model, which):
    """the non-empty sets `model` runs for `which` ("aba", "rnea", "bias"; the bias has no third input)"""
    sets = ("V", "G", "Gobl") if which == "bias" else ("V", "G", "Gobl", "T", "all")
    return tuple(s for s in sets if (model, s) not in NOT_RUN)


def gpu_cases():
    """(route, model, set, which) of every fp32 / fp64 term comparison of test_term_parity_gpu.py"""
    return [(r, m, s, w) for r, (_, models) in ROUTES.items() for m in models for w in ("aba", "rnea", "bias") for s in sets_of(m, w)]


model_blob = functools.lru_cache(maxsize=None)(lambda name: zoo()[name])


def with_gravity(blob, g):
    """the description `blob` at gravity g, through a plan of its own (plans of entry_points.plan_for are shared: never set_gravity on them)"""
    plan = G.Plan(blob)
    plan.set_gravity(g)
    out = bytes(plan.blob)
    assert G.Plan(out).get_gravity() == [float(x) for x in g]
    return out


def native_gravity(blob):
    return tuple(G.Plan(blob).get_gravity())


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def fp32_rounded(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _draw(blob, B, seed):
    return tuple(_frozen(fp32_rounded(a)) for a in valid_states(blob, B, config_index=seed))


@functools.lru_cache(maxsize=None)
def _blob_at(blob, gravity):
    g = {"zero": (0.0, 0.0, 0.0), "oblique": OBLIQUE, "native": native_gravity(blob)}[gravity]
    return with_gravity(blob, g)


def term_set(blob, name, B=B_TERMS, seed=SEED):
    """(blob at the set's gravity, q, qd, x): fp64 arrays of fp32-representable values, shared and read-only"""
    gravity, keep_qd, keep_x = _SET[name]
    q, qd, x = _draw(blob, B, seed)
    zero = _frozen(np.zeros_like(qd))
    return _blob_at(blob, gravity), q, qd if keep_qd else zero, x if keep_x else zero


_ORACLE = {"aba": (O.forward_dynamics, O.forward_dynamics_f32), "rnea": (O.inverse_dynamics, O.inverse_dynamics_f32),
           "bias": (O.inverse_dynamics, O.inverse_dynamics_f32)}


@functools.lru_cache(maxsize=None)
def references(blob, name, which, B=B_TERMS, seed=SEED):
    """(fp64 oracle, float oracle as fp64) of set `name`: computed once per process, shared, read-only"""
    gblob, q, qd, x = term_set(blob, name, B, seed)
    if which == "bias":
        x = np.zeros_like(x)
    f64, f32 = _ORACLE[which]
    return _frozen(f64(gblob, q, qd, x)), _frozen(f32(gblob, q, qd, x).astype(np.float64))


def kept(ref):
    """the states of a batch whose term is not degenerate: |ref|_inf at least FLOOR x the batch median"""
    scale = np.abs(ref).max(axis=1)
    return (scale > 0) & (scale >= FLOOR * np.median(scale))


def left_out(ref):
    return 1.0 - float(kept(ref).mean())


def term_error(got, ref):
    """per state, on the term's own scale: |got - ref|_inf / |ref|_inf (no `1 +`), of the states kept(ref)"""
    keep = kept(ref)
    assert 1.0 - keep.mean() <= MAX_LEFT_OUT, f"{(~keep).sum()} of {len(keep)} states have no term to measure: list the case in NOT_RUN"
    return np.abs(got - ref)[keep].max(axis=1) / np.abs(ref)[keep].max(axis=1)


def float_ratio(got32, ref64, float32_oracle_out):
    """(worst, median) term_error of got32 over that of the float oracle"""
    e, f = term_error(got32, ref64), term_error(float32_oracle_out, ref64)
    return float(e.max() / f.max()), float(np.median(e) / np.median(f))


def passes_float(got32, ref64, float32_oracle_out, margin=MARGIN):
    e, f = term_error(got32, ref64), term_error(float32_oracle_out, ref64)
    return bool(e.max() <= margin * f.max() and np.median(e) <= margin * np.median(f))


def within_float(got32, ref64, float32_oracle_out, margin=MARGIN, what=""):
    e, f = term_error(got32, ref64), term_error(float32_oracle_out, ref64)
    assert e.max() <= margin * f.max(), f"{what}: worst term error {e.max():.2e} against {f.max():.2e} of the float oracle ({e.max() / f.max():.1f} x, margin {margin})"
    assert np.median(e) <= margin * np.median(f), f"{what}: median term error {np.median(e):.2e} against {np.median(f):.2e} of the float oracle ({np.median(e) / np.median(f):.1f} x, margin {margin})"


def component_error(got, ref):
    """the worst of |got_i - ref_i| / (|ref_i| + 1e-3 |ref|_inf) (test_componentwise_parity_fp64's measure)"""
    return float((np.abs(got - ref) / (np.abs(ref) + 1e-3 * np.abs(ref).max(axis=1, keepdims=True))).max())


def compile_under(blob, env):
    """a plan of its own, compiled under the plan-time switches `env` (a dict); the environment is put back (entry_points.plan_for without
    the cache: the caller may set_gravity on it)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return G.Plan(blob)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
