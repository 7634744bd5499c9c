"""Models, states and references of the inverse-dynamics derivative tests (a helper module, not a test file): shared by
test_id_derivatives_cpu.py, which pins the references on the CPU, and test_id_derivatives_gpu.py, which holds grbda_rnea_derivatives_*
against them.

References at (q, qd, ydd), all from the CPU oracle's inverse dynamics:
    dydd  the mass matrix (entry_points._mass_oracle: unit-acceleration columns, exact)
    dqd   central differences with unit step (exact: the inverse dynamics are quadratic in qd)
    dq    central differences, h = 1e-6, along deriv_recursion_numpy.plus (the reference's tangent step; implicit clusters: an
          independent position moves and the oracle's Newton projection puts the dependent ones back)
and, for models of explicit clusters, the numpy statement of the analytic recursion (deriv_recursion_numpy.rnea_derivs).
Every model has one draw of B_MAX states; the batch sizes of the GPU test are its first rows."""
import functools

import numpy as np

import oracle_py as O
from deriv_recursion_numpy import parse, plus, rnea_derivs
from entry_points import _mass_oracle, _zoo
from models import random_cluster_tree, valid_states

B_MAX = 70
H_STEP = 1e-6
# batch sizes: no full group of four states; the tail alone; one group; a group and a tail state; a tile and a half (17 groups, a
# tail of 2, lanes past the end in the second tile)
BATCHES = (1, 3, 4, 5, 70)


def _tree(nv, floating, seed):
    return lambda: random_cluster_tree(seed, nv - 6 if floating else nv, floating=floating, kinds=("rev", "rotor")).serialize()


# name -> (blob maker, plan-time switches, the plan takes the analytic route)
# the interleaved / state-major rule of the run unpack (unpack_runs_interleave: a group's block of LDS <= 32 KiB) flips between
# nv = 31 and 32 in fp64 and between 44 and 45 in fp32
MODELS = {
    "mini_cheetah": (lambda: _zoo()["urdf_mini_cheetah"], (), True),
    "mini_cheetah_rpy": (lambda: _zoo()["urdf_mini_cheetah_rpy"], (), True),
    "pair_rotor_chain_4": (lambda: _zoo()["rev_pair_rotor_chain_4"], (), True),
    "tree16_fixed": (_tree(16, False, 516), (), True),
    "tree64_floating": (_tree(64, True, 564), (), True),
    "tree65_fixed": (_tree(65, False, 565), (), False),
    "tree31_fixed": (_tree(31, False, 531), (), True),
    "tree32_floating": (_tree(32, True, 532), (), True),
    "tree44_floating": (_tree(44, True, 544), (), True),
    "tree45_fixed": (_tree(45, False, 545), (), True),
    "four_bar": (lambda: _zoo()["urdf_four_bar"], (), False),
    "mini_cheetah_no_analytic": (lambda: _zoo()["urdf_mini_cheetah"], (("GRBDA_NO_ANALYTIC", "1"),), False),
}
RANDOM_TREES = [k for k in MODELS if k.startswith("tree")]


@functools.lru_cache(maxsize=None)
def blob_of(name):
    return MODELS[name][0]()


def is_explicit(blob):
    return all(c[9] in (0, 1) for c in parse(blob)["clusters"])


def _round(a, dt):
    return a if dt == "f64" else a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def states_of(name, dt="f64"):
    """B_MAX states {"q", "qd", "ydd"}, rounded to the type (implicit models: on the constraint manifold, cond(K_d) < 100 -- the
    bound entry_points.draw_bound gives the tests that differentiate along re-projected states)"""
    blob = blob_of(name)
    q, qd, ydd = valid_states(blob, B_MAX, config_index=77, max_cond=None if is_explicit(blob) else 100.0)
    # (q_start: run_guarded places a projection input for every call)
    return {"q": _round(q, dt), "qd": _round(qd, dt), "ydd": _round(ydd, dt), "q_start": _round(q, dt)}


def plus_on_manifold(blob, m, q, k, d):
    """q after the tangent step d along velocity coordinate k; a coordinate of an implicit cluster moves its k-th INDEPENDENT
    position and the dependent ones are re-projected onto phi(q) = 0"""
    for c in m["clusters"]:
        qi, vi, nvel, nsv, ctype, io = c[3], c[5], c[6], c[8], c[9], c[11]
        if ctype in (2, 3) and vi <= k < vi + nvel:
            flags = m["ints"][io + 1: io + 1 + nsv] if ctype == 2 else m["ints"][io: io + nsv]
            ind = [j for j in range(nsv) if flags[j]]
            out = q.copy()
            out[qi + ind[k - vi]] += d
            qp, ok = O.project_positions(blob, out[None])
            assert ok[0]
            return qp[0]
    e = np.zeros(m["nv"])
    e[k] = d
    return plus(m, q, e)


def oracle_dqd(blob, q, qd, ydd):
    B, nv = qd.shape
    out = np.empty((B, nv, nv))
    for k in range(nv):
        e = np.zeros((B, nv))
        e[:, k] = 1.0
        out[:, :, k] = (O.inverse_dynamics(blob, q, qd + e, ydd) - O.inverse_dynamics(blob, q, qd - e, ydd)) / 2
    return out


def oracle_dq(blob, q, qd, ydd, h=H_STEP):
    m = parse(blob)
    B, nv = qd.shape
    out = np.empty((B, nv, nv))
    for k in range(nv):
        qp = np.stack([plus_on_manifold(blob, m, q[b], k, +h) for b in range(B)])
        qm = np.stack([plus_on_manifold(blob, m, q[b], k, -h) for b in range(B)])
        out[:, :, k] = (O.inverse_dynamics(blob, qp, qd, ydd) - O.inverse_dynamics(blob, qm, qd, ydd)) / (2 * h)
    return out


def oracle_refs(blob, s):
    return {"dydd": _mass_oracle(blob, s["q"]), "dqd": oracle_dqd(blob, s["q"], s["qd"], s["ydd"]), "dq": oracle_dq(blob, s["q"], s["qd"], s["ydd"])}


@functools.lru_cache(maxsize=None)
def refs_of(name):
    """the oracle references of the model's B_MAX fp64 states; shared, never written to"""
    return oracle_refs(blob_of(name), states_of(name))


def recursion_refs(blob, s, idx):
    """(dq, dqd) of the numpy recursion on the states idx of s"""
    m = parse(blob)
    got = [rnea_derivs(m, s["q"][b], s["qd"][b], s["ydd"][b]) for b in idx]
    return np.stack([g[1] for g in got]), np.stack([g[2] for g in got])


@functools.lru_cache(maxsize=None)
def _recursion_state(name, b):
    return rnea_derivs(parse(blob_of(name)), *(states_of(name)[k][b] for k in ("q", "qd", "ydd")))[1:]


def recursion_refs_of(name, idx):
    """(dq, dqd) of the numpy recursion on the states idx of the model's fp64 draw; each state is evaluated once"""
    got = [_recursion_state(name, int(b)) for b in idx]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def related_mask(blob):
    """[nv, nv] bool: coordinates i and j lie on one root path (same cluster, or one cluster an ancestor of the other) -- from the
    bodies' parent table of the description, not from the library"""
    m = parse(blob)
    nc, nv = m["nc"], m["nv"]
    anc = [{c} for c in range(nc)]
    for b in m["bodies"]:
        p = b["parent"]
        while p >= 0:
            anc[b["cluster"]].add(m["bodies"][p]["cluster"])
            p = m["bodies"][p]["parent"]
    owner = np.empty(nv, dtype=int)
    for c, cl in enumerate(m["clusters"]):
        owner[cl[5]: cl[5] + cl[6]] = c
    return np.array([[owner[i] in anc[owner[j]] or owner[j] in anc[owner[i]] for j in range(nv)] for i in range(nv)])
