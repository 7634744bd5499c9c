"""Writes outside an output, output elements never written, inputs written to, and results that depend on the pointer's alignment.

Every row of the entry-point table (entry_points.py: entry point x route x model x switches -- the inverse-dynamics derivatives,
integrate / step / rollout, the contact entry points, energy, the centroidal quantities and the momentum matrix included), fp32 and fp64
(less entry_points.NOT_RUN), with every input and every
output inside a guarded buffer of guarded.py -- a view between two 4 KiB bands of a canary bit pattern, the view itself pre-filled with
it -- at the row's own batch size and at a ragged small one (B = 65: one full tile and one state; the chain rows' B_CHAIN is ragged as
it is, and needed for their route).  lead = 0 keeps the allocator's alignment, lead = 1 moves every pointer by one element (4 / 8 bytes),
which include/grbda_hip.h allows.  Asserted (run_guarded): both bands of every output intact, no output element left holding the
canary, every input bit-identical to its copy (bands included; project_positions' in-place q: bands and the columns it does not own),
outputs finite, the row's oracle checker at the table's tolerances on state 0, state B - 1, both ends of the last tile and a seeded few,
and lead = 1 bit-identical to lead = 0.  Forward / inverse dynamics also run with a caller-supplied out= arena.

The input bands are NaN: rows >= B that reach a live result show as a non-finite output.  An over-read that stays in dead lanes is
neither detected nor a defect (guarded.py)."""
import numpy as np
import pytest

import guarded  # noqa: F401  (the helper the runner uses)
from entry_points import B_CHAIN, CASES, ENTRY, IDS, TOL32, TOL64, TYPED, _body_index, _contacts, _host_inputs, _model, _rel, OFFSET, OSIM_BODIES, draw_bound, edge_states, plan_for, run_guarded, same_bits_np

pytestmark = pytest.mark.gpu
B_RAGGED = 65

# each row at its own size and at the ragged small one (a chain row's own size IS the ragged one: its route needs the large batch)
SIZED = [(c, b) for c in CASES for b in ((c[3],) if c[3] == B_CHAIN else (c[3], B_RAGGED))]
SIZED_IDS = [f"{ep}-{route}-{model}-B{b}" for (route, model, env, B, ep), b in SIZED]
assert {i.rsplit("-B", 1)[0] for i in SIZED_IDS} == {i.rsplit("-B", 1)[0] for i in IDS}  # every row of the table
# ... in both types, less what the table itself leaves out (entry_points.NOT_RUN)
SIZED_TYPED = [(c, b, dt) for c, b in SIZED for dt in ("f64", "f32") if (c, dt) in TYPED]
SIZED_TYPED_IDS = [f"{ep}-{route}-{model}-B{b}-{dt}" for (route, model, env, B, ep), b, dt in SIZED_TYPED]


def _dtype(name):
    import torch

    return torch.float64 if name == "f64" else torch.float32


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("case,B,dtype_name", SIZED_TYPED, ids=SIZED_TYPED_IDS)
def test_entry_point_keeps_to_its_buffers(case, B, dtype_name, lead, gpu):
    route, model, env, _, entry = case
    dtype, tol = _dtype(dtype_name), TOL64 if dtype_name == "f64" else TOL32
    blob, plan = _model(model), plan_for(model, tuple(sorted(env.items())))
    call, check = ENTRY[entry]
    s = _host_inputs(blob, plan.n_bodies, B, 11, dtype, draw_bound(entry))
    got = run_guarded(plan, call, s, dtype, gpu, lead, out_arena=entry if entry in ("aba", "rnea") else None)
    assert all(len(o) == B for o in got)
    if check is not None:
        idx = edge_states(B, seed=B)
        check(blob, {k: v[idx] for k, v in s.items()}, [o[idx] for o in got], tol)
    if lead:  # the same bits through pointers that keep the allocator's alignment
        assert same_bits_np(got, run_guarded(plan, call, s, dtype, gpu, 0)), "lead = 1 and lead = 0 differ"


# ---- optional outputs: only what was asked for is allocated, and all of it is written ------------------------------------------------
def _osim_linv_only(plan, x):
    return (plan.inv_osim(x["q"], [_body_index(plan.blob, b) for b in OSIM_BODIES], [OFFSET, (0.0, 0.0, 0.0)]),)


OPTIONAL = {  # name -> (model, switches, call, full entry point of the table, indices of its outputs this call returns)
    "inv_osim_linv_only": ("urdf_mini_cheetah", {}, _osim_linv_only, "inv_osim", (0,)),
    "inv_osim_linv_only_no_efpa": ("urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, _osim_linv_only, "inv_osim", (0,)),
    "fd_derivatives_dq_only": ("urdf_mini_cheetah", {}, lambda p, x: tuple(p.fd_derivatives(x["q"], x["qd"], x["tau"], want=("dq",)).values()),
                               "fd_derivatives", (0,)),
    "fd_derivatives_dqd_dtau": ("urdf_mini_cheetah", {}, lambda p, x: tuple(p.fd_derivatives(x["q"], x["qd"], x["tau"], want=("dqd", "dtau")).values()),
                                "fd_derivatives", (1, 2)),
    "fd_derivatives_dtau_manifold": ("tello", {}, lambda p, x: tuple(p.fd_derivatives(x["q"], x["qd"], x["tau"], want=("dtau",)).values()),
                                     "fd_derivatives", (2,)),
    "state_positions_only": ("urdf_four_bar", {}, lambda p, x: tuple(o for o in p.state_to_independent(x["q"], tol=1e-8 if x["q"].dtype.itemsize == 8 else 1e-3)
                                                                     if o is not None), "state_to_independent", (0, 2)),
    # (an output that is not asked for is not allocated: an arena made and left unwritten would fail run_guarded)
    "contact_points_positions_only": ("urdf_mini_cheetah", {}, lambda p, x: tuple(o for o in p.contact_points(x["q"], *_contacts(p.blob)) if o is not None),
                                      "contact_points", (0,)),
    "centroidal_hdot_only": ("urdf_mit_humanoid", {}, lambda p, x: tuple(p.centroidal(x["q"], x["qd"], x["tau"], want=("hdot",)).values()),
                             "centroidal", (3,)),
    "energy_without_qd": ("urdf_mit_humanoid", {}, lambda p, x: tuple(o for o in p.energy(x["q"]) if o is not None), "energy", (1,)),
}


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("B", [1000, B_RAGGED])
@pytest.mark.parametrize("name", list(OPTIONAL))
def test_optional_outputs(name, B, dtype_name, lead, gpu):
    """A call that asks for some of an entry point's outputs: the arenas made are exactly those, each complete and in bounds, and they
    agree with the same outputs of the full call (which the test above holds against the oracle) at the table's tolerance."""
    model, env, call, entry, which = OPTIONAL[name]
    dtype, tol = _dtype(dtype_name), TOL64 if dtype_name == "f64" else TOL32
    blob, plan = _model(model), plan_for(model, tuple(sorted(env.items())))
    s = _host_inputs(blob, plan.n_bodies, B, 11, dtype)
    got = run_guarded(plan, call, s, dtype, gpu, lead)
    full = run_guarded(plan, ENTRY[entry][0], s, dtype, gpu, lead)
    assert len(got) == len(which)
    for o, i in zip(got, which):
        assert o.shape == full[i].shape and _rel(o.astype(float), full[i].astype(float)) < tol


def test_state_to_independent_with_conditioning_output(gpu):
    """want_gmax: the fourth output, cond[B, 2], in its arena too (constraint_gain goes through it)"""
    import torch

    import oracle_py as O

    blob, plan = _model("urdf_four_bar"), plan_for("urdf_four_bar", ())
    for dtype in (torch.float64, torch.float32):
        for lead in (0, 1):
            s = _host_inputs(blob, plan.n_bodies, B_RAGGED, 11, dtype)
            q, qd, status, cond = run_guarded(plan, lambda p, x: p.state_to_independent(x["q"], x["qd"], tol=1e-8 if dtype == torch.float64 else 1e-3,
                                                                                         want_gmax=True), s, dtype, gpu, lead)
            gmax, kcond = O.spanning_state(blob, s["q"], s["qd"])[2:]
            assert (status == 0).all() and cond.shape == (B_RAGGED, 2)
            if dtype == torch.float64:  # (the bounds of test_state_input_gpu.py)
                assert np.abs(cond[:, 0] - gmax).max() <= 1e-8 * (1 + gmax.max()) and (np.abs(cond[:, 1] - kcond) / kcond).max() <= 1e-7
            else:
                assert _rel(cond[:, 0], gmax) < TOL32 and _rel(cond[:, 1], kcond) < TOL32
