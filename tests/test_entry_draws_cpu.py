"""The conditions the entry-point table's draws must meet, asserted on the reference alone (no GPU): what a checker of entry_points.py
leaves out, or what would trip run_guarded's finiteness check, is a property of the draw and is decided here, not measured on the device.

Draws are taken per (model, seed, B, type).  The four GPU files use: graph capture seeds 1, 2, 3 at the row's B; buffer edges seed 11 at
the row's B and at 65; the batch ladder the first 1, 2, 63, 64, 65, 127, 128, 129, 257 rows of seed 21 at 257; the concurrent streams
seeds 100 + i at B - i.  (Graph capture also warms up with seed 4 at 2 B: nothing of that call is read.)

1. integrate / step on models with implicit clusters: integrate_ref.reference_step accepts at least 95 % of every draw (the share
   integrate_ref.py and test_integrate_cpu.py use), at the time step the row runs with.  Measured: 100 % of every draw of the four-bar at
   dt = 0.05, fp64 and fp32-rounded inputs alike, so no row's time step is halved (entry_points.DT_HALVED is empty).
2. contact_dynamics: the reference's lambda is finite for every state of every draw, and cond(A) of the rows run in fp32 stays below
   1e3 -- cond(A) eps32 = 6e-5 is then a sixteenth of TOL32; test_contact_gpu.py's own draws measure 2.4e2 on the same contact sets.
   Measured over the draws below: Mini Cheetah feet 4.25e2, Tello feet 1.78e2, eight damped sole corners (fp64 only) 9.63e3.
3. contact_impulse: qd_next and the impulse of impulse_ref are finite for every state of every draw, and cond(A) -- the matrix of the
   contact_dynamics rows on the same contact sets -- stays below 1e3 in fp32 by the same reasoning.  Measured: 4.25e2 and 1.78e2 again.
4. test_gravity_gpu.py runs the later rows on one more draw, seed 41 at B = 300, at four gravities: the four-bar's step keeps the 95 %
   of condition 1 at each of them (measured: 100 %), and the contact rows keep conditions 2 and 3 (gravity does not enter A; lambda is
   finite at every gravity; cond(A) on that draw: 2.90e2, 1.35e2, 9.55e3)."""
import numpy as np
import pytest

import contact_ref as C
import generalized_rbda_amd as G
import impulse_ref as I
import integrate_ref as R
import oracle_py as O
from entry_points import CASES, TYPED, _big, _contacts, _dt, _host_inputs, _model, DAMPING, RESTITUTION, draw_bound
from generalized_rbda_amd.states import parse_clusters

LADDER = (1, 2, 63, 64, 65, 127, 128, 129, 257)  # test_batch_ladder_gpu.TILES (asserted below)


def draws(B):
    """(seed, batch, prefixes held) of a row of batch B"""
    out = [(seed, B, (B,)) for seed in (1, 2, 3, 11)] + [(11, 65, (65,)), (21, LADDER[-1], LADDER)]
    return out + [(100 + i, B - i, (B - i,)) for i in range(4)]


def _dtype(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def _implicit(blob):
    return any(c[9] in (2, 3) for c in parse_clusters(blob)["clusters"])


STEPPING = [(c, dt) for c, dt in TYPED if c[4] in ("integrate", "step", "step_fext", "rollout") and _implicit(_model(c[1]))]
CONTACT = [(c, dt) for c, dt in TYPED if c[4].startswith("contact_dynamics") and not c[2]]  # (a plan-time switch does not change the draw)
IMPULSE = [(c, dt) for c, dt in TYPED if c[4] == "contact_impulse" and not c[2]]
GRAVITY_DRAW = (41, 300)  # test_gravity_gpu.SEED, B (asserted below)


def test_the_ladder_is_the_ladder():
    import test_batch_ladder_gpu as L

    assert tuple(L.TILES) == LADDER and L.SEED == 21
    import test_gravity_gpu as TG

    assert (TG.SEED, TG.B) == GRAVITY_DRAW


@pytest.mark.parametrize("case,dt", STEPPING, ids=[f"{c[4]}-{c[1]}-{dt}" for c, dt in STEPPING])
def test_the_reference_accepts_95_percent_of_every_stepped_draw(case, dt):
    route, model, env, B, entry = case
    blob = _model(model)
    nb = G.Plan(blob).n_bodies
    assert entry != "rollout", "a rollout row on an implicit model: hold every step's share here"
    for seed, n, prefixes in draws(B):
        s = _host_inputs(blob, nb, n, seed, _dtype(dt), draw_bound(entry))
        ydd = s["tau"] if entry == "integrate" else O.forward_dynamics(blob, s["q"], s["qd"], s["tau"], s["fext"] if entry == "step_fext" else None)
        ok = R.reference_step(blob, s["q"], s["qd"], ydd, _dt(blob), big=_big(blob))[2]
        for b in prefixes:
            print(f"{entry} {model} {dt} seed {seed} B {b} dt {_dt(blob)}: {ok[:b].mean():.3f} accepted")
            assert ok[:b].mean() >= 0.95, (seed, b, ok[:b].mean())


@pytest.mark.parametrize("case,dt", CONTACT, ids=[f"{c[4]}-{c[1]}-{dt}" for c, dt in CONTACT])
def test_the_contact_reference_is_finite_on_every_draw(case, dt):
    route, model, env, B, entry = case
    blob = _model(model)
    nb = G.Plan(blob).n_bodies
    damped = entry.endswith("damped_fext")
    worst = 0.0
    for seed, n, _ in draws(B):
        s = _host_inputs(blob, nb, n, seed, _dtype(dt))
        ref = C.contact_dynamics(blob, s["q"], s["qd"], s["tau"], *_contacts(blob), s["a_des"], DAMPING if damped else 0.0, s["fext"] if damped else None)
        assert all(np.isfinite(ref[k]).all() for k in ("ydd", "lam", "ydd_free")), (seed, n)
        worst = max(worst, float(np.linalg.cond(ref["A"]).max()))
    print(f"{entry} {model} {dt}: cond(A) at most {worst:.2e}")
    if dt == "f32":
        assert worst < 1e3, worst


@pytest.mark.parametrize("case,dt", IMPULSE, ids=[f"{c[4]}-{c[1]}-{dt}" for c, dt in IMPULSE])
def test_the_impulse_reference_is_finite_on_every_draw(case, dt):
    route, model, env, B, entry = case
    blob = _model(model)
    nb = G.Plan(blob).n_bodies
    worst = 0.0
    for seed, n, _ in draws(B) + [GRAVITY_DRAW + ((GRAVITY_DRAW[1],),)]:
        s = _host_inputs(blob, nb, n, seed, _dtype(dt))
        ref = I.contact_impulse(blob, s["q"], s["qd"], *_contacts(blob), s["v_des"], RESTITUTION, 0.0)
        assert np.isfinite(ref["qd_next"]).all() and np.isfinite(ref["impulse"]).all(), (seed, n)
        cond = float(np.linalg.cond(ref["A"]).max())
        print(f"{entry} {model} {dt} seed {seed} B {n}: cond(A) at most {cond:.2e}")
        worst = max(worst, cond)
    print(f"{entry} {model} {dt}: cond(A) at most {worst:.2e}")
    if dt == "f32":
        assert worst < 1e3, worst


def _gravity_blobs(model):
    """the description of `model` at the four gravities of test_gravity_gpu.py, under the model's name as that file registers them"""
    import test_gravity_gpu as TG
    import term_states as TS

    out = {}
    for gname, g in TG.GRAVITIES.items():
        out[gname] = _model(model) if g is None else TS.with_gravity(_model(model), g)
        TG.register(model, out[gname])
    return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_reference_accepts_95_percent_of_the_gravity_files_draw(dt):
    """the four-bar's step row of test_gravity_gpu.py, seed 41, at every gravity it runs"""
    model, entry = "urdf_four_bar", "step"
    seed, B = GRAVITY_DRAW
    nb = G.Plan(_model(model)).n_bodies
    s = _host_inputs(_model(model), nb, B, seed, _dtype(dt), draw_bound(entry))
    for gname, blob in _gravity_blobs(model).items():
        ydd = O.forward_dynamics(blob, s["q"], s["qd"], s["tau"])
        ok = R.reference_step(blob, s["q"], s["qd"], ydd, _dt(blob), big=_big(blob))[2]
        print(f"{entry} {model} {dt} seed {seed} B {B} dt {_dt(blob)} {gname}: {ok.mean():.3f} accepted")
        assert _dt(blob) == 0.05 and ok.mean() >= 0.95, (gname, ok.mean())


@pytest.mark.parametrize("case,dt", CONTACT, ids=[f"{c[4]}-{c[1]}-{dt}" for c, dt in CONTACT])
def test_the_contact_reference_is_finite_on_the_gravity_files_draw(case, dt):
    route, model, env, _, entry = case
    seed, B = GRAVITY_DRAW
    damped = entry.endswith("damped_fext")
    s = _host_inputs(_model(model), G.Plan(_model(model)).n_bodies, B, seed, _dtype(dt))
    for gname, blob in _gravity_blobs(model).items():
        ref = C.contact_dynamics(blob, s["q"], s["qd"], s["tau"], *_contacts(blob), s["a_des"], DAMPING if damped else 0.0, s["fext"] if damped else None)
        assert all(np.isfinite(ref[k]).all() for k in ("ydd", "lam", "ydd_free")), gname
        cond = float(np.linalg.cond(ref["A"]).max())
        print(f"{entry} {model} {dt} seed {seed} {gname}: cond(A) at most {cond:.2e}")
        if dt == "f32":
            assert cond < 1e3, cond


def test_every_contact_row_is_covered():
    """the rows left out above differ from a row held above by a plan-time switch only"""
    held = {(c[1], c[4], dt) for c, dt in CONTACT}
    assert all((c[1], c[4], dt) in held for c, dt in TYPED if c[4].startswith("contact_dynamics"))
    held = {(c[1], c[4], dt) for c, dt in IMPULSE}
    assert len(held) == 4 and all((c[1], c[4], dt) in held for c, dt in TYPED if c[4] == "contact_impulse")
    assert any(c[4] == "integrate" for c, _ in STEPPING) and any(c[4] == "step" for c, _ in STEPPING)
    assert len(CASES) > 0
