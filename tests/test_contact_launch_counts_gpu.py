"""The launch sequence of the contact, kinematics and time-stepping entry points, per route: kernel and memset node counts of ONE captured
call (the shape of test_deriv_launch_counts_gpu.py).

Rows at B = 70 (a tile and a half), uncapped, so one chunk: applyTestForce, the inverse OSIM with and without J, contact points asking for
pos / pos + vel / pos + vel + acc, contact dynamics on the four feet of the Mini Cheetah, body poses and twists, step, and rollout over
three steps; the OSIM, test-force and contact-dynamics rows again under GRBDA_NO_EFPA=1 (the unit-wrench route of choose_osim, capi.cpp);
contact dynamics on tello_with_arms (differential clusters on the contacts' paths); contact points and twists on the depth-10 parallel
chains (big clusters: the spanning rates come from the manifold kernel); integrate on the four-bar (implicit clusters: LDS slots in use).

Rows in chunks, pinning what is launched and cleared per chunk.  Chunks of the budgeted pipelines are whole tiles of 64 states, so 70
states never make three chunks: contact dynamics runs 134 states under the work-slab cap of test_chunk_seams_gpu.py (64 + 64 + 6; the
fp32 force-propagation row fits 128 to a chunk and makes two).  The stand-alone inverse OSIM on the unit-wrench route takes fixed chunks
of 256 MiB whatever the cap: its row runs two such chunks and a ragged third.

EXPECTED was measured on the PARENT of the commit that gave the inverse OSIM one route record and the contact stages one launch site
each (its library built apart and selected with GRBDA_HIP_LIB), never on the code under test: the counts are integers, the margin is
zero.  The parent refuses none of the rows; a refusal would be pinned by its GrbdaError code."""
import pytest

import contact_ref as C
import generalized_rbda_amd as G
from entry_points import ENTRY, _inputs, _model, _osim_frames
from graph_capture import capture
from test_chunk_seams_gpu import CAP_MB

pytestmark = pytest.mark.gpu
B = 70
B_CAPPED = 134
DT = 1e-3
NO_EFPA = {"GRBDA_NO_EFPA": "1"}


def _points(want):
    def call(p, x):
        from test_contact_gpu import points_of

        bodies, offsets = points_of(x["model"])
        return p.contact_points(x["q"], bodies, offsets, qd=x["qd"] if "vel" in want else None, ydd=x["tau"] if "acc" in want else None)
    return call


def _dynamics(key):
    return lambda p, x: p.contact_dynamics(x["q"], x["qd"], x["tau"], *C.contact_set(key)[1:])


CALLS = {
    "apply_test_force": ENTRY["apply_test_force"][0],
    "inv_osim_J": ENTRY["inv_osim"][0],
    "inv_osim": lambda p, x: (p.inv_osim(x["q"], *_osim_frames(p.blob)),),
    "points_pos": _points(("pos",)),
    "points_pos_vel": _points(("pos", "vel")),
    "points_pos_vel_acc": _points(("pos", "vel", "acc")),
    "dynamics_feet": _dynamics("cheetah_feet"),
    "dynamics_tello": _dynamics("tello_feet"),
    "body_poses": ENTRY["body_poses"][0],
    "body_twists": ENTRY["body_twists"][0],
    "integrate": lambda p, x: p.integrate(x["q"], x["qd"], x["tau"], DT),
    "step": lambda p, x: p.step(x["q"], x["qd"], x["tau"], DT),
    "rollout3": lambda p, x: p.rollout(x["q"], x["qd"], x["tau"], DT, 3),
}
CHEETAH = "urdf_mini_cheetah"
# (id, model, plan-time switches, entry, batch -- "fixed": three fixed chunks of the unit-wrench inverse OSIM --, work-slab cap)
ROWS = [(e, CHEETAH, {}, e, B, False) for e in ("apply_test_force", "inv_osim_J", "inv_osim", "points_pos", "points_pos_vel", "points_pos_vel_acc",
                                                "dynamics_feet", "body_poses", "body_twists", "step", "rollout3")]
ROWS += [(e + "-no_efpa", CHEETAH, NO_EFPA, e, B, False) for e in ("apply_test_force", "inv_osim_J", "inv_osim", "dynamics_feet")]
ROWS += [("dynamics_tello", "tello_with_arms", {}, "dynamics_tello", B, False),
         ("points_pos_vel_acc-big_clusters", "parallel_chain_exp_d10_l16", {}, "points_pos_vel_acc", B, False),
         ("body_twists-big_clusters", "parallel_chain_exp_d10_l16", {}, "body_twists", B, False),
         ("integrate-four_bar", "urdf_four_bar", {}, "integrate", B, False),
         ("dynamics_feet-capped", CHEETAH, {}, "dynamics_feet", B_CAPPED, True),
         ("dynamics_feet-no_efpa-capped", CHEETAH, NO_EFPA, "dynamics_feet", B_CAPPED, True),
         ("inv_osim_J-no_efpa-three_chunks", CHEETAH, NO_EFPA, "inv_osim_J", "fixed", True)]
ROWS = [(f"{r[0]}-{dt}",) + r[1:] + (dt,) for r in ROWS for dt in ("f64", "f32")]

# id -> (kernel nodes, memset nodes) of the captured call, measured on the parent
EXPECTED = {
    "apply_test_force": (1, 1), "inv_osim_J": (1, 1), "inv_osim": (1, 1),
    "points_pos": (2, 0), "points_pos_vel": (4, 1), "points_pos_vel_acc": (4, 0),
    "dynamics_feet": (7, 1), "body_poses": (1, 0), "body_twists": (2, 0), "step": (3, 0), "rollout3": (8, 0),
    "apply_test_force-no_efpa": (7, 1), "inv_osim_J-no_efpa": (5, 1), "inv_osim-no_efpa": (5, 1), "dynamics_feet-no_efpa": (11, 1),
    "dynamics_tello": (7, 1), "points_pos_vel_acc-big_clusters": (4, 0), "body_twists-big_clusters": (2, 0), "integrate-four_bar": (2, 0),
    "dynamics_feet-capped": (21, 3), "dynamics_feet-no_efpa-capped": (33, 3), "inv_osim_J-no_efpa-three_chunks": (15, 3),
}
EXPECTED = {f"{k}-{dt}": v for k, v in EXPECTED.items() for dt in ("f64", "f32")}
EXPECTED["dynamics_feet-capped-f32"] = (14, 2)  # (128 states fit the cap in fp32: two chunks)


def _three_fixed_chunks(plan, itemsize):
    """two chunks of the 256 MiB the unit-wrench inverse OSIM takes for the two frames of entry_points.py, and a ragged third"""
    rows = 6 * len(_osim_frames(plan.blob)[0]) + 1
    per_state = plan.n_bodies * 12 + rows * (plan.nq + plan.n_bodies * 6 + 3 * plan.nv)
    return 2 * ((256 << 20) // (per_state * itemsize)) + 45


def measure(row, gpu, monkeypatch):
    """(kernel nodes, memset nodes) of one captured call of the row, or the error code of its refusal"""
    import torch

    _, model, env, entry, batch, capped, dtype_name = row
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if capped:
        monkeypatch.setenv("GRBDA_WORK_MAX_MB", str(CAP_MB))
    blob = _model(model)
    plan = G.Plan(blob)
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    n = _three_fixed_chunks(plan, dtype.itemsize) if batch == "fixed" else batch
    _, x = _inputs(blob, plan, n, 1, dtype, gpu)
    x["model"] = model
    try:
        cap = capture(lambda: CALLS[entry](plan, x))
    except G.GrbdaError as err:
        torch.cuda.synchronize()
        return err.code
    nodes = cap.nodes
    cap.drop()
    plan.release_work()
    return (nodes["kernel"], nodes["memset"])


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_launch_counts_of_one_captured_call(row, gpu, monkeypatch):
    got = measure(row, gpu, monkeypatch)
    print(f"COUNT {row[0]}: {got} (parent: {EXPECTED.get(row[0])})")
    assert got == EXPECTED[row[0]]
