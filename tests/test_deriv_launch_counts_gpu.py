"""The launch sequence of the derivative entry points, per route: kernel and memset node counts of ONE captured call.

Every row is (model, plan-time switches, dtype, entry point) at B = 70: a tile and a half, and no multiple of kDerivGroup = 4, so the
interleaved layouts take their state-major tail and an interleaved H leaves the caller's d/dtau array for the workspace.  No cap on the
work slabs: every call is one chunk.  The rows cover what choose_derivs (capi.cpp) can answer -- H^-1 from the articulated-body
quantities, the dense factorisation (plain, and fp32 widened to fp64), the manifold route (structured clusters; big clusters: d/dtau
alone, the rest difference batches), difference batches alone -- the three mass-matrix routes, the inverse-dynamics derivatives, and
forward dynamics through the spanning tree (projection_run).

EXPECTED was measured on the PARENT of the commit that gave the derivative entry points one route record and one launch site per
stage (its library built apart and selected with GRBDA_HIP_LIB), never on the code under test: a refactor of the host side has to
reproduce these counts exactly -- they are integers, the margin is zero.  A row that changes on purpose is measured the same way.
graph_capture.py gives the capture helper and the lifetime rules: the graph is dropped before release_work."""
import pytest

import generalized_rbda_amd as G
from entry_points import ENTRY, _inputs, _model
from graph_capture import capture

pytestmark = pytest.mark.gpu
B = 70

ENTRY_HERE = dict(ENTRY)
ENTRY_HERE["rnea_derivatives"] = (lambda p, x: tuple(p.id_derivatives(x["q"], x["qd"], x["tau"]).values()), None)
ENTRY_HERE["forward_dynamics"] = ENTRY["aba"]

# (id, model, plan-time switches, dtype, entry point)
ROWS = [
    ("minv-f32", "urdf_mini_cheetah", {}, "f32", "fd_derivatives"),
    ("minv-f64", "urdf_mini_cheetah", {}, "f64", "fd_derivatives"),
    ("factor-f32", "urdf_mini_cheetah", {"GRBDA_NO_MINV": "1"}, "f32", "fd_derivatives"),
    ("factor-f64", "urdf_mini_cheetah", {"GRBDA_NO_MINV": "1"}, "f64", "fd_derivatives"),
    ("factor-widened-f32", "urdf_mini_cheetah", {"GRBDA_SOLVE_F64": "1"}, "f32", "fd_derivatives"),
    ("differences-f64", "urdf_mini_cheetah", {"GRBDA_NO_ANALYTIC": "1"}, "f64", "fd_derivatives"),
    ("dtau-alone-f32", "urdf_mini_cheetah", {}, "f32", "fd_dtau"),
    ("mass-crba-f64", "urdf_mini_cheetah", {}, "f64", "mass_matrix"),
    ("mass-unit-batch-f64", "urdf_mini_cheetah", {"GRBDA_NO_CRBA": "1"}, "f64", "mass_matrix"),
    ("id-derivs-f32", "urdf_mini_cheetah", {}, "f32", "rnea_derivatives"),
    ("id-derivs-f64", "urdf_mini_cheetah", {}, "f64", "rnea_derivatives"),
    ("manifold-tello-f64", "tello", {}, "f64", "fd_derivatives"),
    ("mass-manifold-tello-f64", "tello", {}, "f64", "mass_matrix"),
    ("manifold-four-bar-f64", "urdf_four_bar", {}, "f64", "fd_derivatives"),
    ("manifold-four-bar-full-constraint-f64", "urdf_four_bar", {"GRBDA_NO_SMALL_CONSTRAINT": "1"}, "f64", "fd_derivatives"),
    ("big-clusters-dtau-f64", "parallel_chain_exp_d10_l16", {}, "f64", "fd_dtau"),
    ("big-clusters-split-f64", "parallel_chain_exp_d10_l16", {}, "f64", "fd_derivatives"),
    ("projection-two-parent-f64", "two_parent", {}, "f64", "forward_dynamics"),
    ("projection-two-parent-f32", "two_parent", {}, "f32", "forward_dynamics"),
]

# id -> (kernel nodes, memset nodes) of the captured call, measured on the parent (which refuses none of the rows; a refusal would be
# pinned by its GrbdaError code)
EXPECTED = {
    "minv-f32": (4, 0),
    "minv-f64": (4, 0),
    "factor-f32": (3, 0),
    "factor-f64": (3, 0),
    "factor-widened-f32": (3, 0),
    "differences-f64": (9, 0),
    "dtau-alone-f32": (2, 0),
    "mass-crba-f64": (4, 0),
    "mass-unit-batch-f64": (3, 0),
    "id-derivs-f32": (8, 0),
    "id-derivs-f64": (8, 0),
    "manifold-tello-f64": (6, 0),
    "mass-manifold-tello-f64": (4, 3),
    "manifold-four-bar-f64": (6, 0),
    "manifold-four-bar-full-constraint-f64": (6, 0),
    "big-clusters-dtau-f64": (4, 3),
    "big-clusters-split-f64": (20, 3),
    "projection-two-parent-f64": (6, 0),
    "projection-two-parent-f32": (6, 0),
}


def measure(row, gpu, monkeypatch):
    """(kernel nodes, memset nodes) of one captured call of the row, or the error code of its refusal"""
    import torch

    _, model, env, dtype_name, entry = row
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob = _model(model)
    plan = G.Plan(blob)
    _, x = _inputs(blob, plan, B, 1, torch.float64 if dtype_name == "f64" else torch.float32, gpu)
    call = ENTRY_HERE[entry][0]
    try:
        cap = capture(lambda: call(plan, x))
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
    print(f"{row[0]}: {got} (parent: {EXPECTED.get(row[0])})")
    assert got == EXPECTED[row[0]]
