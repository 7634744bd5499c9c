"""The fp32 chain forward dynamics whose lanes fetch their own rows of qd and tau (and of q, where its rows allow it) from global memory
instead of through LDS (devmath.h, load_row_regs; devplan.h, chain_direct_inputs), and its slab without input rows (devplan.h,
chain_slab_rows) -- run with -m gpu.

An input goes direct when its rows are whole 16-byte units and its base is 16-byte aligned: qd and tau of the MIT Humanoid (nv = 24) do,
its q (25 columns) stays staged; Mini Cheetah (19 / 18) stages everything; limbs on the ground with nq = nv = 16 or 32 fetch all three
(32: the prologue without room for three staged blocks).  What can go wrong is a row of the wrong lane or tile, a ragged tile reading past
the batch, a misaligned base taken for an aligned one, the floating base's velocity read from the wrong registers, and a slab sized by one
rule and indexed by another.  Every comparison with the fp64 oracle holds TOL32 in rel_err of tests/test_gpu_parity.py, on
fp32-representable inputs; plans are compiled with latency mode off, so that the small batches run the kernel the large ones run."""
import functools
import os

import numpy as np
import pytest

import generalized_rbda_amd as G
import oracle_py as O
import term_states as TS
from graph_capture import capture
from models import ROBOT_MODELS, valid_states
from test_gpu_parity import TOL32, rel_err
from test_inreg_inputs_gpu import INREG, limbs_on_the_ground

pytestmark = pytest.mark.gpu
RAGGED = (1, 63, 64, 65, 129)
PERIOD = 1031          # states drawn for the long batch (a prime: no tile, and no multiple of the grid, brings the same rows back)
LONG_B = 2048 * 64 + 65  # more tiles than the launch's grid (8 wavefronts on each of 256 compute units), a ragged last one
GROUND = {"limbs_4x4_nv16": (4,) * 4, "limbs_8x4_nv32": (4,) * 8}


@functools.lru_cache(maxsize=None)
def case(model, n=max(RAGGED)):
    """(plan with latency mode off, q, qd, tau rounded to fp32, fp64 oracle), shared and read-only"""
    blob = limbs_on_the_ground(GROUND[model]) if model in GROUND else G.urdf_to_blob(os.path.join(ROBOT_MODELS, model + ".urdf"))
    q, qd, tau = (TS._frozen(TS.fp32_rounded(a)) for a in valid_states(blob, n, config_index=31))
    return TS.compile_under(blob, TS.ROUTES["chain"][0]), blob, q, qd, tau, TS._frozen(O.forward_dynamics(blob, q, qd, tau))


def dev(a, gpu):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)


def fd(plan, q, qd, tau, **kw):
    import torch

    out = plan.forward_dynamics(q, qd, tau, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def padded(a, pad_rows, gpu):
    """the rows of `a` at the head of a buffer with pad_rows rows of NaN behind them"""
    import torch

    buf = torch.full((a.shape[0] + pad_rows, a.shape[1]), float("nan"), dtype=torch.float32, device=gpu)
    buf[: a.shape[0]] = dev(a, gpu)
    return buf[: a.shape[0]]


def shifted(a, gpu):
    """the same values in a view that starts one element into a larger tensor: a base that is 4-byte aligned only"""
    import torch

    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=gpu)
    view = buf[1 : 1 + a.size].view(a.shape)
    view.copy_(dev(a, gpu))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("B", RAGGED)
def test_ragged_and_seam_batches(B, gpu):
    plan, _, q, qd, tau, ref = case("mit_humanoid")
    assert INREG in plan.kernel_name("aba", "f32", B)
    exact = fd(plan, dev(q[:B], gpu), dev(qd[:B], gpu), dev(tau[:B], gpu))
    err = rel_err(exact.astype(np.float64), ref[:B])
    print(f"DIRECT mit_humanoid B={B}: rel err {err:.2e}")
    assert exact.shape == (B, plan.nv) and np.isfinite(exact).all()
    assert err < TOL32
    behind_nan = fd(plan, padded(q[:B], 64, gpu), padded(qd[:B], 64, gpu), padded(tau[:B], 64, gpu))
    assert np.array_equal(exact, behind_nan), "a lane consumed a row past the batch"


def test_second_trip_of_the_persistent_loop(gpu):
    plan, blob, q, qd, tau, ref = case("mit_humanoid", PERIOD)
    rows = np.arange(LONG_B) % PERIOD
    assert INREG in plan.kernel_name("aba", "f32", LONG_B)
    got = fd(plan, dev(q[rows], gpu), dev(qd[rows], gpu), dev(tau[rows], gpu))
    sample = np.unique(np.concatenate([np.arange(130), np.arange(LONG_B - 130, LONG_B), np.arange(0, LONG_B, 997)]))
    err = rel_err(got[sample].astype(np.float64), ref[rows[sample]])
    print(f"DIRECT mit_humanoid B={LONG_B}: rel err {err:.2e} over {len(sample)} rows")
    assert got.shape == (LONG_B, plan.nv) and np.isfinite(got).all()
    assert err < TOL32
    assert np.array_equal(got[PERIOD : 2 * PERIOD], got[:PERIOD]) and np.array_equal(got[-PERIOD:], got[rows[-PERIOD:]])


def test_misaligned_base_selects_the_staged_path(gpu):
    B = 65
    plan, _, q, qd, tau, ref = case("mit_humanoid")
    aligned = fd(plan, dev(q[:B], gpu), dev(qd[:B], gpu), dev(tau[:B], gpu))
    off = fd(plan, dev(q[:B], gpu), shifted(qd[:B], gpu), shifted(tau[:B], gpu))
    one = fd(plan, dev(q[:B], gpu), dev(qd[:B], gpu), shifted(tau[:B], gpu))
    assert np.isfinite(aligned).all() and rel_err(aligned.astype(np.float64), ref[:B]) < TOL32
    assert np.array_equal(aligned, off) and np.array_equal(aligned, one)


@pytest.mark.parametrize("model", ("mini_cheetah",) + tuple(GROUND))
def test_all_staged_and_all_direct_models(model, gpu):
    B = 65
    plan, _, q, qd, tau, ref = case(model)
    assert INREG in plan.kernel_name("aba", "f32", B)
    assert (plan.nq % 4 == 0 and plan.nv % 4 == 0) == (model in GROUND)
    got = fd(plan, dev(q[:B], gpu), dev(qd[:B], gpu), dev(tau[:B], gpu))
    err = rel_err(got.astype(np.float64), ref[:B])
    print(f"DIRECT {model} B={B} nq={plan.nq} nv={plan.nv}: rel err {err:.2e}")
    assert np.isfinite(got).all()
    assert err < TOL32
    if model in GROUND:  # the same states from misaligned bases: everything staged, the same bits
        assert np.array_equal(got, fd(plan, shifted(q[:B], gpu), shifted(qd[:B], gpu), shifted(tau[:B], gpu)))


def test_floating_base_velocity_from_registers(gpu):
    B = 65
    plan, blob, q, _, tau, _ = case("mit_humanoid")
    rng = np.random.default_rng(8)
    qd = np.zeros((B, plan.nv))
    qd[:, :6] = TS.fp32_rounded(rng.uniform(-2.0, 2.0, (B, 6)))  # the base's twist: the first six velocities; every joint at rest
    ref = O.forward_dynamics(blob, q[:B], qd, tau[:B])
    assert rel_err(ref, O.forward_dynamics(blob, q[:B], np.zeros_like(qd), tau[:B])) > 1e-2, "the twist must show in the result"
    got = fd(plan, dev(q[:B], gpu), dev(qd, gpu), dev(tau[:B], gpu))
    err = rel_err(got.astype(np.float64), ref)
    print(f"DIRECT mit_humanoid base twist only B={B}: rel err {err:.2e}")
    assert np.isfinite(got).all()
    assert err < TOL32


def test_graph_capture_on_a_second_stream(gpu):
    import torch

    B = 129
    plan, _, q, qd, tau, _ = case("mit_humanoid")
    tq, tqd, ttau = dev(q[:B], gpu), dev(qd[:B], gpu), dev(tau[:B], gpu)
    eager = fd(plan, tq, tqd, ttau)
    side = torch.cuda.Stream()
    outs = [torch.empty((B, plan.nv), dtype=torch.float32, device=gpu) for _ in range(3)]
    cap = capture(lambda: [plan.forward_dynamics(tq, tqd, ttau, out=o, stream=side) for o in outs], stream=side)
    for o in outs:
        o.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        replayed = cap.replay()
    try:
        for o in replayed:
            assert np.array_equal(o.cpu().numpy(), eager)
    finally:
        cap.drop()
