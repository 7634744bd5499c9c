"""The fp32 chain forward dynamics that keeps a tile's inputs AND results in registers (aba_chain_kernel<float, 2, 3>): every lane fetches
its own rows of q, qd and tau from global memory at the element's own alignment (devmath.h, load_row_regs: 16-byte loads plus a narrow
tail), the acceleration sweep writes ydd[j] over tau[j] in the lane's register vector (chain_kernels.hip, ChainMemR::put_f), and the
epilogue stores the lane's own result row (devmath.h, store_row_regs) -- run with -m gpu.

What can go wrong: a column in the wrong register, a row of the wrong lane or tile, a byte read or written outside the arrays (the last
row's tail, a ragged tile), a 16-byte access that only works from a 16-byte base, a result left in the vector from the tile or the call
before, and the floating base's velocity read from the wrong registers.  Models: MIT Humanoid (nq 25: a tail of one column; nv 24), Mini
Cheetah (19 / 18: tails of three and two, no row a multiple of 16 bytes) and four limbs of four links on the ground (nq = nv = 16: no
tail).  Every comparison with the fp64 oracle holds TOL32 in rel_err of tests/test_gpu_parity.py on fp32-representable inputs; plans are
compiled with latency mode off, so that the small batches run the kernel the large ones run."""
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
PERIOD = 1031  # states drawn for the long batch (a prime: no tile, and no multiple of the grid, brings the same rows back)
GROUND = {"limbs_4x4_nv16": (4,) * 4}
MODELS = ("mit_humanoid", "mini_cheetah", "limbs_4x4_nv16")
SENTINEL = -12345.5
# the long batch runs a plan of its own, compiled under the library's launch-shape option of INTEGRATION.md section 3: that many
# one-wavefront workgroups per compute unit at the most, so the launch's grid is at most that times the device's compute units
WAVES_PER_CU = 8


@functools.lru_cache(maxsize=None)
def case(model, n=max(RAGGED)):
    """(plan with latency mode off, blob, q, qd, tau rounded to fp32, fp64 oracle), shared and read-only"""
    blob = limbs_on_the_ground(GROUND[model]) if model in GROUND else G.urdf_to_blob(os.path.join(ROBOT_MODELS, model + ".urdf"))
    q, qd, tau = (TS._frozen(TS.fp32_rounded(a)) for a in valid_states(blob, n, config_index=37))
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


def shifted(a, k, gpu):
    """the same values in a view that starts k elements into a larger tensor: a base 4 k bytes past a 16-byte boundary"""
    import torch

    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=gpu)
    assert buf.data_ptr() % 16 == 0
    view = buf[k : k + a.size].view(a.shape)
    view.copy_(dev(a, gpu))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * k
    return view


def fenced(shape, k, gpu):
    """(buffer filled with SENTINEL, a contiguous view of `shape` that starts k elements into it)"""
    import torch

    n = int(np.prod(shape))
    buf = torch.full((n + 2 * 64,), SENTINEL, dtype=torch.float32, device=gpu)
    return buf, buf[k : k + n].view(shape)


@pytest.mark.parametrize("B", RAGGED)
@pytest.mark.parametrize("model", MODELS)
def test_ragged_batches_and_stale_lanes(model, B, gpu):
    plan, _, q, qd, tau, ref = case(model)
    assert INREG in plan.kernel_name("aba", "f32", B)
    assert (plan.nq % 4 == 0) == (model in GROUND)
    exact = fd(plan, dev(q[:B], gpu), dev(qd[:B], gpu), dev(tau[:B], gpu))
    err = rel_err(exact.astype(np.float64), ref[:B])
    print(f"DIRECT-IO {model} B={B} nq={plan.nq} nv={plan.nv}: rel err {err:.2e}")
    assert exact.shape == (B, plan.nv) and np.isfinite(exact).all()
    assert err < TOL32
    behind_nan = fd(plan, padded(q[:B], 64, gpu), padded(qd[:B], 64, gpu), padded(tau[:B], 64, gpu))
    assert np.array_equal(exact, behind_nan), "a lane consumed a row past the batch"


def test_more_tiles_than_the_grid(gpu):
    import torch

    _, blob, q, qd, tau, ref = case("mit_humanoid", PERIOD)
    plan = TS.compile_under(blob, dict(TS.ROUTES["chain"][0], GRBDA_WAVES_PER_CU_ABA32=str(WAVES_PER_CU)))
    grid_cap = torch.cuda.get_device_properties(gpu).multi_processor_count * WAVES_PER_CU
    B = 2 * grid_cap * 64 + 1  # every workgroup takes a second trip at least, and the last tile, a single row, is somebody's third
    rows = np.arange(B) % PERIOD
    assert INREG in plan.kernel_name("aba", "f32", B)
    got = fd(plan, dev(q, gpu)[rows], dev(qd, gpu)[rows], dev(tau, gpu)[rows])
    sample = np.unique(np.concatenate([np.arange(130), np.arange(B - 130, B), np.arange(0, B, 997)]))
    err = rel_err(got[sample].astype(np.float64), ref[rows[sample]])
    print(f"DIRECT-IO mit_humanoid B={B}: rel err {err:.2e} over {len(sample)} rows")
    assert got.shape == (B, plan.nv) and np.isfinite(got).all()
    assert err < TOL32
    # the same state gives the same bits wherever it sits: first trip or a later one, a full tile or the lone last row
    whole = (B // PERIOD) * PERIOD
    assert np.array_equal(got[:whole].reshape(-1, PERIOD, plan.nv), np.broadcast_to(got[:PERIOD], (B // PERIOD, PERIOD, plan.nv)))
    assert np.array_equal(got[whole:], got[: B - whole])


@pytest.mark.parametrize("k", (1, 2, 3))
@pytest.mark.parametrize("model", MODELS)
def test_misaligned_bases(model, k, gpu):
    B = 65
    plan, _, q, qd, tau, ref = case(model)
    tq, tqd, ttau = dev(q[:B], gpu), dev(qd[:B], gpu), dev(tau[:B], gpu)
    aligned = fd(plan, tq, tqd, ttau)
    assert np.isfinite(aligned).all() and rel_err(aligned.astype(np.float64), ref[:B]) < TOL32
    assert np.array_equal(aligned, fd(plan, shifted(q[:B], k, gpu), shifted(qd[:B], k, gpu), shifted(tau[:B], k, gpu)))
    buf, out = fenced((B, plan.nv), k, gpu)
    assert out.data_ptr() % 16 == 4 * k
    assert np.array_equal(aligned, fd(plan, tq, tqd, ttau, out=out))


@pytest.mark.parametrize("B", (1, 65))
@pytest.mark.parametrize("model", MODELS)
def test_no_write_past_the_output(model, B, gpu):
    import torch

    plan, _, q, qd, tau, _ = case(model)
    expect = fd(plan, dev(q[:B], gpu), dev(qd[:B], gpu), dev(tau[:B], gpu))
    k, n = 64, B * plan.nv
    buf, out = fenced((B, plan.nv), k, gpu)
    got = fd(plan, dev(q[:B], gpu), dev(qd[:B], gpu), dev(tau[:B], gpu), out=out)
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    assert np.array_equal(got, expect) and np.array_equal(whole[k : k + n].reshape(B, plan.nv), expect)
    assert (whole[:k] == SENTINEL).all(), "a store in front of the output"
    assert (whole[k + n :] == SENTINEL).all(), "a store behind the output"


def test_floating_base_velocity_from_registers(gpu):
    B = 65
    plan, blob, q, _, tau, _ = case("mit_humanoid")
    rng = np.random.default_rng(9)
    qd = np.zeros((B, plan.nv))
    qd[:, :6] = TS.fp32_rounded(rng.uniform(-2.0, 2.0, (B, 6)))  # the base's twist: the first six velocities; every joint at rest
    ref = O.forward_dynamics(blob, q[:B], qd, tau[:B])
    assert rel_err(ref, O.forward_dynamics(blob, q[:B], np.zeros_like(qd), tau[:B])) > 1e-2, "the twist must show in the result"
    got = fd(plan, dev(q[:B], gpu), dev(qd, gpu), dev(tau[:B], gpu))
    err = rel_err(got.astype(np.float64), ref)
    print(f"DIRECT-IO mit_humanoid base twist only B={B}: rel err {err:.2e}")
    assert np.isfinite(got).all()
    assert err < TOL32


def test_tile_seam_between_calls(gpu):
    """B = 65 and then B = 64 of OTHER states on the same plan and stream: the second call's lanes start from the first call's leftovers"""
    plan, _, q, qd, tau, ref = case("mit_humanoid")
    first, second = slice(0, 65), slice(65, 129)
    alone = fd(plan, dev(q[second], gpu), dev(qd[second], gpu), dev(tau[second], gpu))
    assert rel_err(alone.astype(np.float64), ref[second]) < TOL32
    a = [dev(x[first], gpu) for x in (q, qd, tau)]
    b = [dev(x[second], gpu) for x in (q, qd, tau)]
    got_first = plan.forward_dynamics(*a)
    got_second = fd(plan, *b)
    assert rel_err(got_first.double().cpu().numpy(), ref[first]) < TOL32
    assert np.array_equal(got_second, alone), "a result of the first call showed in the second"


def test_graph_capture_on_a_second_stream(gpu):
    import torch

    B = 129
    plan, _, q, qd, tau, _ = case("mini_cheetah")
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
