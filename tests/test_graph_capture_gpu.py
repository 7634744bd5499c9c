"""Graph capture of every stream-taking device entry point ("Graph capture"), fp32 and fp64, on each route a plan can take:
the rows of the entry-point table by number type (entry_points.TYPED), from forward dynamics to rollout (whose recorded trajectories
are allocated inside the captured call), the contact pipeline and the centroidal quantities.

For every case: (a) capture succeeds after one eager call of the same batch on the capturing stream; (b) two replays with fresh inputs
(written in place) equal, bit for bit, eager calls on those inputs; (c) a seeded sample agrees with the oracle at the tolerances of
test_gpu_parity.py; (d) the graph has the same nodes as a capture of the same call taken after an eager call of TWICE the batch on a
fresh stream -- the launch sequence a graph records does not depend on what the stream held before.  Then the refusals of the
contract: a capture that would have to grow a slab, and release_work while a stream captures, raise GRBDA_EINVAL before any launch.
graph_capture.py gives the capture helper and the lifetime rules these tests follow."""
import numpy as np
import pytest

import generalized_rbda_amd as G
from entry_points import B_CHAIN, CASES, ENTRY, IDS, TOL32, TOL64, TYPED, TYPED_IDS, _host, _inputs, _model  # noqa: F401
from graph_capture import capture
from models import zoo

pytestmark = pytest.mark.gpu
N_ORACLE = 6         # states of each replay checked against the oracle


@pytest.mark.parametrize("route,model,env,B,entry,dtype_name", [c + (dt,) for c, dt in TYPED], ids=TYPED_IDS)
def test_capture_replay_matches_eager_and_oracle(route, model, env, B, entry, dtype_name, gpu, monkeypatch):
    import torch

    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob = _model(model)
    plan = G.Plan(blob)
    if entry in ("aba", "rnea"):
        name = plan.kernel_name(entry, dtype_name, B)
        assert {"chain": "_chain_kernel<", "latency": "_chain_lm_kernel<", "interpreter": f"{entry}_kernel<", "gen1": "_gen1_kernel<"}.get(
            route, "") in name, name
    if route in ("spanning_tree", "two_parent"):
        assert plan.info().spanning_tree_route == 1
    call, check = ENTRY[entry]
    tol = TOL64 if dtype == torch.float64 else TOL32
    _, x = _inputs(blob, plan, B, 1, dtype, gpu)
    cap = capture(lambda: call(plan, x))  # (a)
    try:
        assert cap.nodes["kernel"] >= 1
        for seed in (2, 3):  # (b) fresh inputs in place, replay, against an eager call on the same inputs
            s, fresh = _inputs(blob, plan, B, seed, dtype, gpu)
            for k in x:
                x[k].copy_(fresh[k])
            got = _host(cap.replay())
            with torch.cuda.stream(cap.stream):  # (the eager call on the capturing stream: same slab, same chunks)
                want = _host(call(plan, x))
            cap.stream.synchronize()
            for a, b in zip(got, want):
                assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"replay {seed} differs from the eager call"
            if check is not None:  # (c)
                idx = np.random.default_rng(seed).choice(B, N_ORACLE, replace=False)
                check(blob, {k: v[idx] for k, v in s.items()}, [a[idx] for a in got], tol)
        nodes = cap.nodes
    finally:
        cap.drop()
    # (d) after an eager call of 2B on a fresh stream: the same launch sequence
    _, x2 = _inputs(blob, plan, 2 * B, 4, dtype, gpu)
    cap2 = capture(lambda: call(plan, x), warm=lambda: call(plan, x2))
    try:
        assert cap2.nodes == nodes, f"{cap2.nodes} after a warm-up of 2B, {nodes} after one of B"
    finally:
        cap2.drop()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
# (id, model, switches, entry point, warm-up B, captured B, the slab that would have to grow): the interpreter's scratch slab (its
# persistent grid grows with the batch up to n_cu * waves tiles), the work slab of the difference batches (fixed 256 MiB chunks), and the
# zero block of the inverse OSIM's force-propagation route -- both batches of 257 tiles, so that its scratch slab (a grid of
# min(4 n_cu, tiles) wavefronts) keeps its size and only the zero block, B nv scalars, would grow
REFUSALS = [
    ("ensure_scratch", "urdf_mit_humanoid", {"GRBDA_NO_CHAIN": "1"}, "aba", 200, 4 * 4096 + 3, "scratch slab"),
    ("ensure_work", "urdf_mini_cheetah", {"GRBDA_NO_CRBA": "1"}, "mass_matrix", 200, 4 * 4096 + 3, "work buffer"),
    ("inv_osim_zero_block", "urdf_mini_cheetah", {}, "inv_osim", 4 * 4096 + 1, 4 * 4096 + 3, "work buffer"),
]


@pytest.mark.parametrize("what,model,env,entry,B_warm,B_big,slab", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_capture_of_a_larger_batch_is_refused(what, model, env, entry, B_warm, B_big, slab, gpu, monkeypatch):
    import torch

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob = _model(model)
    plan = G.Plan(blob)
    call, _ = ENTRY[entry]
    _, small = _inputs(blob, plan, B_warm, 1, torch.float64, gpu)
    _, big = _inputs(blob, plan, B_big, 2, torch.float64, gpu)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        call(plan, small)
    stream.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with pytest.raises(G.GrbdaError) as err:
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            call(plan, big)
    assert err.value.code == -1 and "capture" in str(err.value) and slab in str(err.value), str(err.value)  # GRBDA_EINVAL
    from graph_capture import node_counts

    assert node_counts(g)["kernel"] == 0  # (host-side, before any launch; the graph is never replayed)
    stream.synchronize()
    g.reset()
    # (the refused graph goes HERE: `err` holds a traceback that holds this frame, and a graph left to the garbage collector may be
    # destroyed inside a later capture, where its destructor's device synchronisation is an error thrown out of a destructor)
    del g, err
    # the stream is usable again, and the small batch still captures
    cap = capture(lambda: call(plan, small), stream=stream)
    cap.drop()


def test_release_work_during_capture_is_refused(gpu):
    import torch

    blob = zoo()["urdf_mini_cheetah"]
    plan = G.Plan(blob)  # (a fresh plan: its only slab is the capturing stream's)
    _, x = _inputs(blob, plan, 200, 1, torch.float64, gpu)
    call, _ = ENTRY["fd_derivatives"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        call(plan, x)
    stream.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with pytest.raises(G.GrbdaError) as err:
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            call(plan, x)
            plan.release_work()
    assert err.value.code == -1
    stream.synchronize()
    g.reset()
    del g, err  # (as above: not left to a garbage collection inside a later capture)
    assert plan.release_work() > 0  # (the slab was kept, and goes now)


def test_capped_derivatives_capture_after_their_warm_up(gpu, monkeypatch):
    """GRBDA_WORK_MAX_MB=1, Mini Cheetah fp32, 20 000 states: the whole-batch ydd alone is larger than the cap, so the forward dynamics
    run per chunk; the eager call keeps within the cap, its capture needs no larger slab, and the replay equals the uncapped (one-chunk)
    call bit for bit (test_chunk_seams_gpu.py holds this route against the oracle at its seams)."""
    import torch

    monkeypatch.setenv("GRBDA_WORK_MAX_MB", "1")
    blob = zoo()["urdf_mini_cheetah"]
    plan = G.Plan(blob)
    B = 20000
    call, _ = ENTRY["fd_derivatives"]
    _, x = _inputs(blob, plan, B, 1, torch.float32, gpu)
    cap = capture(lambda: call(plan, x))
    try:
        got = _host(cap.replay())
        with torch.cuda.stream(cap.stream):
            want = _host(call(plan, x))
        cap.stream.synchronize()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert cap.nodes["kernel"] >= 3 * 10  # (many chunks)
    finally:
        cap.drop()
    held = plan.release_work()
    assert 0 < held <= (1 << 20) + 256
    monkeypatch.delenv("GRBDA_WORK_MAX_MB")
    whole = _host(call(plan, x))
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(got, whole)), "the capped replay differs from the one-chunk call"
