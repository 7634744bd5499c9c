"""Time the reverse sweep of a rollout against its forward sweep and against what a caller had to run before it existed, with hipEvents
after warm-up, for Mini Cheetah at 262 144 states and JVRC-1 at 1 048 576 states in fp32 and fp64, T steps of dt = 0.01:
    (a) rollout(record=True)      the forward sweep of the same B, T
    (b) rollout_vjp               cotangents of every state, gradients of (q0, qd0, tau[T])
    (c) T x (fd_derivatives (all three matrices), then three torch.bmm with a cotangent): the dynamics part alone of a hand-written sweep
        (one step is timed and multiplied by T; the manifold part and the sums are left out of it)
Every side runs alone; printed per side: the median and the fastest repeat, and the peak memory beyond the inputs --
torch.cuda.max_memory_allocated (outputs, matrices) plus the work slabs the plan held (release_work).  When a side does not fit, the batch
is halved until it does and the B used is printed.
usage: python tools/time_rollout_vjp.py [T] [iters] [repeats]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import generalized_rbda_amd as G
from generalized_rbda_amd.states import valid_random_states_device

T = int(sys.argv[1]) if len(sys.argv) > 1 else 4
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 2
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
DT = 0.01
dev = torch.device("cuda:0")
MODELS = os.path.join(ROOT, "tests", "golden", "robot-models")
CASES = [("mini_cheetah", 262144), ("jvrc1_humanoid", 1048576)]


def timed(fn):
    """mean hipEvent time of `iters` calls, ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def contracted(g, mats):
    return [torch.bmm(g.unsqueeze(1), m).squeeze(1) for m in mats.values()]


def inputs(plan, B, dtype, recorded):
    """q, qd, tau[T], and for the reverse sweep the recorded trajectory and unit cotangents of every state"""
    n0 = 4096
    q, qd, x, _ = valid_random_states_device(plan, n0, 3, dev)
    q, qd, x = (torch.as_tensor(np.tile(a, (B // n0, 1)), dtype=dtype, device=dev) for a in (q, qd, x))
    x = x.unsqueeze(0).repeat(T, 1, 1)
    if not recorded:
        return q, qd, x
    qt, vt = plan.rollout(q, qd, x, DT, T, record=True)[3:]
    g = np.random.default_rng(5).uniform(-1, 1, (2, n0, plan.nv))
    g /= np.abs(g).sum(axis=(0, 2), keepdims=True)
    gq, gqd = (torch.as_tensor(np.tile(a, (B // n0, 1)), dtype=dtype, device=dev).unsqueeze(0).repeat(T, 1, 1) for a in g)
    return q, qd, x, qt, vt, gq, gqd


def measure(plan, B, dtype, fn, recorded):
    """(times of the repeats, peak bytes beyond the inputs) of fn(*inputs), or None when the batch does not fit"""
    args = None
    try:
        args = inputs(plan, B, dtype, recorded)
        plan.release_work()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(2):  # warm-up: tables, slabs, the allocator's blocks
            fn(*args)
        torch.cuda.synchronize()
        times = [timed(lambda: fn(*args)) for _ in range(repeats)]
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base + plan.release_work()
        return times, peak
    except (torch.cuda.OutOfMemoryError, G.GrbdaError) as e:
        print(f"    B={B}: {type(e).__name__} {str(e)[:80]}", flush=True)
        return None
    finally:
        args = None
        torch.cuda.empty_cache()


for name, B in CASES:
    plan = G.Plan.from_urdf(os.path.join(MODELS, name + ".urdf"))
    for dtype in (torch.float32, torch.float64):
        sides = {"(a) rollout": (False, 1, lambda q, qd, x: plan.rollout(q, qd, x, DT, T, record=True)),
                 "(b) rollout_vjp": (True, 1, lambda q, qd, x, qt, vt, gq, gqd: plan.rollout_vjp(q, qd, x, DT, qt, vt, gq, gqd)),
                 f"(c) {T} x (fd_derivatives + bmm)": (True, T, lambda q, qd, x, qt, vt, gq, gqd: contracted(gqd[0], plan.fd_derivatives(q, qd, x[0])))}
        print(f"{name} {str(dtype)[6:]} nv={plan.nv} B={B} T={T}:", flush=True)
        for side, (recorded, times_T, fn) in sides.items():
            b, got = B, None
            while got is None and b >= 4096:
                got = measure(plan, b, dtype, fn, recorded)
                if got is None:
                    b //= 2
            if got is None:
                print(f"  {side}: no batch fits")
                continue
            times, peak = got
            med = float(np.median(times)) * times_T
            print(f"  {side}: B={b} median {med:.3f} ms (min {min(times) * times_T:.3f}), {med / b * 1e6:.1f} ns per state, peak memory "
                  f"{peak / 2 ** 20:.0f} MiB", flush=True)
