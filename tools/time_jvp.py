"""Time the Jacobian-vector products against what a forward-mode caller had to run before they existed, and against their
reverse-mode twins, with hipEvents after warm-up, for MIT Humanoid at 262 144 states and JVRC-1 at 1 048 576 states in fp32 and fp64:
    (a) fd_jvp         (b) fd_derivatives (all three matrices), then three torch.bmm with the tangents        (c) fd_vjp
    (d) id_jvp         (e) id_derivatives (all three matrices), then three torch.bmm                          (f) id_vjp
(c) and (f) run on the same states: they move the same bytes through the same stages as (a) and (d) and differ only in the contraction and
in one zero-velocity pair, so (a) - (c) and (d) - (f) bound what the row-wise contraction costs over the column-wise one.
Every side runs alone (the matrices of (b) / (e) leave no room for another side's); printed per side: the median and the fastest repeat,
and the peak memory beyond the inputs -- torch.cuda.max_memory_allocated (outputs, matrices) plus the work slabs the plan held
(release_work).  When the matrices of (b) / (e) do not fit, the batch is halved until they do and the B used is printed.
usage: python tools/time_jvp.py [iters] [repeats]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import generalized_rbda_amd as G
from generalized_rbda_amd.states import valid_random_states_device

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 3
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")
MODELS = os.path.join(ROOT, "tests", "golden", "robot-models")
CASES = [("mit_humanoid", 262144), ("jvrc1_humanoid", 1048576)]


def timed(fn):
    """mean hipEvent time of `iters` calls, ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def multiplied(u, mats):
    """sum_k M_k u_k: the product the JVP returns, from the matrices"""
    return sum(torch.bmm(m, v.unsqueeze(2)).squeeze(2) for m, v in zip(mats.values(), u))


def inputs(plan, B, dtype):
    n0 = 4096
    q, qd, x, _ = valid_random_states_device(plan, n0, 3, dev)
    u = np.random.default_rng(5).uniform(-1, 1, (3, n0, plan.nv))
    u /= np.abs(u).sum(axis=2, keepdims=True)
    return [torch.as_tensor(np.tile(a, (B // n0, 1)), dtype=dtype, device=dev) for a in (q, qd, x, *u)]


def measure(plan, B, dtype, fn):
    """(times of the repeats, peak bytes beyond the inputs) of fn(q, qd, x, u), or None when the batch does not fit"""
    try:
        q, qd, x, *u = inputs(plan, B, dtype)
        plan.release_work()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(2):  # warm-up: tables, slabs, the allocator's blocks
            fn(q, qd, x, u)
        torch.cuda.synchronize()
        times = [timed(lambda: fn(q, qd, x, u)) for _ in range(repeats)]
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base + plan.release_work()
        return times, peak
    except (torch.cuda.OutOfMemoryError, G.GrbdaError) as e:
        print(f"    B={B}: {type(e).__name__} {str(e)[:80]}", flush=True)
        return None
    finally:
        q = qd = x = u = None
        torch.cuda.empty_cache()


for name, B in CASES:
    plan = G.Plan.from_urdf(os.path.join(MODELS, name + ".urdf"))
    for dtype in (torch.float32, torch.float64):
        sides = {"(a) fd_jvp": lambda q, qd, x, u: plan.fd_jvp(q, qd, x, *u),
                 "(b) fd_derivatives + bmm": lambda q, qd, x, u: multiplied(u, plan.fd_derivatives(q, qd, x)),
                 "(c) fd_vjp": lambda q, qd, x, u: plan.fd_vjp(q, qd, x, u[0]),
                 "(d) id_jvp": lambda q, qd, x, u: plan.id_jvp(q, qd, x, *u),
                 "(e) id_derivatives + bmm": lambda q, qd, x, u: multiplied(u, plan.id_derivatives(q, qd, x)),
                 "(f) id_vjp": lambda q, qd, x, u: plan.id_vjp(q, qd, x, u[0])}
        print(f"{name} {str(dtype)[6:]} nv={plan.nv} B={B}:", flush=True)
        for side, fn in sides.items():
            b, got = B, None
            while got is None and b >= 4096:
                got = measure(plan, b, dtype, fn)
                if got is None:
                    b //= 2
            if got is None:
                print(f"  {side}: no batch fits")
                continue
            times, peak = got
            med = float(np.median(times))
            print(f"  {side}: B={b} median {med:.3f} ms (min {min(times):.3f}), {med / b * 1e6:.1f} ns per state, peak memory "
                  f"{peak / 2 ** 20:.0f} MiB", flush=True)
