"""J v and J^T f at the MIT Humanoid's two feet, fp32 and fp64, both frames: Plan.frame_jv, Plan.frame_jtf and the two in one call, against
what a caller does without them through the entry points that were there before --
    frame_jacobians followed by torch.einsum (either product);
    J v:    body_twists_list at (q, v, 0) (the velocity at the body origin; moving it to the point is left out of the timing);
    J^T f:  inverse_dynamics minus inverse_dynamics_wrench at qd = ydd = 0 (the wrench taken as it is);
and one body_poses_list call, the cost of ONE walk over the two feet's ancestors.
Device events around each call, two warm-up rounds, then `reps` rounds in which the paths take turns (interleaved), the median per path.
Peak memory beyond the inputs: torch.cuda.max_memory_allocated over one more call plus the work slab the plan held (release_work).
usage, on a machine with the GPU: python tools/time_jacobian_products.py [B] [reps]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch
import generalized_rbda_amd as G
import contact_ref as C
import entry_points as EP

B = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 11
name = "urdf_mit_humanoid"
blob = EP._model(name)
plan = G.Plan(blob)
bodies = [C.body_index(blob, nm) for nm in ("left_ankle_link", "right_ankle_link")]
offsets = [(0.0, 0.0, -0.05)] * 2
q, qd, _ = EP._states(blob, 512, 3)
rng = np.random.default_rng(5)
v, f = rng.uniform(-2, 2, size=(512, plan.nv)), rng.uniform(-3, 3, size=(512, len(bodies), 6))
print(f"{name} B {B}, feet {bodies}, nv {plan.nv}: route {plan.frame_jacobians_route(bodies)}", flush=True)


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


for dtype in (torch.float32, torch.float64):
    t = lambda a: torch.as_tensor(np.tile(a, ((B + 511) // 512,) + (1,) * (a.ndim - 1))[:B], dtype=dtype, device="cuda:0")
    tq, tv, tf = t(q), t(v), t(f)
    z = torch.zeros_like(tv)
    for frame in ("body", "world"):
        paths = {
            "frame_jv": lambda: plan.frame_jv(tq, tv, bodies, offsets, frame),
            "frame_jtf": lambda: plan.frame_jtf(tq, tf, bodies, offsets, frame),
            "frame_jacobian_products, both": lambda: plan.frame_jacobian_products(tq, bodies, v=tv, f=tf, offsets=offsets, frame=frame),
            "frame_jacobians + einsum, J v": lambda: torch.einsum("bcik,bk->bci", plan.frame_jacobians(tq, bodies, offsets, frame), tv),
            "frame_jacobians + einsum, J^T f": lambda: torch.einsum("bcik,bci->bk", plan.frame_jacobians(tq, bodies, offsets, frame), tf),
            "body_twists_list at (q, v, 0)": lambda: plan.body_twists_list(tq, tv, z, bodies),
            "inverse_dynamics - inverse_dynamics_wrench": lambda: plan.inverse_dynamics(tq, z, z) - plan.inverse_dynamics_wrench(tq, z, z, bodies, tf, frame),
            "body_poses_list (one walk)": lambda: plan.body_poses_list(tq, bodies),
        }
        for _ in range(2):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(REPS):
            for k, fn in paths.items():
                ms[k].append(one(fn))
        peak = {}
        for k, fn in paths.items():
            plan.release_work()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base + plan.release_work()
        for k in paths:
            print(f"{str(dtype)[6:]} {frame} | {k}: median {statistics.median(ms[k]):.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f}) of {REPS}, "
                  f"peak memory {peak[k] / 2 ** 20:.0f} MiB", flush=True)
