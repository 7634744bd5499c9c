"""Frame Jacobians of the MIT Humanoid's two feet, fp32, on three paths: Plan.frame_jacobians without the drift, with the drift, and the
J output of Plan.inv_osim (which computes J H^-1 J^T as well).  Median of `reps` device-timed calls after two warm-up calls, outputs
allocated outside the timed region where the method takes them (frame_jacobians allocates its own: the caching allocator's reuse).
usage, on a machine with the GPU: python tools/time_frame_jacobians.py [B] [reps]"""
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
t = lambda a: torch.as_tensor(np.tile(a, ((B + 511) // 512, 1))[:B], dtype=torch.float32, device="cuda:0")
tq, tqd = t(q), t(qd)
print(f"{name} fp32 B {B}, feet {bodies}: route {plan.frame_jacobians_route(bodies)}", flush=True)


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


for frame in ("body", "world"):
    for what, fn in ((f"frame_jacobians {frame}, J", lambda: plan.frame_jacobians(tq, bodies, offsets, frame)),
                     (f"frame_jacobians {frame}, J and drift", lambda: plan.frame_jacobians(tq, bodies, offsets, frame, qd=tqd, drift=True))):
        med, lo, hi = timed(fn)
        print(f"{what}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) of {REPS}", flush=True)
med, lo, hi = timed(lambda: plan.inv_osim(tq, bodies, offsets, with_jacobian=True))
print(f"inv_osim with J (body): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) of {REPS}", flush=True)
