"""Time grbda_centroidal_* with all four outputs against what a user had to run before it existed -- grbda_body_poses_* followed by
grbda_body_twists_* on the same batch, before any reduction of their outputs -- with hipEvents, for MIT Humanoid fp32 at 262 144 states
and JVRC-1 fp32 at 1 048 576 states (the flagship sizes of DESIGN.md).  The two sides alternate within every repeat; printed: the median
and the fastest of the repeats, the ratio of the medians, and the bytes each side moves through HBM per state (inputs read once,
spanning rates written and read once, outputs written once).
usage: python tools/time_centroidal.py [iters] [repeats]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import generalized_rbda_amd as G
from generalized_rbda_amd.states import valid_random_states_device

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
MODELS = os.path.join(ROOT, "tests", "golden", "robot-models")
CASES = [("mit_humanoid", G.Plan.from_urdf(os.path.join(MODELS, "mit_humanoid.urdf")), 262144),
         ("jvrc1_humanoid", G.Plan.from_urdf(os.path.join(MODELS, "jvrc1_humanoid.urdf")), 1048576)]


def timed(fn):
    """mean hipEvent time of `iters` calls, ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


for name, plan, B in CASES:
    dtype, size, n0 = torch.float32, 4, 4096
    q, qd, ydd, _ = valid_random_states_device(plan, n0, 3, dev)
    tq, tqd, ty = (torch.as_tensor(np.tile(a, (B // n0, 1)), dtype=dtype, device=dev) for a in (q, qd, ydd))
    fused = lambda: plan.centroidal(tq, tqd, ty)
    both = lambda: (plan.body_poses(tq), plan.body_twists(tq, tqd, ty))
    for fn in (fused, both):  # warm-up: tables, slabs, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    t = {"fused": [], "both": []}
    for _ in range(repeats):
        t["fused"].append(timed(fused))
        t["both"].append(timed(both))
    ns, nb = plan.n_span_vel, plan.n_bodies
    span = 2 * 2 * ns  # written by the spanning stage, read by the walk
    b_fused = (2 * plan.nq + 2 * plan.nv + span + 18) * size          # q twice (both stages), qd, ydd, the rates, com + com_vel + h + hdot
    b_both = (3 * plan.nq + 2 * plan.nv + span + 24 * nb) * size      # q three times, qd, ydd, the rates, Xa and V
    mf, mb = float(np.median(t["fused"])), float(np.median(t["both"]))
    print(f"{name} f32 B={B} nq={plan.nq} nv={plan.nv} n_bodies={nb}: centroidal median {mf:.4f} ms (min {min(t['fused']):.4f}), "
          f"poses + twists median {mb:.4f} ms (min {min(t['both']):.4f}), ratio {mf / mb:.3f}; bytes per state {b_fused} against {b_both}", flush=True)
