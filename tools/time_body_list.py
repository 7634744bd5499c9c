"""Time the poses and twists of the two feet of the MIT Humanoid, fp32, 262 144 states, with hipEvents: body_poses against body_poses_list,
body_twists against body_twists_list, and the four rows of tools/time_wrench.py (plain, dense f_ext, sparse body, sparse world) for forward
and inverse dynamics, in ONE session.  The calls are interleaved: three rounds, in each round every call is timed `iters` times (one event
pair per call) after a warm-up call and its median kept; the figure of a call is the minimum of its three medians.

A library without the list entry points (an older build named by GRBDA_HIP_LIB) runs the rows it has: that is how the sparse world-frame
call of an earlier commit is measured next to this one's -- run the tool once per library, alternately.
usage: python tools/time_body_list.py [iters] [B]"""
import os, struct, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import generalized_rbda_amd as G
from generalized_rbda_amd.states import random_states

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
dev = torch.device("cuda:0")
plan = G.Plan.from_urdf(os.path.join(ROOT, "tests/golden/robot-models", "mit_humanoid.urdf"))
blob = plan.blob
_, _, nb, nc = struct.unpack_from("<II2i", blob, 0)
n_ints, n_dbls, n_names = struct.unpack_from("<3i", blob, 28)
off = 96 + 416 * nb + 64 * nc + 4 * ((n_ints + 1) & ~1) + 8 * n_dbls
names = [n.decode() for n in blob[off: off + n_names].split(b"\0")[:nb]]
feet = [names.index("left_ankle_link"), names.index("right_ankle_link")]
has_lists = hasattr(G.lib(), "grbda_body_poses_list_f32")

n0 = 4096
q, qd, tau = random_states(blob, n0, 3)
tq, tqd, tt = (torch.as_tensor(np.tile(a, (B // n0, 1)), dtype=torch.float32, device=dev) for a in (q, qd, tau))
B = tq.shape[0]
w = torch.as_tensor(np.random.default_rng(1).uniform(-50, 50, (B, 2, 6)), dtype=torch.float32, device=dev)
fe = torch.zeros((B, plan.n_bodies, 6), dtype=torch.float32, device=dev)
fe[:, feet] = w
out = torch.empty_like(tt)


def median_ms(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def best_of(calls):
    return {k: min(m) for k, m in zip(calls, zip(*[[median_ms(fn) for fn in calls.values()] for _ in range(3)]))}


print(f"library: {G.LIB_PATH} ({'with' if has_lists else 'without'} the list entry points)", flush=True)
calls = {"body_poses": lambda: plan.body_poses(tq), "body_twists": lambda: plan.body_twists(tq, tqd, tt)}
if has_lists:
    print(f"  feet {feet}: (walk length, saved at once, route) = {plan.body_list_walk(feet)} of {plan.n_bodies} bodies", flush=True)
    calls["body_poses_list"] = lambda: plan.body_poses_list(tq, feet)
    calls["body_twists_list"] = lambda: plan.body_twists_list(tq, tqd, tt, feet)
best = best_of(calls)
print(f"mit_humanoid f32 B={B} kinematics: " + " ".join(f"{k}={v:.4f}ms" for k, v in best.items()), flush=True)
if has_lists:
    print(f"  body_poses_list / body_poses = {best['body_poses_list'] / best['body_poses']:.3f}; "
          f"body_twists_list / body_twists = {best['body_twists_list'] / best['body_twists']:.3f}", flush=True)

for algo, plain, sparse in (("aba", plan.forward_dynamics, plan.forward_dynamics_wrench), ("rnea", plan.inverse_dynamics, plan.inverse_dynamics_wrench)):
    calls = {"plain": lambda: plain(tq, tqd, tt, out=out),
             "dense f_ext": lambda: plain(tq, tqd, tt, out=out, f_ext=fe),
             "sparse body": lambda: sparse(tq, tqd, tt, feet, w, frame="body", out=out),
             "sparse world": lambda: sparse(tq, tqd, tt, feet, w, frame="world", out=out)}
    best = best_of(calls)
    print(f"mit_humanoid f32 B={B} {algo}: " + " ".join(f"{k.replace(' ', '_')}={v:.4f}ms" for k, v in best.items()), flush=True)
    print(f"  sparse world / dense f_ext = {best['sparse world'] / best['dense f_ext']:.3f}; "
          f"sparse world - sparse body = {best['sparse world'] - best['sparse body']:.4f}ms", flush=True)
