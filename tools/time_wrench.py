"""Time forward and inverse dynamics with wrenches on the two feet of the MIT Humanoid, fp32, 262 144 states, with hipEvents: the sparse
call (frame = body, frame = world) against the dense f_ext call with the same forces and against the plain call without forces, in ONE
session.  The calls are interleaved: three rounds, in each round every call is timed `iters` times (one event pair per call) and its
median kept; the figure of a call is the minimum of its three medians.
usage: python tools/time_wrench.py [iters] [B]"""
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


for algo, plain, sparse in (("aba", plan.forward_dynamics, plan.forward_dynamics_wrench), ("rnea", plan.inverse_dynamics, plan.inverse_dynamics_wrench)):
    calls = {"plain": lambda: plain(tq, tqd, tt, out=out),
             "dense f_ext": lambda: plain(tq, tqd, tt, out=out, f_ext=fe),
             "sparse body": lambda: sparse(tq, tqd, tt, feet, w, frame="body", out=out),
             "sparse world": lambda: sparse(tq, tqd, tt, feet, w, frame="world", out=out)}
    best = {k: min(m) for k, m in zip(calls, zip(*[[median_ms(fn) for fn in calls.values()] for _ in range(3)]))}
    print(f"mit_humanoid f32 B={B} {algo}: " + " ".join(f"{k.replace(' ', '_')}={v:.4f}ms" for k, v in best.items()), flush=True)
    print(f"  kernels: plain {plan.kernel_name(algo, 'f32', B)}; sparse {plan.wrench_kernel_name(algo, 'f32', feet, 'body', B)}", flush=True)
    print(f"  sparse body / dense f_ext = {best['sparse body'] / best['dense f_ext']:.3f}; sparse body / plain = {best['sparse body'] / best['plain']:.3f}; "
          f"sparse world / sparse body = {best['sparse world'] / best['sparse body']:.3f}", flush=True)
