"""Time grbda_rnea_derivatives_* (d tau / d q and d tau / d qd) next to grbda_fd_derivatives_* on one model, hipEvents on the launch
stream: one warm-up call, then `iters` calls between two events, median of `reps` such measurements.
usage: python tools/time_id_derivs.py [model] [B] [iters] [id|fd|both]
Under `rocprofv3 --kernel-trace --stats -- python tools/time_id_derivs.py MODEL B 20 id` (or fd) the kernel table gives
rnea_deriv_kernel and unpack_runs_kernel on their own; the fd mode is the yardstick: the same recursion inside fd_derivatives."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import generalized_rbda_amd as G
from generalized_rbda_amd.states import random_states

model = sys.argv[1] if len(sys.argv) > 1 else "jvrc1_humanoid"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 131072
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
mode = sys.argv[4] if len(sys.argv) > 4 else "both"
plan = G.Plan.from_urdf(os.path.join(ROOT, "tests/golden/robot-models", model + ".urdf"))
q, qd, tau = random_states(plan.blob, B, 2)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


for dt in (torch.float32, torch.float64):
    t = lambda a: torch.as_tensor(a, dtype=dt, device="cuda:0")
    tq, tqd, tt = t(q), t(qd), t(tau)
    ydd = plan.forward_dynamics(tq, tqd, tt)
    nn, size = plan.nv * plan.nv, torch.finfo(dt).bits // 8
    res = {}
    if mode in ("id", "both"):
        res["id dq+dqd"] = timed(lambda: plan.id_derivatives(tq, tqd, ydd, want=("dq", "dqd")))
        res["id dq+dqd+dydd"] = timed(lambda: plan.id_derivatives(tq, tqd, ydd))
    if mode in ("fd", "both"):
        res["fd dq+dqd"] = timed(lambda: plan.fd_derivatives(tq, tqd, tt, want=("dq", "dqd")))
    print(f"{model} B={B} nv={plan.nv} {str(dt).split('.')[1]}: " + "  ".join(f"{k} = {v[0]:.3f} ms ({v[1]:.3f}..{v[2]:.3f})" for k, v in res.items()) +
          f"  [unpack traffic of dq+dqd: {2 * 2 * nn * size * B / 1e6:.1f} MB read + written]", flush=True)
