"""Time the time-stepping entry points: `integrate` alone, `step`, and the forward dynamics alone from the same run, with hipEvents,
for MIT Humanoid fp32 at 262 144 states and TelloWithArms fp32 at 1 048 576 states (the flagship sizes of DESIGN.md section 4).
Also printed: the bytes `integrate` moves -- (2 nq + 3 nv) sizeof(T) per state: q, qd, ydd in, q', qd' out -- as GB/s, to hold
against the copy rate of tools/traffic_calib.hip, and the ratio integrate / aba.
usage: python tools/time_step.py [iters]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import generalized_rbda_amd as G
from generalized_rbda_amd.robots import tello_with_arms
from generalized_rbda_amd.states import valid_random_states_device
import numpy as np

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda:0")
CASES = [("mit_humanoid", G.Plan.from_urdf(os.path.join(ROOT, "tests/golden/robot-models", "mit_humanoid.urdf")), 262144),
         ("tello_with_arms", G.Plan(tello_with_arms().serialize()), 1048576)]


def timed(fn):
    """mean hipEvent time of `iters` calls after one warm-up call, ms"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


for name, plan, B in CASES:
    dtype, size = torch.float32, 4
    # distinct valid states for a small batch, tiled to B: the integrator's cost does not depend on the values of an explicit model, and
    # the Newton projection of an implicit one takes the same number of iterations on every copy
    n0 = 4096
    q, qd, tau, _ = valid_random_states_device(plan, n0, 3, dev)
    rep = B // n0
    tq, tqd, tt = (torch.as_tensor(np.tile(a, (rep, 1)), dtype=dtype, device=dev) for a in (q, qd, tau))
    ydd = plan.forward_dynamics(tq, tqd, tt)
    qn, vn = torch.empty_like(tq), torch.empty_like(tqd)
    t_aba = timed(lambda: plan.forward_dynamics(tq, tqd, tt, out=ydd))
    t_int = timed(lambda: plan.integrate(tq, tqd, ydd, 1e-3, out=(qn, vn), tol=1e-3))
    t_step = timed(lambda: plan.step(tq, tqd, tt, 1e-3))
    nbytes = (2 * plan.nq + 3 * plan.nv) * size * B
    print(f"{name} f32 B={B} nq={plan.nq} nv={plan.nv}: aba={t_aba:.4f}ms integrate={t_int:.4f}ms step={t_step:.4f}ms "
          f"integrate/aba={t_int / t_aba:.3f} integrate_bytes={nbytes / 1e6:.1f}MB integrate_rate={nbytes / t_int / 1e6:.1f}GB/s "
          f"kernel={plan.kernel_name('aba', 'f32', B)}", flush=True)
