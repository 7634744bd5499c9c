"""Time `contact_impulse` against `contact_dynamics` on the same contact set and against its own inverse OSIM, with hipEvents, for MIT
Humanoid fp32 at 262 144 states: one point per sole (2 contacts, damping 0) and four corners per sole (8 contacts, rank 12 of 24,
damping 1e-3).  Also printed: the two forward-dynamics calls the pipeline contains (at rest, with and without external forces).
usage: python tools/time_contact_impulse.py [iters] [B]"""
import os, struct, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import generalized_rbda_amd as G
from generalized_rbda_amd.states import random_states

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
dev = torch.device("cuda:0")
plan = G.Plan.from_urdf(os.path.join(ROOT, "tests/golden/robot-models", "mit_humanoid.urdf"))
blob = plan.blob
_, _, nb, nc = struct.unpack_from("<II2i", blob, 0)
n_ints, n_dbls, n_names = struct.unpack_from("<3i", blob, 28)
off = 96 + 416 * nb + 64 * nc + 4 * ((n_ints + 1) & ~1) + 8 * n_dbls
names = [n.decode() for n in blob[off: off + n_names].split(b"\0")[:nb]]
left, right = names.index("left_ankle_link"), names.index("right_ankle_link")
corners = [(sx * 0.1, sy * 0.05, -0.05) for sx in (1, -1) for sy in (1, -1)]
SETS = [("2 contacts", [left, right], [(0.0, 0.0, -0.05)] * 2, 0.0), ("8 contacts", [left] * 4 + [right] * 4, corners * 2, 1e-3)]


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


n0 = 4096
q, qd, tau = random_states(blob, n0, 3)
tq, tqd, tt = (torch.as_tensor(np.tile(a, (B // n0, 1)), dtype=torch.float32, device=dev) for a in (q, qd, tau))
zero = torch.zeros_like(tqd)
fe = torch.zeros((tq.shape[0], plan.n_bodies, 6), dtype=torch.float32, device=dev)
t_aba = timed(lambda: plan.forward_dynamics(tq, zero, zero))
t_aba_fe = timed(lambda: plan.forward_dynamics(tq, zero, zero, f_ext=fe))
print(f"mit_humanoid f32 B={tq.shape[0]}: at rest aba={t_aba:.4f}ms aba_with_f_ext={t_aba_fe:.4f}ms two_calls={t_aba + t_aba_fe:.4f}ms", flush=True)
for label, bodies, offsets, mu in SETS:
    t_ci = timed(lambda: plan.contact_impulse(tq, tqd, bodies, offsets, damping=mu))
    t_cd = timed(lambda: plan.contact_dynamics(tq, tqd, tt, bodies, offsets, damping=mu))
    t_osim = timed(lambda: plan.inv_osim(tq, bodies, offsets))
    bad = G.spd_bad_pivots(0, reset=True)
    print(f"  {label} (damping {mu:g}): contact_impulse={t_ci:.4f}ms = {t_ci / t_cd:.2f} x contact_dynamics ({t_cd:.4f}ms) = "
          f"{t_ci / t_osim:.2f} x inv_osim ({t_osim:.4f}ms) bad_pivots={bad}", flush=True)
