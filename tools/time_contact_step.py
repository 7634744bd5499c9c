"""Time the scheduled contacts against the same work composed from the existing calls, with hipEvents, all contacts active:
    contact_step              against  contact_impulse + contact_dynamics + integrate
    contact_dynamics_active   against  contact_dynamics
for MIT Humanoid with two feet and Mini Cheetah with four feet, fp32 and fp64, at 262 144 states: the median of `reps` event-timed
batches of `iters` calls each, and the peak device memory of each side (every work pool released in between).
usage: python tools/time_contact_step.py [iters] [B] [reps]"""
import os, struct, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import generalized_rbda_amd as G
from generalized_rbda_amd.states import random_states

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
DT = 1e-3
WORKLOADS = [("mit_humanoid", ["left_ankle_link", "right_ankle_link"], [(0.0, 0.0, -0.05)] * 2),
             ("mini_cheetah", ["FR_knee_link", "FL_knee_link", "HR_knee_link", "HL_knee_link"], [(0.0, 0.0, -0.2)] * 4)]


def body_names(blob):
    _, _, nb, nc = struct.unpack_from("<II2i", blob, 0)
    n_ints, n_dbls, n_names = struct.unpack_from("<3i", blob, 28)
    off = 96 + 416 * nb + 64 * nc + 4 * ((n_ints + 1) & ~1) + 8 * n_dbls
    return [n.decode() for n in blob[off: off + n_names].split(b"\0")[:nb]]


def timed(plan, fn):
    """(median over `reps` of the mean hipEvent time of `iters` calls, ms; peak device memory above what was held before, MiB)"""
    torch.cuda.synchronize()
    plan.release_work()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    fn()
    torch.cuda.synchronize()
    low = torch.cuda.mem_get_info()[0]
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
        low = min(low, torch.cuda.mem_get_info()[0])
    return float(np.median(ms)), (free0 - low) / 2**20


print("| model | contacts | precision | contact_step ms | composed ms | step MiB | composed MiB | dynamics_active ms | contact_dynamics ms | "
      "active MiB | dynamics MiB |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
for model, links, offsets in WORKLOADS:
    plan = G.Plan.from_urdf(os.path.join(ROOT, "tests/golden/robot-models", model + ".urdf"))
    names = body_names(plan.blob)
    bodies, n = [names.index(l) for l in links], len(links)
    n0 = 4096
    q, qd, tau = random_states(plan.blob, n0, 3)
    for dtype, label in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        tq, tqd, tt = (torch.as_tensor(np.tile(a, (B // n0, 1)), dtype=dtype, device=dev) for a in (q, qd, tau))
        nB = tq.shape[0]
        full = torch.full((nB,), (1 << n) - 1, dtype=torch.int32, device=dev)
        none = torch.zeros((nB,), dtype=torch.int32, device=dev)  # (everything closes in this step: the impulse stage does its full work)

        def composed():
            v, _ = plan.contact_impulse(tq, tqd, bodies, offsets)
            ydd, _, _ = plan.contact_dynamics(tq, v, tt, bodies, offsets)
            return plan.integrate(tq, v, ydd, DT)

        t_step, m_step = timed(plan, lambda: plan.contact_step(tq, tqd, tt, bodies, offsets, full, DT, prev_active=none))
        t_comp, m_comp = timed(plan, composed)
        t_act, m_act = timed(plan, lambda: plan.contact_dynamics_active(tq, tqd, tt, bodies, offsets, full))
        t_dyn, m_dyn = timed(plan, lambda: plan.contact_dynamics(tq, tqd, tt, bodies, offsets))
        bad = G.spd_bad_pivots(0, reset=True)
        print(f"| {model} | {n} | {label} | {t_step:.4f} | {t_comp:.4f} | {m_step:.0f} | {m_comp:.0f} | {t_act:.4f} | {t_dyn:.4f} | {m_act:.0f} | "
              f"{m_dyn:.0f} |" + (f" bad_pivots={bad}" if bad else ""), flush=True)
        del tq, tqd, tt, full, none
