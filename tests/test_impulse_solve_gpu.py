"""impulse_solve_kernel (contact_kernels.hip) alone, held as test_contact_solve_gpu.py holds its sibling: Mini Cheetah, 130 states, n = 1 .. 8
contacts (contact_ref.SETS["cheetah_n*"]; mu = 0 for n <= 5, 1e-3 above) x {fp32, fp64}, v_des in U(-1, 1), e = 0.5.  Draws:
entry_points._states, seed 73 (rounded to float32 for the fp32 runs).

The kernel's inputs are public outputs: inv_osim, body_poses, body_twists at qd.  impulse_ref.solve_inputs forms A and rhs from those
DEVICE arrays in float64, and the device's impulse is held by its backward error |A x - rhs|_inf / (|A|_inf |x|_inf + |rhs|_inf) per state
(contact_ref.backward_error), which does not grow with cond(A).  Allowed: 4 x the worst of a plain numpy Cholesky of the same A, rhs in the
kernel's precision (contact_ref.cholesky_solve), and never more than m (3 m + 1) u (contact_ref.cholesky_bound) -- the rule of the
existing solve test.  Counter 0, everything finite.

Measured on an MI355X: see DESIGN.md 7g'."""
import functools

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import generalized_rbda_amd as G
import impulse_ref as I
import term_states as TS

pytestmark = pytest.mark.gpu
B, E = I.B_TOP, 0.5


@functools.lru_cache(maxsize=None)
def inputs(n, dtype):
    model, bodies, offsets = C.contact_set(f"cheetah_n{n}")
    blob = EP._model(model)
    rnd = TS.fp32_rounded if dtype == "f32" else (lambda a: a)
    q, qd, _ = (TS._frozen(rnd(a)) for a in EP._states(blob, B, I.SEED))
    vd = TS._frozen(rnd(np.random.default_rng(I.SEED + n).uniform(-1, 1, (B, n, 3))))
    return list(bodies), [tuple(o) for o in offsets], q, qd, vd


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", range(1, 9))
def test_impulse_solve_alone(n, dtype, gpu):
    import torch

    td, nd = (torch.float32, np.float32) if dtype == "f32" else (torch.float64, np.float64)
    plan = EP.plan_for("urdf_mini_cheetah", ())
    bodies, offsets, q, qd, vd = inputs(n, dtype)
    mu = 0.0 if n <= 5 else 1e-3
    tq, tqd, tvd = (torch.as_tensor(a, dtype=td, device=gpu) for a in (q, qd, vd))
    G.spd_bad_pivots(0, reset=True)
    qn, imp = plan.contact_impulse(tq, tqd, bodies, offsets, v_des=tvd, restitution=E, damping=mu)
    assert G.spd_bad_pivots(0, reset=True) == 0
    host = lambda t: t.detach().double().cpu().numpy()
    assert np.isfinite(host(qn)).all() and np.isfinite(host(imp)).all()
    A, rhs = I.solve_inputs(host(plan.inv_osim(tq, bodies, offsets)), host(plan.body_poses(tq)), host(plan.body_twists(tq, tqd, torch.zeros_like(tqd))),
                            bodies, offsets, vd, E, mu)
    got = C.backward_error(A, host(imp), rhs)
    yard = C.backward_error(A, C.cholesky_solve(A, rhs, nd), rhs)
    m = 3 * n
    allowed = min(4 * yard.max(), C.cholesky_bound(m, nd))
    lanes = G.contact_solve_launch(n, dtype)[0]
    print(f"cheetah_n{n} {dtype} lanes {lanes} backward error: measured {got.max():.2e} (state {int(got.argmax())}), yardstick {yard.max():.2e}, "
          f"ratio {got.max() / yard.max():.2f}, bound {C.cholesky_bound(m, nd):.2e}")
    assert got.max() <= allowed, (n, dtype, int(got.argmax()), got.max(), yard.max())
