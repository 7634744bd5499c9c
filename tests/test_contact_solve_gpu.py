"""contact_solve_kernel (contact_kernels.hip) held to a reference at every contact count, lane width and failure.  Draws: entry_points._states,
seed 61 (rounded to float32 for the fp32 runs); B = lanes + 1 (one workgroup and one state, the width from
grbda_contact_solve_launch) and 130.

1  The solve alone, n = 1 .. 8 contacts x {fp32, fp64} on the Mini Cheetah (contact_ref.SETS["cheetah_n*"]), and in fp64 TelloWithArms
   (implicit clusters) and two_parent (unit-wrench inverse OSIM).  The kernel's inputs are public outputs (inv_osim, body_poses, body_twists
   at the returned ydd_free); contact_ref.solve_inputs forms A and rhs from those DEVICE arrays in float64, and the device's lambda is held
   by its backward error |A lambda - rhs|_inf / (|A|_inf |lambda|_inf + |rhs|_inf) per state, which does not grow with cond(A).  Allowed:
   4 x the worst of a plain numpy Cholesky of the same A, rhs in the kernel's precision, and never more than m (3 m + 1) u.  Then the
   wrench rows (ydd against forward_dynamics with contact_ref.wrenches of the device's lambda, TOL64 / TOL32), the constraint
   p_ddot(ydd) + mu lambda = a_des on the device outputs, and: counter 0, everything finite.
   The constraint in fp64 is held at 1e-8 on the scale 1 + |a_des|_inf as in test_contact_gpu.py.  In fp32 that scale is not honest for
   the damped sets: p_ddot(ydd) is p_ddot(ydd_free) + (A - mu I) lambda, two terms of size |rhs| and |A| |lambda| (up to 1e5 here) that
   cancel, each evaluated by fp32 forward dynamics and kinematics; it is held at TOL32 on the scale 1 + |A|_inf |lambda|_inf + |rhs|_inf.
2  ydd_free == NULL through the C ABI: the bits of the call that keeps ydd_free, at one chunk and under GRBDA_WORK_MAX_MB.
3  The failure contract state by state: (a) NaN positions in the first lane, the last lane of a workgroup, the first of the next and the
   ragged tail; (b) an exactly singular matrix in every state.
4  One launch past grid_cap x lanes states: the grid-stride loop of the solve takes a second trip.

Measured on an MI355X: see DESIGN.md 7g."""
import ctypes
import functools

import numpy as np
import pytest

import contact_ref as C
import entry_points as EP
import generalized_rbda_amd as G
import term_states as TS
from test_contact_gpu import B_TOP, SEED, _dev, _np, draw, points_of

pytestmark = pytest.mark.gpu

# (id, model, contact set or None = one point on the last link, damping, external forces)
ROWS = [(f"cheetah_n{n}", "urdf_mini_cheetah", f"cheetah_n{n}", 0.0 if n <= 5 else 1e-3, n > 5) for n in range(1, 9)]
OTHER_BASES = [("tello2", "tello_with_arms", "tello_feet", 0.0, False), ("two_parent1", "two_parent", None, 0.0, False)]
CHAIN = ("rev_rotor_chain_4", "rev_rotor_chain_4", None, 1e-3, False)  # (item 3b with damping)
ALL_ROWS = {r[0]: r for r in ROWS + OTHER_BASES + [CHAIN]}
REF = {}  # (id, dtype) -> contact_ref.contact_dynamics of case(id, dtype)


@functools.lru_cache(maxsize=None)
def case(rid, dtype="f64"):
    """(blob, bodies, offsets, (q, qd, tau, f_ext, a_des), mu) of B_TOP states, computed once and never written to; for "f32" every input
    is rounded to float32 first (the fp64 runs keep the draws: a rounded quaternion is not a unit quaternion to double precision).  The
    float64 reference alone must be well-posed: its A is positive definite in every state (REF keeps it)"""
    _, name, key, mu, fext = ALL_ROWS[rid]
    blob = EP._model(name)
    bodies, offsets = C.contact_set(key)[1:] if key else points_of(name)
    q, qd, tau = draw(name, dtype == "f32")
    rng = np.random.default_rng(SEED)
    rnd = TS.fp32_rounded if dtype == "f32" else TS._frozen
    fe = rnd(rng.uniform(-1, 1, (B_TOP, EP.K._parse(blob)["nb"], 6))) if fext else None
    ad = rnd(rng.uniform(-1, 1, (B_TOP, len(bodies), 3)))
    ref = C.contact_dynamics(blob, q, qd, tau, bodies, offsets, ad, mu, fe)
    assert np.linalg.eigvalsh(ref["A"]).min() > 0, f"{rid}: the reference's matrix is not positive definite"
    REF[rid, dtype] = ref
    return blob, list(bodies), [tuple(o) for o in offsets], (q, qd, tau, fe, ad), mu


def _torch_dtype(dtype):
    import torch

    return torch.float32 if dtype == "f32" else torch.float64


def _batches(n, dtype):
    return sorted({G.contact_solve_launch(n, dtype)[0] + 1, B_TOP})


def check_outputs(plan, rid, B, dtype, gpu, outs, what=""):
    """item 1's checks of (ydd, lambda, ydd_free) = outs, device tensors of the first B states of case(rid)"""
    blob, bodies, offsets, (q, qd, tau, fe, ad), mu = case(rid, dtype)
    td, nd = _torch_dtype(dtype), (np.float32 if dtype == "f32" else np.float64)
    tol = EP.TOL32 if dtype == "f32" else EP.TOL64
    t = lambda a: _dev(a, B, td, gpu)
    tq, tqd, ttau = t(q), t(qd), t(tau)
    ydd, lam, free = outs
    m, tag = 3 * len(bodies), f"{rid} {dtype} B={B}{what}"
    assert all(np.isfinite(_np(o)).all() for o in outs), f"{tag}: not finite"
    # the solve by its backward error, on the arrays the kernel read
    A, rhs = C.solve_inputs(_np(plan.inv_osim(tq, bodies, offsets)), _np(plan.body_poses(tq)), _np(plan.body_twists(tq, tqd, free)), bodies,
                            offsets, ad[:B], mu, EP.K._parse(blob)["grav"][3:])
    got = C.backward_error(A, _np(lam), rhs)
    yard = C.backward_error(A, C.cholesky_solve(A, rhs, nd), rhs)
    allowed = min(4 * yard.max(), C.cholesky_bound(m, nd))
    print(f"{tag} backward error: measured {got.max():.2e} (state {int(got.argmax())}), yardstick {yard.max():.2e}, "
          f"ratio {got.max() / yard.max():.2f}, bound {C.cholesky_bound(m, nd):.2e}")
    assert got.max() <= allowed, (tag, int(got.argmax()), got.max(), yard.max())
    # the wrench rows: ydd is the forward dynamics under f_ext + [p x lambda_c; lambda_c] of the device's lambda
    w = C.wrenches(blob, q[:B], bodies, offsets, _np(lam), None if fe is None else fe[:B])
    err = C.rel_per_state(_np(ydd), _np(plan.forward_dynamics(tq, tqd, ttau, f_ext=t(w))))
    print(f"{tag} wrenches: {err.max():.2e}")
    assert err.max() < tol, (tag, "wrenches", int(err.argmax()), err.max())
    # the constraint, on the device outputs alone
    acc = _np(plan.contact_points(tq, bodies, offsets, qd=tqd, ydd=ydd)[2])
    if dtype == "f64":
        err = C.rel_per_state(acc + mu * _np(lam), ad[:B])
        bound = 1e-8
    else:
        scale = 1 + np.abs(A).sum(axis=2).max(axis=1) * np.abs(_np(lam)).reshape(B, -1).max(axis=1) + np.abs(rhs).max(axis=1)
        err = np.abs(acc + mu * _np(lam) - ad[:B]).reshape(B, -1).max(axis=1) / scale
        bound = EP.TOL32
    print(f"{tag} constraint: {err.max():.2e}")
    assert err.max() < bound, (tag, "constraint", int(err.argmax()), err.max())


def run(plan, rid, B, dtype, gpu, mu=None, q=None):
    """contact_dynamics on the first B states of case(rid): (outs, states counted)"""
    blob, bodies, offsets, (q0, qd, tau, fe, ad), mu0 = case(rid, dtype)
    t = lambda a: _dev(a, B, _torch_dtype(dtype), gpu)
    G.spd_bad_pivots(0, reset=True)
    outs = plan.contact_dynamics(t(q0 if q is None else q), t(qd), t(tau), bodies, offsets, a_des=t(ad), damping=mu0 if mu is None else mu,
                                 f_ext=t(fe))
    return outs, G.spd_bad_pivots(0, reset=True)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_solve_alone(row, dtype, gpu):
    """fp64 with 7 contacts is the one launch that asks for more than 64 KiB of dynamic LDS (129 024 B)"""
    rid, name = row[:2]
    plan = EP.plan_for(name, ())
    for B in _batches(len(case(rid)[1]), dtype):
        outs, bad = run(plan, rid, B, dtype, gpu)
        assert bad == 0, (rid, dtype, B, bad)
        check_outputs(plan, rid, B, dtype, gpu, outs)


@pytest.mark.parametrize("row", OTHER_BASES, ids=[r[0] for r in OTHER_BASES])
def test_solve_alone_other_bases_fp64(row, gpu):
    rid, name = row[:2]
    plan = EP.plan_for(name, ())
    for B in _batches(len(case(rid)[1]), "f64"):
        outs, bad = run(plan, rid, B, "f64", gpu)
        assert bad == 0, (rid, B, bad)
        check_outputs(plan, rid, B, "f64", gpu, outs)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_null_ydd_free_gives_the_same_bits(gpu, monkeypatch):
    """without ydd_free the pipeline carves the unconstrained accelerations from its work slab"""
    import torch

    from test_chunk_seams_gpu import CAP_MB

    plan = G.Plan(EP._model("urdf_mini_cheetah"))
    blob, bodies, offsets, (q, qd, tau, fe, ad), mu = case("cheetah_n4")
    B, n = B_TOP, len(bodies)
    tq, tqd, ttau, tad = (_dev(a, B, torch.float64, gpu) for a in (q, qd, tau, ad))
    want = [_np(o) for o in plan.contact_dynamics(tq, tqd, ttau, bodies, offsets, a_des=tad)][:2]
    bod, off = (ctypes.c_int * n)(*bodies), (ctypes.c_double * (3 * n))(*[x for o in offsets for x in o])

    def call():
        ydd, lam = torch.full((B, plan.nv), float("nan"), dtype=torch.float64, device=gpu), torch.full((B, n, 3), float("nan"), dtype=torch.float64, device=gpu)
        rc = G.lib().grbda_contact_dynamics_f64(plan._h, tq.data_ptr(), tqd.data_ptr(), ttau.data_ptr(), None, n, bod, off, tad.data_ptr(), 0.0,
                                                ydd.data_ptr(), lam.data_ptr(), None, B, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, G.lib().grbda_last_error()
        torch.cuda.synchronize()
        return [_np(ydd), _np(lam)]

    plan.release_work()
    whole = call()
    assert plan.release_work() > (CAP_MB << 20) + 256, "the batch fits the cap in one chunk: nothing is tested"
    monkeypatch.setenv("GRBDA_WORK_MAX_MB", str(CAP_MB))
    chunked = call()
    assert 0 < plan.release_work() <= (CAP_MB << 20) + 256
    for name, a, b, w in zip(("ydd", "lambda"), whole, chunked, want):
        assert np.array_equal(a, w), f"{name}: one chunk without ydd_free differs from the call that keeps it"
        assert np.array_equal(b, w), f"{name}: the chunked call without ydd_free differs from the call that keeps it"


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nan_states_poison_nobody_and_are_counted(dtype, gpu):
    """(a) a pivot that is not finite, in chosen states: NaN positions (the model has no iteration: NaN only propagates).
    The counter: the word behind spd_bad_pivots is shared by the pipeline's kernels, and the forward dynamics count a state whose
    D = S^T IA S has a pivot that is not positive or not a number (ChainMem::pivot in chain_kernels.hip, Slots::pivot in kernels.hip:
    !(d > 0)) -- with NaN positions that is every such state, once per launch.  The pipeline launches forward dynamics twice (ydd_free on
    the chain kernel, ydd on the interpreter with the wrench rows) and the solve once; the inverse OSIM's sweep sets the same mask but
    never flushes it, poses and twists do not count.  So a NaN state is counted exactly three times."""
    rid = "cheetah_n4"
    plan = EP.plan_for("urdf_mini_cheetah", ())
    blob, bodies, offsets, (q, qd, tau, fe, ad), mu = case(rid, dtype)
    B, lanes = B_TOP, G.contact_solve_launch(len(bodies), dtype, 0)[0]
    assert lanes == (32 if dtype == "f64" else 64)
    hit = [0, lanes - 1, lanes, B - 1]
    clean, bad = run(plan, rid, B, dtype, gpu)
    assert bad == 0
    qn = np.array(q)
    qn[hit] = np.nan
    outs, bad = run(plan, rid, B, dtype, gpu, q=qn)
    ok = np.setdiff1d(np.arange(B), hit)
    for name, a, b in zip(("ydd", "lambda", "ydd_free"), outs, clean):
        a, b = _np(a).reshape(B, -1), _np(b).reshape(B, -1)
        if name != "ydd_free":
            assert np.isnan(a[hit]).all(), f"{name}: a NaN state has an entry that is a number"
        rows = np.flatnonzero((a[ok] != b[ok]).any(axis=1))
        assert rows.size == 0, f"{name}: states {ok[rows].tolist()} differ from the clean batch"
    assert bad == 3 * len(hit), f"{bad} counted for {len(hit)} NaN states (forward dynamics, solve, forward dynamics: 3 each)"


@functools.lru_cache(maxsize=None)
def chain_case():
    """one contact on the last link of the fixed-base chain whose joint axes are all z: the point cannot move along z, the z row of J_w
    is made of exact zeros, and so is row 2 of A = J_w H^-1 J_w^T"""
    case(CHAIN[0])
    ref = REF[CHAIN[0], "f64"]
    A0 = np.einsum("bij,bjk,blk->bil", ref["Jw"], ref["Hinv"], ref["Jw"])
    assert (A0[:, 2, :] == 0).all() and np.linalg.eigvalsh(A0[:, :2, :2]).min() > 0
    return ref["ydd_free"]


def test_singular_matrix_in_every_state(gpu):
    """(b) a pivot that is exactly zero, in every state (mu = 0); with mu = 1e-3 the same call solves"""
    rid = CHAIN[0]
    plan = EP.plan_for(rid, ())
    free_ref = chain_case()
    B = B_TOP
    (ydd, lam, free), bad = run(plan, rid, B, "f64", gpu, mu=0.0)
    print(f"{rid} mu = 0: {bad} of {B} states counted")
    assert bad == B
    assert np.isnan(_np(ydd)).all() and np.isnan(_np(lam)).all()
    err = C.rel_per_state(_np(free), free_ref)
    assert err.max() < EP.TOL64, (int(err.argmax()), err.max())
    outs, bad = run(plan, rid, B, "f64", gpu)
    assert bad == 0
    check_outputs(plan, rid, B, "f64", gpu, outs, " mu=1e-3")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_second_trip_of_the_grid(gpu):
    """fp64 with 8 contacts: 16 lanes, 3 workgroups per CU, the smallest grid capacity of the table.  The 130 states are tiled to
    grid_cap x lanes + lanes + 1 states; replica 0 is held to item 1's checks and every other replica to replica 0's bits."""
    import torch

    rid, dtype = "cheetah_n8", "f64"
    plan = G.Plan(EP._model("urdf_mini_cheetah"))
    blob, bodies, offsets, (q, qd, tau, fe, ad), mu = case(rid)
    lanes, _, cap = G.contact_solve_launch(len(bodies), dtype, 0)
    B = cap * lanes + lanes + 1
    assert lanes == 16 and B > cap * lanes
    idx = np.arange(B) % B_TOP
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a[idx]), dtype=torch.float64, device=gpu)
    args = (t(q), t(qd), t(tau))
    call = lambda n: plan.contact_dynamics(*(a[:n] for a in args), bodies, offsets, a_des=t(ad)[:n], damping=mu, f_ext=t(fe)[:n])
    # one chunk: the slab of a one-tile call gives the bytes per state (slab = 256 + states rounded up to tiles of 64 x bytes per state)
    call(64)
    torch.cuda.synchronize()
    per_state = (plan.release_work() - 256) // 64
    G.spd_bad_pivots(0, reset=True)
    outs = call(B)
    bad = G.spd_bad_pivots(0, reset=True)
    held = plan.release_work()
    assert per_state > 0 and held == 256 + (B + 63) // 64 * 64 * per_state, \
        f"a slab of {held} B for {B} states of {per_state} B: the batch was split, the solve's grid-stride loop was not reached"
    assert bad == 0
    check_outputs(plan, rid, B_TOP, dtype, gpu, [o[:B_TOP].contiguous() for o in outs], f" of {B}")
    for name, o in zip(("ydd", "lambda", "ydd_free"), outs):
        o = _np(o).reshape(B, -1)
        rows = np.flatnonzero((o != o[idx]).any(axis=1))
        assert rows.size == 0, f"{name}: {rows.size} states differ from their replica in the first {B_TOP}, the first at {rows[:4].tolist()}"
