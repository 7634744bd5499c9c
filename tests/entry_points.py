"""The table of device entry points the GPU tests share: ENTRY (name -> (call, oracle checker)), CASES (route x model x plan-time switches
x batch x entry point), and what makes their models, states and inputs.  A plain module, not a test file: test_graph_capture_gpu.py,
test_buffer_edges_gpu.py, test_batch_ladder_gpu.py and test_concurrent_streams_gpu.py all go through it, so an entry point added to the
library is covered by every one of them with one more row here.  Covered: forward / inverse dynamics (with and without f_ext), bias force,
mass matrix, the forward-dynamics derivatives, body poses and twists, applyTestForce, the inverse OSIM, the projection, the state
conversion, the spanning rates, the inverse-dynamics derivatives, integrate / step / rollout, contact points, contact dynamics and contact
impulses, energy, the centroidal quantities and the momentum matrix.

call(plan, x) returns a tuple of output tensors whose leading dimension is the batch, x holding the device tensors "q", "qd", "tau",
"fext", "force", "q_start", "q_proj", "a_des", "tau_T", "v_des"; check(blob, s, outs, tol) compares the numpy outputs `outs` of the states `s` (a
dict of numpy inputs) with the oracle, or with a numpy reference the CPU suite pins to the oracle.  The checkers of the later rows print
what they measured (HELD model type what: error of bound).  TYPED is the table by number type: the rows of CASES in fp64 and fp32 less
NOT_RUN, and what every one of the four files is parametrised over."""
import functools
import os

import numpy as np

import kinematics_ref as K
import oracle_py as O
import generalized_rbda_amd as G
from generalized_rbda_amd.states import parse_clusters, random_states
from models import ROBOT_MODELS, valid_states, zoo

TOL64 = 1e-9
TOL32 = 1e-3
B_CHAIN = 65536 + 37  # beyond four tiles per SIMD of 256 CUs: the chain kernels, not latency mode


_BIG = set()  # blobs of plans with clusters beyond the structured limits: the oracle built with room for them (big=True)


def _big(blob):
    return blob in _BIG


_zoo = functools.lru_cache(maxsize=None)(zoo)  # (the descriptions are immutable bytes: built once per process)
_NAMES = {}  # blob -> the name _model() made it under (a checker is handed the blob: its contact set and time step go by the name)


@functools.lru_cache(maxsize=None)
def _model(name):
    if name == "two_parent":
        from test_capi_cpu import two_parent_model

        blob = two_parent_model().serialize()
    elif name.startswith("parallel_chain"):
        blob = G.urdf_to_blob(os.path.join(ROBOT_MODELS, name + ".urdf"))
        _BIG.add(blob)
    else:
        blob = _zoo()[name]
    _NAMES.setdefault(blob, name)
    return blob


def _name(blob):
    return _NAMES.get(bytes(blob), "?")


def _states(blob, B, seed, max_cond=None):
    if _big(blob):
        return valid_states(blob, B, config_index=seed, big=True, scale=0.5, max_cond=50)
    if any(c[9] in (2, 3) for c in parse_clusters(blob)["clusters"]):  # implicit loops: states on the constraint manifold
        return valid_states(blob, B, config_index=seed, max_cond=max_cond)
    return random_states(blob, B, config_index=seed)


def _rel(a, b):
    return float(np.abs(a - b).max() / (1.0 + np.abs(b).max()))


def _fd_columns(blob, q, qd, tau, wrt):
    """d ydd / d tau (exact: linear) and d ydd / d qd (exact central difference: quadratic) of the oracle's forward dynamics"""
    B, nv = qd.shape
    out = np.empty((B, nv, nv))
    for k in range(nv):
        e = np.zeros((B, nv))
        e[:, k] = 1.0
        if wrt == "dtau":
            out[:, :, k] = O.forward_dynamics(blob, q, qd, tau + e) - O.forward_dynamics(blob, q, qd, tau)
        else:
            out[:, :, k] = (O.forward_dynamics(blob, q, qd + e, tau) - O.forward_dynamics(blob, q, qd - e, tau)) / 2
    return out


def _mass_oracle(blob, q):
    B, nv = q.shape[0], parse_clusters(blob)["nv"]
    z = np.zeros((B, nv))
    C = O.inverse_dynamics(blob, q, z, z, big=_big(blob))
    H = np.empty((B, nv, nv))
    for k in range(nv):
        e = np.zeros((B, nv))
        e[:, k] = 1.0
        H[:, :, k] = O.inverse_dynamics(blob, q, z, e, big=_big(blob)) - C
    return H


def _dq_oracle(blob, q, qd, tau):
    from test_gpu_parity import _reference_plus_on_manifold

    m = parse_clusters(blob)
    B, nv, h = q.shape[0], qd.shape[1], 1e-6
    out = np.empty((B, nv, nv))
    for b in range(B):
        for k in range(nv):
            qp = _reference_plus_on_manifold(blob, m, q[b], k, +h)[None]
            qm = _reference_plus_on_manifold(blob, m, q[b], k, -h)[None]
            out[b, :, k] = (O.forward_dynamics(blob, qp, qd[b:b + 1], tau[b:b + 1])[0] - O.forward_dynamics(blob, qm, qd[b:b + 1], tau[b:b + 1])[0]) / (2 * h)
    return out


# ---- the cases: (id, model, plan-time switches, B, entry point) -------------------------------------------------------------------
# Entry point: call(plan, x) -> tuple of output tensors, where x holds device tensors "q", "qd", "tau", "fext", "force";
# check(blob, s, outs, tol) compares the numpy outputs `outs` of the states `s` (a dict of numpy inputs) with the oracle.
def _aba(plan, x):
    return (plan.forward_dynamics(x["q"], x["qd"], x["tau"]),)


def _aba_fext(plan, x):
    return (plan.forward_dynamics(x["q"], x["qd"], x["tau"], f_ext=x["fext"]),)


def _rnea(plan, x):
    return (plan.inverse_dynamics(x["q"], x["qd"], x["tau"]),)


def _rnea_fext(plan, x):
    return (plan.inverse_dynamics(x["q"], x["qd"], x["tau"], f_ext=x["fext"]),)


def _chk_aba(blob, s, o, tol, fext=False):
    assert _rel(o[0], O.forward_dynamics(blob, s["q"], s["qd"], s["tau"], s["fext"] if fext else None, big=_big(blob))) < tol


def _chk_rnea(blob, s, o, tol, fext=False):
    assert _rel(o[0], O.inverse_dynamics(blob, s["q"], s["qd"], s["tau"], s["fext"] if fext else None, big=_big(blob))) < tol


def _chk_bias(blob, s, o, tol):
    assert _rel(o[0], O.inverse_dynamics(blob, s["q"], s["qd"], np.zeros_like(s["qd"]))) < tol


def _chk_mass(blob, s, o, tol):
    assert _rel(o[0], _mass_oracle(blob, s["q"])) < tol


def _chk_dtau(blob, s, o, tol):
    assert _rel(o[0], _fd_columns(blob, s["q"], s["qd"], s["tau"], "dtau")) < max(tol, 1e-8)


def _chk_dqd(blob, s, o, tol):
    assert _rel(o[0], _fd_columns(blob, s["q"], s["qd"], s["tau"], "dqd")) < max(tol, 1e-8)


def _chk_dq(blob, s, o, tol):
    assert _rel(o[0], _dq_oracle(blob, s["q"], s["qd"], s["tau"])) < max(tol, 2e-5)


def _chk_derivs(blob, s, o, tol):
    _chk_dq(blob, s, o[0:1], tol)
    _chk_dqd(blob, s, o[1:2], tol)
    _chk_dtau(blob, s, o[2:3], tol)


def _chk_poses(blob, s, o, tol):
    nb = o[0].shape[1]
    assert _rel(o[0].reshape(len(s["q"]), -1), O.body_poses(blob, s["q"], nb).reshape(len(s["q"]), -1)) < tol


def _chk_force(blob, s, o, tol):
    # applyTestForce at OFFSET on FORCE_BODY: dstate = FD with the force applied - FD without (zero velocity and torque)
    nb, B, body = s["fext"].shape[1], len(s["q"]), _body_index(blob, FORCE_BODY)
    lam, ds = o
    Xa = O.body_poses(blob, s["q"], nb)[:, body]
    E, r = Xa[:, :9].reshape(B, 3, 3), Xa[:, 9:]
    fe = np.zeros((B, nb, 6))
    fe[:, body, :3] = np.cross(r + np.einsum("bji,j->bi", E, OFFSET), s["force"])
    fe[:, body, 3:] = s["force"]
    z = np.zeros_like(s["qd"])
    ds_ref = O.forward_dynamics(blob, s["q"], z, z, fe) - O.forward_dynamics(blob, s["q"], z, z)
    jtf = O.inverse_dynamics(blob, s["q"], z, z) - O.inverse_dynamics(blob, s["q"], z, z, fe)
    assert _rel(ds, ds_ref) < max(tol, 1e-8)
    assert np.abs(lam.reshape(-1) - np.einsum("bi,bi->b", jtf, ds_ref)).max() / (1 + np.abs(lam).max()) < max(tol, 1e-8)


def _chk_twists(blob, s, o, tol):
    # v and a apart, every state on its own scale: a wrong state, or a term that is small next to the batch's largest |a|, cannot hide.
    # The call feeds x["tau"] as ydd, so the reference does.
    err = K.block_errors(o[0], K.body_twists(blob, s["q"], s["qd"], s["tau"], big=_big(blob)))
    assert err.max() < tol, f"state {int(err.max(axis=1).argmax())}: v {err[:, 0].max():.2e}, a {err[:, 1].max():.2e} against {tol:.0e}"


def _osim_frames(blob):
    return [_body_index(blob, b) for b in OSIM_BODIES], [OFFSET, (0.0, 0.0, 0.0)]


def _chk_osim(blob, s, o, tol, frames=None):
    # frames: (bodies, offsets) of the call, the table's when None.  J against the numpy recursion's frame Jacobians: the identity below
    # has the kernel's own J on both sides, and passes a frame on the wrong body or a dropped offset
    Linv, J = o
    J_ref = K.frame_jacobians(blob, s["q"], *(frames or _osim_frames(blob)), big=_big(blob))
    assert _rel(J, J_ref) < max(tol, 1e-9)
    # Linv = J H^-1 J^T, H^-1 from the oracle's forward dynamics (columns of d ydd / d tau)
    Hinv = _fd_columns(blob, s["q"], np.zeros_like(s["qd"]), np.zeros_like(s["qd"]), "dtau")
    assert _rel(Linv, np.einsum("bij,bjk,blk->bil", J, Hinv, J)) < max(tol, 1e-8)


def _chk_project(blob, s, o, tol):
    q_ref, ok_ref = O.project_positions(blob, s["q_start"])
    got, ok = o
    both = ok.astype(bool) & ok_ref
    assert both.any()
    assert np.abs(got[both] - q_ref[both]).max() < (1e-7 if tol < 1e-6 else 1e-3)


def _chk_spanning(blob, s, o, tol):
    assert _rel(o[0], O.spanning_state(blob, s["q"], s["qd"])[1]) < max(tol, 1e-10)
    # qdd_span = G ydd + g (the call feeds x["tau"] as ydd), at the bound test_spanning_recovery_matches_oracle holds the implicit bias to
    ref = K.spanning_rates(blob, s["q"], s["qd"], s["tau"], big=_big(blob))[1]
    g = ref - K.spanning_rates(blob, s["q"], np.zeros_like(s["qd"]), s["tau"], big=_big(blob))[1]
    assert np.abs(o[1] - ref).max() < max(tol, 1e-8) * (1 + np.abs(g).max())


def _chk_indep(blob, s, o, tol):
    # engine coordinates in, engine coordinates out: valid states come back unchanged
    q, qd, status = o
    assert (status == 0).all()
    assert np.abs(q - s["q"]).max() < (1e-12 if tol < 1e-6 else 1e-6) and np.abs(qd - s["qd"]).max() < (1e-12 if tol < 1e-6 else 1e-6)


OFFSET = (0.05, -0.02, 0.1)
# contact frames on links, not rotors: a frame on a rotor sends the inverse OSIM and applyTestForce from the force-propagation kernel
# (capi.cpp, choose_osim) to the unit-wrench route (Mini Cheetah)
FORCE_BODY = "FL_knee_link"
OSIM_BODIES = ("FR_knee_link", "FL_knee_link")


def _body_index(blob, name):
    from test_gpu_parity import _body_index as index

    return index(blob, name)


def _test_force(plan, x):
    return plan.apply_test_force(x["q"], _body_index(plan.blob, FORCE_BODY), OFFSET, x["force"])


def _inv_osim(plan, x):
    return plan.inv_osim(x["q"], *_osim_frames(plan.blob), with_jacobian=True)


def _project(plan, x):
    # (in place: the input is refilled from q_start inside the captured call, so every replay starts from the same positions)
    x["q_proj"].copy_(x["q_start"])
    return x["q_proj"], plan.project_positions(x["q_proj"])


# ---- the entry points added after the table: inverse-dynamics derivatives, time stepping, contacts, centroidal quantities -------------
# Their checkers reuse references the CPU suite pins to the oracle (id_derivative_refs, integrate_ref, contact_ref, impulse_ref, centroidal_ref); those
# modules import this one, so they are imported where they are used.
T_ROLL = 3  # steps of the rollout row
# the contact set of a model's contact rows (contact_ref.SETS); every other model: one point, OFFSET, on its last link
CONTACT_SETS = {"urdf_mini_cheetah": "cheetah_feet", "tello_with_arms": "tello_feet", "urdf_mit_humanoid": "humanoid_soles"}
DAMPING = 1e-3  # of the redundant eight-contact set, as test_contact_gpu.py runs it
# time steps of the integrate / step / rollout rows where integrate_ref.dt_of(model) fails the 95 % condition on a draw of the table
# (test_entry_draws_cpu.py asserts the condition for every draw): none does -- the four-bar's reference accepts every state of every
# draw at integrate_ref.DT's 0.05 (measured shares: 100 % for seeds 1, 2, 3, 4, 11, 21, 100 .. 103, fp64 and fp32-rounded inputs)
DT_HALVED = {}
# (No fp32 row needs an allowance against the float32 run of the reference: every new row holds TOL32 on the MI355X on every draw of the
# four files, tello_with_arms' kinetic energy included -- worst 2.5e-6 on the scale 1 + |ref| of centroidal_ref.scale_error.)


def _held(blob, tol, what, err, bound):
    err = float(err)
    print(f"HELD {_name(blob)} {'f64' if tol < 1e-6 else 'f32'} {what}: {err:.2e} of {bound:.1e}")
    assert err < bound, f"{what}: {err:.2e} against {bound:.1e}"


@functools.lru_cache(maxsize=None)
def _contacts(blob):
    """(bodies, offsets) of the contact rows of the model `blob`"""
    import contact_ref

    key = CONTACT_SETS.get(_name(blob))
    if key is not None:
        return tuple(contact_ref.contact_set(key)[1:])
    from test_contact_gpu import _last_link

    return [_last_link(blob)], [OFFSET]


def _dt(blob):
    import integrate_ref

    return DT_HALVED.get(_name(blob), integrate_ref.dt_of(_name(blob)))


def _is64(t):
    return t.dtype.itemsize == 8


def _id_derivs(plan, x):
    return tuple(plan.id_derivatives(x["q"], x["qd"], x["tau"]).values())  # (dq, dqd, dydd; the table feeds tau as ydd)


def _chk_id_derivs(blob, s, o, tol, ref=None):
    """ref: id_derivative_refs.oracle_refs of the states, where the caller has them already (test_gravity_gpu.py: one evaluation for
    both precisions)"""
    from id_derivative_refs import oracle_refs

    ref = ref or oracle_refs(blob, {"q": s["q"], "qd": s["qd"], "ydd": s["tau"]})
    for k, got, floor in (("dydd", o[2], 1e-9), ("dqd", o[1], 1e-8), ("dq", o[0], 2e-5)):  # the bounds of test_id_derivatives_gpu.py
        _held(blob, tol, "id_derivatives " + k, _rel(got, ref[k]), max(tol, floor))


def _integrate(plan, x):
    import integrate_ref
    import test_integrate_gpu

    # (the table feeds tau as ydd; the projection's tolerance per type as test_integrate_gpu.py passes it)
    return plan.integrate(x["q"], x["qd"], x["tau"], _dt(plan.blob), tol=integrate_ref.TOL if _is64(x["q"]) else test_integrate_gpu.TOL32)


def _hold_step(blob, tol, what, q, qd, ydd, got, flags=True):
    """(q', qd', ok) of one step from (q, qd) with the acceleration ydd against integrate_ref.reference_step on the states the reference
    accepts, by the rules and bounds of test_integrate_gpu.py: fp64 at 1e-9, quaternion up to sign; fp32 qd', explicit and independent
    coordinates at 16 eps32 max(1, |ref|), quaternion at 32 eps32, dependent coordinates at 1e-3 on the gated states; ok equals the
    reference's flag except within a factor 10 of either tolerance (flags=False: the caller cannot hold ok -- step in fp32)."""
    import integrate_ref as R
    import test_integrate_gpu as TI

    qn, vn, ok = got
    rq, rv, rok, phi = R.reference_step(blob, q, qd, ydd, _dt(blob), big=_big(blob))
    assert rok.any(), f"{what}: the reference accepts none of the {len(rok)} states: nothing was compared"
    kinds = R.column_kinds(blob)
    qn = TI.quat_sign_aligned(qn, rq, kinds)
    assert np.isfinite(qn[rok]).all() and np.isfinite(vn[rok]).all()
    if tol < 1e-6:
        _held(blob, tol, what + " q'", np.abs(qn - rq)[rok].max(), 1e-9)
        _held(blob, tol, what + " qd'", np.abs(vn - rv)[rok].max(), 1e-9)
        if flags:
            TI.check_flags(ok, rok, phi, R.TOL, what)
        return
    eps = TI.EPS32
    _held(blob, tol, what + " qd' / (16 eps max(1, |ref|))", (np.abs(vn - rv) / (16 * eps * np.maximum(1.0, np.abs(rv))))[rok].max(), 1.0 + 1e-12)
    plain, quat, dep = (kinds == "pos") | (kinds == "ind"), kinds == "quat", kinds == "dep"
    if plain.any():
        _held(blob, tol, what + " plain q' / (16 eps max(1, |ref|))",
              (np.abs(qn - rq) / (16 * eps * np.maximum(1.0, np.abs(rq))))[np.ix_(rok, plain)].max(), 1.0 + 1e-12)
    if quat.any():
        _held(blob, tol, what + " quaternion / eps", np.abs(qn - rq)[np.ix_(rok, quat)].max() / eps, 32.0 + 1e-9)
    if dep.any():
        gated = rok & R.gate(blob, q, qd) & R.gate(blob, rq, rv)
        assert gated.any(), f"{what}: no state passes the conditioning gate before and after the step"
        _held(blob, tol, what + " dependent q'", np.abs(qn - rq)[np.ix_(gated, dep)].max(), TI.TOL32 * (1 + 1e-12))
        if flags:
            unsure = ((phi > R.TOL / 10) & (phi < R.TOL * 10)) | ((phi > TI.TOL32 / 10) & (phi < TI.TOL32 * 10))
            bad = (ok.astype(bool) != rok) & ~unsure & gated
            assert not bad.any(), f"{what}: ok differs from the reference on gated states {np.nonzero(bad)[0][:8]}"
    elif flags:
        assert ok.all()


def _chk_integrate(blob, s, o, tol):
    _hold_step(blob, tol, "integrate", s["q"], s["qd"], s["tau"], o)


def _hold_dynamics_step(blob, tol, what, q, qd, ydd_ref, got, flags=True):
    """(q', qd', ok) of a step whose acceleration the DEVICE computed, against reference_step fed the oracle's ydd_ref.  qd' = qd + dt ydd
    carries dt times the error of ydd, which the table bounds by tol (1 + max |ydd|); q' moves by dt qd' through maps of gain about one
    (a rotation, unit rows of G, rows of G inside the conditioning gate).  So both are held at tol on the scale 1 + max |ref| + dt max |ydd|,
    on the states the reference accepts; ok in fp64 by the rule of test_integrate_gpu.py, in fp32 on models without implicit clusters
    (all true) -- grbda_step_* passes the reference's 1e-8 to the projection, which fp32 cannot reach, so its fp32 flag says nothing."""
    import integrate_ref as R
    import test_integrate_gpu as TI

    qn, vn, ok = got
    rq, rv, rok, phi = R.reference_step(blob, q, qd, ydd_ref, _dt(blob), big=_big(blob))
    assert rok.any(), f"{what}: the reference accepts none of the {len(rok)} states: nothing was compared"
    kinds = R.column_kinds(blob)
    qn = TI.quat_sign_aligned(qn, rq, kinds)
    assert np.isfinite(qn[rok]).all() and np.isfinite(vn[rok]).all()
    scale = 1.0 + max(np.abs(rq[rok]).max(), np.abs(rv[rok]).max()) + _dt(blob) * np.abs(ydd_ref[rok]).max()
    _held(blob, tol, what + " q'", np.abs(qn - rq)[rok].max() / scale, tol)
    _held(blob, tol, what + " qd'", np.abs(vn - rv)[rok].max() / scale, tol)
    if flags and tol < 1e-6:
        TI.check_flags(ok, rok, phi, R.TOL, what)
    elif flags and not ((kinds == "ind") | (kinds == "dep")).any():
        assert ok.all()
    return rq, rv, rok


def _chk_step(blob, s, o, tol, fext=False):
    qn, vn, ydd, ok = o
    ref = O.forward_dynamics(blob, s["q"], s["qd"], s["tau"], s["fext"] if fext else None, big=_big(blob))
    _held(blob, tol, "step ydd", _rel(ydd, ref), tol)
    _hold_dynamics_step(blob, tol, "step", s["q"], s["qd"], ref, (qn, vn, ok))


def _rollout(plan, x):
    # (per-step torques [T, B, nv] from the table's [B, T, nv]; the recorded trajectories come back with the batch in front)
    qT, vT, ok, qt, vt = plan.rollout(x["q"], x["qd"], x["tau_T"].transpose(0, 1).contiguous(), _dt(plan.blob), T_ROLL, record=True)
    return qt.transpose(0, 1), vt.transpose(0, 1), ok


def _chk_rollout(blob, s, o, tol):
    """T_ROLL reference steps of the oracle's forward dynamics, every recorded state held.  fp64: the chain of reference steps from the
    inputs.  fp32: each recorded state against ONE reference step from the device's own previous recorded state (exact in float64) --
    a chain would charge the kernel with the growth of a 1e-3 difference through d ydd / d q over dt = 0.25, which is the dynamics'."""
    qt, vt, ok = o
    q, qd = s["q"], s["qd"]
    for k in range(T_ROLL):
        ydd = O.forward_dynamics(blob, q, qd, s["tau_T"][:, k], big=_big(blob))
        q, qd, _ = _hold_dynamics_step(blob, tol, f"rollout state {k + 1}", q, qd, ydd, (qt[:, k], vt[:, k], ok), flags=False)
        if tol > 1e-6:
            q, qd = qt[:, k], vt[:, k]
    assert ok.all()  # (the AND over the steps; the row's model has no implicit cluster, so the reference accepts every state)


def _contact_points(plan, x):
    return plan.contact_points(x["q"], *_contacts(plan.blob), qd=x["qd"], ydd=x["tau"])  # (the table feeds tau as ydd)


def _chk_contact_points(blob, s, o, tol):
    import contact_ref as C

    ref = C.contact_points(blob, s["q"], *_contacts(blob), s["qd"], s["tau"])
    for what, got, r in zip(("pos", "vel", "acc"), o, ref):
        _held(blob, tol, "contact_points " + what, C.rel_per_state(got, r).max(), tol)


def _contact_dynamics(plan, x, damped=False):
    return plan.contact_dynamics(x["q"], x["qd"], x["tau"], *_contacts(plan.blob), a_des=x["a_des"], damping=DAMPING if damped else 0.0,
                                 f_ext=x["fext"] if damped else None)


def _chk_contact_dynamics(blob, s, o, tol, damped=False):
    import contact_ref as C

    ref = C.contact_dynamics(blob, s["q"], s["qd"], s["tau"], *_contacts(blob), s["a_des"], DAMPING if damped else 0.0, s["fext"] if damped else None)
    for what, got, key in (("ydd", o[0], "ydd"), ("lambda", o[1], "lam"), ("ydd_free", o[2], "ydd_free")):
        _held(blob, tol, "contact_dynamics " + what, C.rel_per_state(got, ref[key]).max(), tol)


RESTITUTION = 0.25  # of the contact_impulse rows


def _contact_impulse(plan, x):
    return plan.contact_impulse(x["q"], x["qd"], *_contacts(plan.blob), v_des=x["v_des"], restitution=RESTITUTION)


def _chk_contact_impulse(blob, s, o, tol):
    """qd_next and impulse against impulse_ref, every state on its own scale: fp64 at TOL64; fp32 by the rule of
    test_impulse_gpu.py::test_contact_impulse_fp32 -- TOL32, or that file's MARGINS32 for the contact set where it lists one -- with the
    closed form carried out in float32 (that file's yardstick) printed beside each figure"""
    import contact_ref as C
    import impulse_ref as I

    ref = I.contact_impulse(blob, s["q"], s["qd"], *_contacts(blob), s["v_des"], RESTITUTION, 0.0)
    bound, yard = tol, None
    if tol > 1e-6:
        from test_impulse_gpu import MARGINS32

        bound = MARGINS32.get(CONTACT_SETS.get(_name(blob)), (tol,))[0]
        yard = I.contact_impulse_in(np.float32, ref, s["qd"], s["v_des"], RESTITUTION, 0.0)
    for i, (what, key) in enumerate((("qd_next", "qd_next"), ("impulse", "impulse"))):
        assert np.isfinite(o[i]).all(), f"contact_impulse {what}: not finite"
        note = "" if yard is None else f" (the closed form in float32: {C.rel_per_state(yard[i].astype(np.float64), ref[key]).max():.2e})"
        _held(blob, tol, f"contact_impulse {what}{note}", C.rel_per_state(o[i], ref[key]).max(), bound)


def _hold_centroidal(blob, s, tol, entry, names, outs, ydd):
    import centroidal_ref as C

    ref = C.centroidal(blob, s["q"], s["qd"], ydd, big=_big(blob))
    for k, got in zip(names, outs):
        _held(blob, tol, f"{entry} {k}", C.scale_error(got, ref[k]).max(), tol)


def _chk_energy(blob, s, o, tol):
    _hold_centroidal(blob, s, tol, "energy", ("kinetic", "potential"), o, None)


def _chk_centroidal(blob, s, o, tol):
    _hold_centroidal(blob, s, tol, "centroidal", ("com", "com_vel", "h", "hdot"), o, s["tau"])  # (the call feeds tau as ydd)


def _chk_centroidal_matrix(blob, s, o, tol):
    import centroidal_ref as C

    _held(blob, tol, "centroidal_matrix A", C.scale_error(o[0], C.momentum_matrix(blob, s["q"], big=_big(blob))).max(), tol)


ENTRY = {
    "aba": (_aba, _chk_aba),
    "aba_fext": (_aba_fext, lambda b, s, o, t: _chk_aba(b, s, o, t, True)),
    "rnea": (_rnea, _chk_rnea),
    "rnea_fext": (_rnea_fext, lambda b, s, o, t: _chk_rnea(b, s, o, t, True)),
    "bias": (lambda p, x: (p.bias_force(x["q"], x["qd"]),), _chk_bias),
    "mass_matrix": (lambda p, x: (p.mass_matrix(x["q"]),), _chk_mass),
    "fd_dtau": (lambda p, x: (p.fd_dtau(x["q"]),), _chk_dtau),
    "fd_dqd": (lambda p, x: (p.fd_dqd(x["q"], x["qd"], x["tau"]),), _chk_dqd),
    "fd_dq": (lambda p, x: (p.fd_dq(x["q"], x["qd"], x["tau"]),), _chk_dq),
    "fd_derivatives": (lambda p, x: tuple(p.fd_derivatives(x["q"], x["qd"], x["tau"]).values()), _chk_derivs),
    "body_poses": (lambda p, x: (p.body_poses(x["q"]),), _chk_poses),
    # (twists: no oracle entry point; the numpy recursion of kinematics_ref.py, pinned to the oracle's inverse dynamics on the CPU)
    "body_twists": (lambda p, x: (p.body_twists(x["q"], x["qd"], x["tau"]),), _chk_twists),
    "apply_test_force": (_test_force, _chk_force),
    "inv_osim": (_inv_osim, _chk_osim),
    "project_positions": (lambda p, x: _project(p, x), _chk_project),
    # (fp32 states sit within rounding of the manifold, not within 1e-8)
    "state_to_independent": (lambda p, x: p.state_to_independent(x["q"], x["qd"], tol=1e-8 if x["q"].dtype.itemsize == 8 else 1e-3), _chk_indep),
    "spanning": (lambda p, x: p.spanning(x["q"], x["qd"], x["tau"]), _chk_spanning),
    "id_derivatives": (_id_derivs, _chk_id_derivs),
    "integrate": (_integrate, _chk_integrate),
    "step": (lambda p, x: p.step(x["q"], x["qd"], x["tau"], _dt(p.blob)), _chk_step),
    "step_fext": (lambda p, x: p.step(x["q"], x["qd"], x["tau"], _dt(p.blob), f_ext=x["fext"]), lambda b, s, o, t: _chk_step(b, s, o, t, True)),
    "rollout": (_rollout, _chk_rollout),
    "contact_points": (_contact_points, _chk_contact_points),
    "contact_dynamics": (_contact_dynamics, _chk_contact_dynamics),
    "contact_dynamics_damped_fext": (lambda p, x: _contact_dynamics(p, x, True), lambda b, s, o, t: _chk_contact_dynamics(b, s, o, t, True)),
    "contact_impulse": (_contact_impulse, _chk_contact_impulse),
    "energy": (lambda p, x: p.energy(x["q"], x["qd"]), _chk_energy),
    "centroidal": (lambda p, x: tuple(p.centroidal(x["q"], x["qd"], x["tau"]).values()), _chk_centroidal),
    "centroidal_matrix": (lambda p, x: (p.centroidal_matrix(x["q"]),), _chk_centroidal_matrix),
}

CASES = []
for _ep in ("aba", "aba_fext", "rnea", "rnea_fext"):
    CASES += [("chain", "urdf_mini_cheetah", {}, B_CHAIN, _ep), ("latency", "urdf_mini_cheetah", {}, 300, _ep),
              ("interpreter", "urdf_mit_humanoid", {"GRBDA_NO_CHAIN": "1"}, 1000, _ep), ("gen1", "urdf_four_bar", {}, 1000, _ep),
              ("spanning_tree", "parallel_chain_exp_d10_l16", {}, 300, _ep), ("two_parent", "two_parent", {}, 300, _ep)]
CASES += [("crba", "urdf_mini_cheetah", {}, B_CHAIN, "mass_matrix"), ("no_crba", "urdf_mini_cheetah", {"GRBDA_NO_CRBA": "1"}, 1000, "mass_matrix"),
          ("chain", "urdf_mini_cheetah", {}, B_CHAIN, "bias"), ("chain", "urdf_mini_cheetah", {}, 1000, "fd_dtau"),
          ("chain", "urdf_mini_cheetah", {}, 1000, "fd_dqd"), ("chain", "urdf_mini_cheetah", {}, 1000, "fd_dq"),
          ("minv", "urdf_mini_cheetah", {}, 1001, "fd_derivatives"), ("dense", "urdf_mini_cheetah", {"GRBDA_NO_MINV": "1"}, 1001, "fd_derivatives"),
          ("manifold", "tello", {}, 301, "fd_derivatives"), ("manifold", "urdf_four_bar", {}, 301, "fd_dq"),
          ("chain", "urdf_mini_cheetah", {}, B_CHAIN, "body_poses"), ("chain", "urdf_mini_cheetah", {}, B_CHAIN, "body_twists"),
          ("chain", "urdf_mini_cheetah", {}, 1000, "apply_test_force"), ("chain", "urdf_mini_cheetah", {}, 1000, "inv_osim"),
          ("no_efpa", "urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, 300, "inv_osim"),
          ("implicit", "urdf_four_bar", {}, 1000, "project_positions"), ("implicit", "urdf_four_bar", {}, 1000, "state_to_independent"),
          ("implicit", "urdf_four_bar", {}, 1000, "spanning"), ("spanning_tree", "parallel_chain_exp_d10_l16", {}, 300, "mass_matrix")]
# twists on the routes the Mini Cheetah row does not reach: implicit differentials, a loop cluster, big clusters, a roll-pitch-yaw base
CASES += [("implicit", "tello_with_arms", {}, 300, "body_twists"), ("implicit", "urdf_four_bar", {}, 300, "body_twists"),
          ("spanning_tree", "parallel_chain_exp_d10_l16", {}, 300, "body_twists"), ("chain", "urdf_mini_cheetah_rpy", {}, 300, "body_twists")]
# the entry points added after the table, B = 300: small, ragged, more than four tiles and below every route threshold
CASES += [("analytic", "urdf_mini_cheetah", {}, 300, "id_derivatives"), ("manifold", "urdf_four_bar", {}, 300, "id_derivatives"),
          ("quaternion", "urdf_mini_cheetah", {}, 300, "integrate"), ("newton", "urdf_four_bar", {}, 300, "integrate"),
          ("explicit", "urdf_mini_cheetah", {}, 300, "step"), ("interpreter", "urdf_mini_cheetah", {}, 300, "step_fext"),
          ("newton", "urdf_four_bar", {}, 300, "step"), ("explicit", "urdf_mini_cheetah", {}, 300, "rollout"),
          ("feet", "urdf_mini_cheetah", {}, 300, "contact_points"), ("feet", "tello_with_arms", {}, 300, "contact_points"),
          ("spanning_tree", "parallel_chain_exp_d10_l16", {}, 300, "contact_points"),
          ("efpa", "urdf_mini_cheetah", {}, 300, "contact_dynamics"), ("no_efpa", "urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, 300, "contact_dynamics"),
          ("feet", "tello_with_arms", {}, 300, "contact_dynamics"), ("soles", "urdf_mit_humanoid", {}, 300, "contact_dynamics_damped_fext")]
for _ep in ("energy", "centroidal"):
    CASES += [("explicit", "urdf_mit_humanoid", {}, 300, _ep), ("implicit", "tello_with_arms", {}, 300, _ep),
              ("spanning_tree", "parallel_chain_exp_d10_l16", {}, 300, _ep)]
CASES += [("explicit", "urdf_mit_humanoid", {}, 300, "centroidal_matrix"), ("implicit", "tello_with_arms", {}, 300, "centroidal_matrix")]
# contact impulses on the contact sets of the contact_dynamics rows: both routes of the inverse OSIM on the Mini Cheetah, implicit clusters
CASES += [("efpa", "urdf_mini_cheetah", {}, 300, "contact_impulse"), ("feet", "tello_with_arms", {}, 300, "contact_impulse"),
          ("no_efpa", "urdf_mini_cheetah", {"GRBDA_NO_EFPA": "1"}, 300, "contact_impulse")]
IDS = [f"{ep}-{route}-{model}-B{B}" for route, model, env, B, ep in CASES]
assert len(set(IDS)) == len(IDS)
# (entry point, model, type) that no file runs, with the reason
NOT_RUN = {
    ("contact_dynamics_damped_fext", "urdf_mit_humanoid", "f32"): "test_contact_gpu.py bounds cond(A) for fp32 on the Mini Cheetah's and Tello's feet only: "
                                                                  "the eight-contact set is rank 12 of 24 and stands on its damping",
}
# the table by number type: what the four files are parametrised over
TYPED = [(c, dt) for c in CASES for dt in ("f64", "f32") if (c[4], c[1], dt) not in NOT_RUN]
TYPED_IDS = [f"{ep}-{route}-{model}-B{B}-{dt}" for (route, model, env, B, ep), dt in TYPED]


@functools.lru_cache(maxsize=8)
def _host_inputs(blob, n_bodies, B, seed, dtype, max_cond=None):
    """the numpy inputs of B states, rounded to `dtype` (the fp32 oracle inputs are the rounded ones); shared, so never written to"""
    import torch

    q, qd, tau = _states(blob, B, seed, max_cond)
    rng = np.random.default_rng(seed)
    s = {"q": q, "qd": qd, "tau": tau, "fext": rng.uniform(-1, 1, (B, n_bodies, 6)), "force": rng.uniform(-1, 1, (B, 3))}
    # projection input: the states moved off the manifold by a little (Newton has something to do)
    s["q_start"] = q + rng.uniform(-0.05, 0.05, q.shape)
    # what the later entry points need, drawn after every key above and from a generator of their own: q, qd, tau, fext, force and q_start
    # keep their bits for every row that was here before.  a_des: one acceleration per contact of the model's contact set; tau_T: the
    # rollout's per-step torques, batch in front like every key (the ladder takes the first B rows of each)
    rng2 = np.random.default_rng([seed, 20250])
    s["a_des"] = rng2.uniform(-1, 1, (B, len(_contacts(blob)[0]), 3))
    s["tau_T"] = tau[:, None, :] * rng2.uniform(0.4, 1.0, (B, T_ROLL, 1))
    # v_des: one velocity per contact for contact_impulse, after every key above and from a generator of its own again
    s["v_des"] = np.random.default_rng([seed, 20251]).uniform(-1, 1, (B, len(_contacts(blob)[0]), 3))
    s = {k: np.asarray(torch.as_tensor(v, dtype=dtype).double()) for k, v in s.items()}
    return s


def _inputs(blob, plan, B, seed, dtype, gpu, max_cond=None):
    import torch

    s = dict(_host_inputs(blob, plan.n_bodies, B, seed, dtype, max_cond))
    x = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=dtype, device=gpu) for k, v in s.items()}
    x["q_proj"] = x["q_start"].clone()
    return s, x


def _host(outs):
    return [o.detach().cpu().double().numpy() if o.is_floating_point() else o.detach().cpu().numpy() for o in outs]


# ---- guarded calls: what test_buffer_edges_gpu.py and test_batch_ladder_gpu.py share ---------------------------------------------------
# Entry points whose checker differentiates the oracle along the constraint manifold.  When EVERY state of a draw is held to the
# reference's 2e-5, the draw bounds cond(K_d) of the implicit loops as the derivative tests of test_gpu_parity.py do (models.py,
# valid_states: a state that satisfies phi to 1e-12 sits 1e-12 / sigma_min off the manifold, and the difference quotient along the
# manifold then differs from the exact derivative at the state; measured on the four-bar, fp64: 1.2e-4 at cond 422, 8e-6 at 325,
# 1.5e-6 at 150 and below).  Explicit models are not affected by the bound.  id_derivatives differentiates the inverse dynamics the same way.
DIFFERENTIATES = ("fd_dq", "fd_derivatives", "id_derivatives")


def draw_bound(entry):
    return 100.0 if entry in DIFFERENTIATES else None


TILE = 64  # states per tile of the tiled kernels (one wavefront); the derivative pipeline packs groups of 4 states


def edge_states(B, n_random=4, seed=0):
    """sorted states to hold against the oracle: 0, B - 1, the first and the last state of the last tile and of the last group of four,
    and a seeded few"""
    idx = {0, B - 1, ((B - 1) // TILE) * TILE, ((B - 1) // 4) * 4}
    idx |= set(np.random.default_rng(seed).choice(B, min(B, n_random), replace=False).tolist())
    return np.array(sorted(idx))


def _owned_by_projection(blob):
    """columns of q that project_positions may change: the dependent positions of the implicit clusters"""
    m = parse_clusters(blob)
    own = np.zeros(m["nq"], dtype=bool)
    for c in m["clusters"]:
        qi, nsv, ctype, io = c[3], c[8], c[9], c[11]
        if ctype in (2, 3):
            flags = m["ints"][io + 1: io + 1 + nsv] if ctype == 2 else m["ints"][io: io + nsv]
            for j in range(nsv):
                own[qi + j] = not flags[j]
    return own


def run_guarded(plan, call, s, dtype, gpu, lead, out_arena=None):
    """call(plan, x) with every input and every output in an arena of guarded.py (alignment `lead`).  Asserts: every output arena has
    both bands intact and no element left unwritten; every input arena, bands included, is bit for bit what it was (project_positions'
    q: its bands and the columns it does not own); every floating-point output is finite.  Returns the outputs as numpy arrays.
    out_arena: "aba" / "rnea" -- forward / inverse dynamics again with a caller-supplied out= arena, which must give the same bits."""
    import torch

    import guarded

    x = {k: guarded.place(v, dtype, gpu, lead) for k, v in s.items()}
    x["q_proj"] = guarded.place(s["q_start"], dtype, gpu, lead)
    before = {k: guarded.snapshot(v) for k, v in x.items()}
    with guarded.guarded_outputs(lead) as made:
        outs = call(plan, x)
    torch.cuda.synchronize()
    assert made, "the call allocated no output through torch.empty"
    for i, a in enumerate(made):
        left = guarded.check(a)
        assert left == 0, f"output arena {i} {tuple(a.shape)} {a.dtype}: {left} of {a.numel()} elements never written"
    for k, v in x.items():
        if k == "q_proj":
            assert guarded.same_bits(v, before[k], 0, v.numel()), "bands of the projected q changed"
            keep = torch.as_tensor(~_owned_by_projection(plan.blob), device=gpu)
            assert torch.equal(v[:, keep].view(torch.uint8), x["q_start"][:, keep].view(torch.uint8)), "project_positions changed a column it does not own"
        else:
            assert guarded.same_bits(v, before[k]), f"input {k} changed"
    host = _host(outs)
    for i, o in enumerate(host):
        assert np.isfinite(o).all(), f"output {i}: {int((~np.isfinite(o)).sum())} non-finite values, first at {np.argwhere(~np.isfinite(o))[0]}"
    if out_arena is not None:
        out = guarded.arena(outs[0].shape, dtype, gpu, lead)
        fn = plan.forward_dynamics if out_arena == "aba" else plan.inverse_dynamics
        with guarded.guarded_outputs(lead) as none_made:
            back = fn(x["q"], x["qd"], x["tau"], out=out)
        torch.cuda.synchronize()
        assert back is out and not none_made and guarded.check(out) == 0
        assert np.array_equal(_host([out])[0], host[0]), "out= gives other bits than the allocated output"
        for k in ("q", "qd", "tau"):
            assert guarded.same_bits(x[k], before[k]), f"input {k} changed"
    return host


def same_bits_np(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)) and len(a) == len(b)


@functools.lru_cache(maxsize=None)
def plan_for(model, env):
    """the plan of `model` compiled under the plan-time switches `env` (a tuple of (name, value) pairs); the switches are read once, at
    compilation, so the environment is put back before this returns"""
    old = {k: os.environ.get(k) for k, _ in env}
    os.environ.update(dict(env))
    try:
        return G.Plan(_model(model))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
