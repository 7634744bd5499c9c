"""Host-array entry points (grbda_*_host_f64) against their device-pointer twins: the same inputs give the same bits.

A host-array entry point stages its arrays on the device, makes the device call on the null stream, waits and copies the results back
(capi.cpp, HostStage), so whatever differs from the twin is a staging fault: a buffer sized for another width, an input that was not
copied, an output read back from the wrong array or short of its tail.  B = 65 is one tile and one state: the smallest batch whose
last state lies in a second tile, where a dropped tail shows.  Two models: Mini Cheetah (explicit clusters, a floating base) and the
four-bar (one implicit cluster: state_to_independent and project_positions have something to do; the derivatives take the
constraint-manifold route; the time step projects it back onto the manifold).  The contact frames are the entry-point table's, links
of Mini Cheetah, so applyTestForce and the inverse OSIM run on that model alone.  No oracle here -- test_gpu_parity.py and the entry-point table hold the device calls against it."""
from ctypes import c_double, c_int, c_size_t, c_void_p

import numpy as np
import pytest

import generalized_rbda_amd as G
import integrate_ref
from entry_points import FORCE_BODY, OFFSET, OSIM_BODIES, _body_index, _inputs, _inv_osim, _model, _test_force, plan_for

pytestmark = pytest.mark.gpu
B = 65
MODELS = ("urdf_mini_cheetah", "urdf_four_bar")


def _c(plan, name, *args):
    G._check(getattr(G.lib(), name)(plan._h, *args))


def _p(a):
    return c_void_p(a.ctypes.data)


def _host_poses(plan, s):
    Xa = np.empty((B, plan.n_bodies, 12))
    _c(plan, "grbda_body_poses_host_f64", _p(s["q"]), _p(Xa), c_size_t(B), c_int(0))
    return [Xa]


def _host_twists(plan, s):
    V = np.empty((B, plan.n_bodies, 12))
    _c(plan, "grbda_body_twists_host_f64", _p(s["q"]), _p(s["qd"]), _p(s["tau"]), _p(V), c_size_t(B), c_int(0))
    return [V]


def _host_test_force(plan, s):
    lam, ds = np.empty(B), np.empty((B, plan.nv))
    _c(plan, "grbda_apply_test_force_host_f64", _p(s["q"]), c_int(_body_index(plan.blob, FORCE_BODY)), (c_double * 3)(*OFFSET), _p(s["force"]),
       _p(lam), _p(ds), c_size_t(B), c_int(0))
    return [lam, ds]


def _host_osim(plan, s):
    bod = (c_int * 2)(*[_body_index(plan.blob, b) for b in OSIM_BODIES])
    off = (c_double * 6)(*OFFSET, 0.0, 0.0, 0.0)  # (the frames of entry_points._inv_osim)
    Linv, J = np.empty((B, 12, 12)), np.empty((B, 12, plan.nv))
    _c(plan, "grbda_inv_osim_host_f64", _p(s["q"]), c_int(2), bod, off, _p(Linv), _p(J), c_size_t(B), c_int(0))
    return [Linv, J]


def _host_mass(plan, s):
    H = np.empty((B, plan.nv, plan.nv))
    _c(plan, "grbda_mass_matrix_host_f64", _p(s["q"]), _p(H), c_size_t(B), c_int(0))
    return [H]


def _host_derivs(plan, s):
    d = [np.empty((B, plan.nv, plan.nv)) for _ in range(3)]
    _c(plan, "grbda_fd_derivatives_host_f64", _p(s["q"]), _p(s["qd"]), _p(s["tau"]), _p(d[0]), _p(d[1]), _p(d[2]), c_size_t(B), c_int(0))
    return d


def _host_project(plan, s):
    q, ok = s["q_start"].copy(), np.empty(B, dtype=np.int32)
    _c(plan, "grbda_project_positions_host_f64", _p(q), _p(ok), c_size_t(B), c_int(50), c_double(1e-8), c_int(0))
    return [q, ok != 0]


def _host_indep(plan, s):
    q, qd = np.empty((B, plan.nq)), np.empty((B, plan.nv))
    _c(plan, "grbda_state_to_independent_host_f64", None, None, _p(s["q"]), _p(s["qd"]), _p(q), _p(qd), c_size_t(B), c_double(1e-8), c_int(0))
    return [q, qd]


def _host_id_derivs(plan, s):
    d = [np.empty((B, plan.nv, plan.nv)) for _ in range(3)]
    _c(plan, "grbda_rnea_derivatives_host_f64", _p(s["q"]), _p(s["qd"]), _p(s["tau"]), c_double(1e-6), _p(d[0]), _p(d[1]), _p(d[2]), c_size_t(B), c_int(0))
    return d


def _host_integrate(plan, s):
    qn, vn, ok = np.empty((B, plan.nq)), np.empty((B, plan.nv)), np.empty(B, dtype=np.int32)
    _c(plan, "grbda_integrate_host_f64", _p(s["q"]), _p(s["qd"]), _p(s["tau"]), c_double(s["dt"]), _p(qn), _p(vn), _p(ok), c_int(50), c_double(1e-8),
       c_size_t(B), c_int(0))
    return [qn, vn, ok != 0]


def _host_step(plan, s, fext=False):
    qn, vn, ydd, ok = np.empty((B, plan.nq)), np.empty((B, plan.nv)), np.empty((B, plan.nv)), np.empty(B, dtype=np.int32)
    _c(plan, "grbda_step_host_f64", _p(s["q"]), _p(s["qd"]), _p(s["tau"]), _p(s["fext"]) if fext else None, c_double(s["dt"]), _p(ydd), _p(qn), _p(vn),
       _p(ok), c_size_t(B), c_int(0))
    return [qn, vn, ydd, ok != 0]


def _dev_project(plan, x):
    x["q_proj"].copy_(x["q_start"])
    return x["q_proj"], plan.project_positions(x["q_proj"], max_iter=50, tol=1e-8)


# name -> (host call(plan, s) -> numpy outputs, device call(plan, x) -> tensors): s, x the same inputs as numpy arrays / device tensors,
# and "dt", the time step of the model
TWINS = {
    "aba": (lambda p, s: [p.forward_dynamics_host(s["q"], s["qd"], s["tau"])], lambda p, x: (p.forward_dynamics(x["q"], x["qd"], x["tau"]),)),
    "aba_fext": (lambda p, s: [p.forward_dynamics_host(s["q"], s["qd"], s["tau"], f_ext=s["fext"])],
                 lambda p, x: (p.forward_dynamics(x["q"], x["qd"], x["tau"], f_ext=x["fext"]),)),
    "rnea": (lambda p, s: [p.inverse_dynamics_host(s["q"], s["qd"], s["tau"])], lambda p, x: (p.inverse_dynamics(x["q"], x["qd"], x["tau"]),)),
    "body_poses": (_host_poses, lambda p, x: (p.body_poses(x["q"]),)),
    "body_twists": (_host_twists, lambda p, x: (p.body_twists(x["q"], x["qd"], x["tau"]),)),
    "apply_test_force": (_host_test_force, _test_force),
    "inv_osim": (_host_osim, _inv_osim),
    "mass_matrix": (_host_mass, lambda p, x: (p.mass_matrix(x["q"]),)),
    "fd_derivatives": (_host_derivs, lambda p, x: tuple(p.fd_derivatives(x["q"], x["qd"], x["tau"])[k] for k in ("dq", "dqd", "dtau"))),
    "rnea_derivatives": (_host_id_derivs, lambda p, x: tuple(p.id_derivatives(x["q"], x["qd"], x["tau"], step=1e-6)[k] for k in ("dq", "dqd", "dydd"))),
    "integrate": (_host_integrate, lambda p, x: p.integrate(x["q"], x["qd"], x["tau"], x["dt"], max_iter=50, tol=1e-8)),
    "step": (_host_step, lambda p, x: p.step(x["q"], x["qd"], x["tau"], x["dt"])),
    "step_fext": (lambda p, s: _host_step(p, s, True), lambda p, x: p.step(x["q"], x["qd"], x["tau"], x["dt"], f_ext=x["fext"])),
    "project_positions": (_host_project, _dev_project),
    "state_to_independent": (_host_indep, lambda p, x: p.state_to_independent(x["q"], x["qd"], tol=1e-8)[:2]),
}


CASES = [(e, m) for m in MODELS for e in TWINS if m == "urdf_mini_cheetah" or e not in ("apply_test_force", "inv_osim")]


@pytest.mark.parametrize("entry,model", CASES, ids=[f"{e}-{m}" for e, m in CASES])
def test_host_arrays_give_the_device_call_s_bits(entry, model, gpu):
    import torch

    blob = _model(model)
    plan = plan_for(model, ())
    s, x = _inputs(blob, plan, B, 21, torch.float64, gpu, max_cond=100.0)
    s = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in s.items()}
    # a fifth of the time-stepping tests' step of the model: the four-bar's projection converges and every output stays finite
    s["dt"] = x["dt"] = integrate_ref.dt_of(model) / 5
    host_call, dev_call = TWINS[entry]
    dev = [o.detach().cpu().numpy() for o in dev_call(plan, x)]
    torch.cuda.synchronize()
    host = host_call(plan, s)
    assert all(np.isfinite(h).all() for h in host)
    assert len(host) == len(dev)
    for i, (h, d) in enumerate(zip(host, dev)):
        assert h.shape == d.shape and h.dtype == d.dtype, f"output {i}: {h.shape} {h.dtype} against {d.shape} {d.dtype}"
        assert np.array_equal(h, d), f"output {i}: {int((h != d).sum())} of {h.size} elements differ from the device call's"
