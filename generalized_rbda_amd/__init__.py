"""generalized_rbda_amd -- Python plumbing over the C ABI of libgrbda_hip.so.

The product is the HIP library (``csrc/``) behind ``include/grbda_hip.h``; this package only loads it,
wraps plans, and passes torch device pointers / streams through.  There is no CPU fallback:
every dynamics call raises ``GrbdaError`` when the library or a HIP device is missing.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import byref, c_char_p, c_double, c_float, c_int, c_size_t, c_void_p

from . import modeldesc  # noqa: F401  (model-description builder)
from ._abi import (BODIES_SIGNATURES, CONTACT_STEP_SIGNATURES, JACOBIAN_PRODUCT_SIGNATURES, JACOBIAN_SIGNATURES, JVP_SIGNATURES, SIGNATURES, STEP_VJP_SIGNATURES,
                   VJP_SIGNATURES, WRENCH_SIGNATURES)

_HERE = os.path.dirname(os.path.abspath(__file__))
# GRBDA_HIP_LIB: another build of the same library (for example the parent commit's); development A/B runs only
LIB_PATH = os.environ.get("GRBDA_HIP_LIB") or os.path.join(_HERE, "libgrbda_hip.so")

# every entry point include/grbda_hip.h declares
C_ABI_SYMBOLS = list(SIGNATURES)


class GrbdaError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        super().__init__(f"grbda error {code}: {detail}")


class PlanInfo(ctypes.Structure):
    _fields_ = [("n_slots", c_int), ("n_lds_slots_f32", c_int), ("n_lds_slots_f64", c_int),
                ("lds_bytes_f32", c_size_t), ("lds_bytes_f64", c_size_t),
                ("scratch_bytes_per_wave_f32", c_size_t), ("scratch_bytes_per_wave_f64", c_size_t),
                ("flops_aba", c_double), ("flops_rnea", c_double),
                ("bytes_aba_f32", c_double), ("bytes_aba_f64", c_double),
                ("n_axisym_bodies", c_int), ("n_carry_clusters", c_int),
                ("split_aba_f32", c_int), ("split_rnea_f32", c_int), ("n_lds_slots_split_f32", c_int),
                ("chain_aba_f32", c_int), ("n_lds_slots_chain_f32", c_int), ("n_chain_segments", c_int),
                ("chain_aba_f64", c_int), ("chain_rnea_f32", c_int), ("chain_rnea_f64", c_int),
                ("analytic_derivatives", c_int), ("n_chain_differentials", c_int),
                ("latency_mode_f32", c_int), ("latency_mode_f64", c_int), ("n_chain_generic", c_int), ("spanning_tree_route", c_int)]


_lib = None


def lib() -> ctypes.CDLL:
    """Load libgrbda_hip.so (built in-tree by ``make`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GrbdaError(-3, f"{LIB_PATH} is missing: build it with `make` (there is no CPU fallback)")
    try:
        # torch bundles its own libamdhip64; load it FIRST so that this library binds to the same
        # HIP runtime instance (device pointers and streams are then shared with torch tensors)
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    # include/grbda_hip_vjp.h (an older build named by GRBDA_HIP_LIB has none of it: a call then raises AttributeError)
    # ... and include/grbda_hip_step_vjp.h, the third table, under the same rule; then grbda_hip_wrench.h, grbda_hip_jvp.h and
    # grbda_hip_bodies.h, grbda_hip_jacobians.h, grbda_hip_jacobian_products.h, and last grbda_hip_contact_step.h
    for name, (restype, argtypes) in {**VJP_SIGNATURES, **STEP_VJP_SIGNATURES, **WRENCH_SIGNATURES, **JVP_SIGNATURES, **BODIES_SIGNATURES,
                                      **JACOBIAN_SIGNATURES, **JACOBIAN_PRODUCT_SIGNATURES, **CONTACT_STEP_SIGNATURES}.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise GrbdaError(rc, (lib().grbda_last_error() or b"").decode() or lib().grbda_strerror(rc).decode())


def _suffix(dtype) -> str:
    """the precision suffix of the entry points for a torch or numpy dtype"""
    return "f32" if str(dtype).endswith("float32") else "f64"


def urdf_to_blob(paths, ori_repr: str = "quaternion") -> bytes:
    """ClusterTreeModel::buildModelFromURDF(path | vector<path>) -> model description bytes."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    arr = (c_char_p * len(paths))(*[os.fspath(p).encode() for p in paths])
    ori = 0 if ori_repr.lower().startswith("q") else 1
    need = c_size_t(0)
    _check(lib().grbda_urdf_to_blob(arr, len(paths), ori, None, 0, byref(need)))
    buf = ctypes.create_string_buffer(need.value)
    _check(lib().grbda_urdf_to_blob(arr, len(paths), ori, buf, need.value, byref(need)))
    return buf.raw[: need.value]


class _VjpMethods:
    """The vector-Jacobian products and the autograd functions of Plan (include/grbda_hip_vjp.h): kept apart from Plan's own methods as
    that header is kept apart from grbda_hip.h.  They go through Plan._call like every other method; tests/test_vjp_gpu.py holds them to
    the argument rules of the tensor methods (strided inputs, the one exception rule, a side stream)."""

    def _vjp(self, stem, last, q, qd, x, g, want, step, stream):
        names = ("q", "qd", last)
        if not any(k in want for k in names) or any(k not in names + (("ydd",) if stem == "aba_vjp" else ()) for k in want):
            raise ValueError(f'want must name at least one of "q", "qd", "{last}"' + (' and besides them only "ydd"' if stem == "aba_vjp" else " and nothing else"))
        outs = {"grad_" + k: self.nv if k in want else None for k in names}
        if stem == "aba_vjp":
            outs["ydd_out"] = self.nv if "ydd" in want else None
        got = self._call(stem, stream, dict(self._state(q, qd=qd, **{last: x}), g=(g, self.nv)), outs, ("q", "qd", last, "g", step) + tuple(outs),
                         skip_empty=True)
        return {k.replace("grad_", "").replace("ydd_out", "ydd"): o for k, o in zip(outs, got) if o is not None}

    def id_vjp(self, q, qd, ydd, g, want=("q", "qd", "ydd"), step: float = 1e-6, stream=None):
        """g^T d tau / d q, g^T d tau / d qd, g^T d tau / d ydd of the inverse dynamics at (q, qd, ydd) for the cotangent g[B, nv]
        (grbda_rnea_vjp_*): a dict of [B, nv] tensors for the names in `want`, out[b, j] = sum_i g[b, i] d tau_i / d x_j -- the rows of
        id_derivatives contracted inside the library, "q" along the tangent step of fd_dq (nv entries).  "ydd" alone runs no
        derivative recursion (H g by two inverse dynamics); `step` as in id_derivatives."""
        return self._vjp("rnea_vjp", "ydd", q, qd, ydd, g, want, step, stream)

    def fd_vjp(self, q, qd, tau, g, want=("q", "qd", "tau"), step: float = 1e-6, stream=None):
        """g^T d ydd / d q, g^T d ydd / d qd, g^T d ydd / d tau of the forward dynamics for the cotangent g[B, nv] (grbda_aba_vjp_*): a dict
        of [B, nv] tensors for the names in `want`.  mu = H^-1 g comes from two forward dynamics at zero velocity ("tau": mu itself),
        "q" and "qd" are -mu^T d tau / d (q, qd) at ydd = FD(q, qd, tau): no factorisation, no solve, no [B, nv, nv] tensor.
        "ydd" in `want` also returns that FD(q, qd, tau)."""
        return self._vjp("aba_vjp", "tau", q, qd, tau, g, want, step, stream)

    def _ad(self, forward, q, qd, x):
        if q.requires_grad and self.nq != self.nv:
            entry = "fd_vjp" if forward else "id_vjp"
            raise ValueError(f"q requires grad on a plan with nq = {self.nq} != nv = {self.nv} (a quaternion base or implicit clusters): a gradient "
                             f"along the tangent step has no unique pull-back to the nq position coordinates -- call {entry} for the tangent gradient")
        return _autograd_function(forward).apply(self, q, qd, x)

    def forward_dynamics_ad(self, q, qd, tau):
        """forward_dynamics as a differentiable torch function (the same bits); backward is fd_vjp for the inputs that require grad.  A
        gradient for q only on plans with nq == nv (fixed or roll-pitch-yaw base, explicit clusters), where the tangent step is q + dq."""
        return self._ad(True, q, qd, tau)

    def inverse_dynamics_ad(self, q, qd, ydd):
        """inverse_dynamics as a differentiable torch function (the same bits); backward is id_vjp; q as in forward_dynamics_ad."""
        return self._ad(False, q, qd, ydd)


class _StepVjpMethods:
    """The vector-Jacobian products of integrate, step and rollout and the autograd functions built on them (include/grbda_hip_step_vjp.h),
    kept apart like _VjpMethods.  Every position cotangent and gradient is [..., nv], along the tangent step of fd_dq; tangent_cotangent
    takes an ambient [..., nq] cotangent there."""

    @staticmethod
    def _wanted(want, names):
        if not want or any(k not in names for k in want):
            raise ValueError("want must name at least one of " + ", ".join(f'"{k}"' for k in names) + " and nothing else")

    @staticmethod
    def _cotangents(g_q, g_qd):
        if g_q is None and g_qd is None:
            raise ValueError("g_q and g_qd cannot both be None")

    def integrate_vjp(self, qd_next, dt: float, g_q=None, g_qd=None, want=("q", "qd", "ydd"), stream=None):
        """The cotangents (g_q, g_qd) of the state AFTER integrate pulled back to (q, qd, ydd) (grbda_integrate_vjp_*): a dict of [B, nv]
        tensors for the names in `want`.  qd_next[B, nv]: the velocities integrate / step returned; either cotangent may be None (zero).
        One kernel launch; q does not enter."""
        names = ("q", "qd", "ydd")
        self._wanted(want, names)
        self._cotangents(g_q, g_qd)
        outs = {"grad_" + k: self.nv if k in want else None for k in names}
        got = self._call("integrate_vjp", stream, dict(qd_next=(qd_next, self.nv), g_q=(g_q, self.nv), g_qd=(g_qd, self.nv)), outs,
                         ("qd_next", float(dt), "g_q", "g_qd") + tuple(outs), skip_empty=True)
        return {k: o for k, o in zip(names, got) if o is not None}

    def step_vjp(self, q, qd, tau, qd_next, dt: float, g_q=None, g_qd=None, want=("q", "qd", "tau"), step: float = 1e-6, stream=None):
        """The cotangents of the state after step(q, qd, tau, dt) pulled back to (q, qd, tau) (grbda_step_vjp_*): integrate_vjp, fd_vjp
        on its grad_ydd, and the two sums, on one stream -- a dict of [B, nv] tensors for the names in `want`.  "tau" alone runs no
        derivative recursion; `step` as in fd_vjp."""
        names = ("q", "qd", "tau")
        self._wanted(want, names)
        self._cotangents(g_q, g_qd)
        outs = {"grad_" + k: self.nv if k in want else None for k in names}
        ins = dict(self._state(q, qd=qd, tau=tau, qd_next=qd_next), g_q=(g_q, self.nv), g_qd=(g_qd, self.nv))
        got = self._call("step_vjp", stream, ins, outs, ("q", "qd", "tau", "qd_next", float(dt), "g_q", "g_qd", float(step)) + tuple(outs),
                         skip_empty=True)
        return {k: o for k, o in zip(names, got) if o is not None}

    def rollout_vjp(self, q0, qd0, tau, dt: float, q_traj, qd_traj, g_q=None, g_qd=None, want=("q", "qd", "tau"), step: float = 1e-6,
                    stream=None):
        """The cotangents of the states of rollout(q0, qd0, tau, dt, T, record=True) pulled back to (q0, qd0, tau) (grbda_rollout_vjp_*):
        the loop of step_vjp from state T to state 0, inside the library.  q_traj[T, B, nq], qd_traj[T, B, nv]: the recorded states
        1 .. T (T is read there).  g_q, g_qd: [B, nv], cotangents of state T alone, or [T, B, nv] for states 1 .. T; either may be
        None.  Returns a dict for the names in `want`: "q", "qd" [B, nv] of state 0 and "tau", shaped like tau (one tau held for all
        steps: the sum over the steps)."""
        names = ("q", "qd", "tau")
        self._wanted(want, names)
        self._cotangents(g_q, g_qd)
        T = qd_traj.shape[0] if qd_traj.dim() == 3 else 0  # (any other rank fails the shape rule below)
        per_step = lambda t: (T, "B", self.nv) if t is not None and t.dim() == 3 else self.nv
        g_shape = per_step(g_q if g_q is not None else g_qd)
        ins = dict(self._state(q0, qd0=qd0), q_traj=(q_traj, (T, "B", self.nq)), qd_traj=(qd_traj, (T, "B", self.nv)), tau=(tau, per_step(tau)),
                   g_q=(g_q, g_shape), g_qd=(g_qd, g_shape))
        outs = dict(grad_q=self.nv if "q" in want else None, grad_qd=self.nv if "qd" in want else None,
                    grad_tau=per_step(tau) if "tau" in want else None)
        got = self._call("rollout_vjp", stream, ins, outs,
                         ("q", "qd0", "q_traj", "qd_traj", "tau", T if tau.dim() == 3 else 1, float(dt), T, "g_q", "g_qd",
                          T if g_shape != self.nv else 1, float(step)) + tuple(outs), skip_empty=True)
        return {k: o for k, o in zip(names, got) if o is not None}

    def tangent_cotangent(self, q, g):
        """The pull-back of an ambient cotangent g[..., nq] of the positions q[..., nq] through the tangent step at q: [..., nv], entry i
        = <g, d plus(q, d) / d d_i at d = 0>.  Explicit coordinates: the identity; base position: R(quat) g_p, into body axes; base
        rotation: entry i = (quat x (0, e_i)) . g_quat / 2.  Plain torch operations (CPU tensors too).  Plans with implicit clusters
        raise ValueError: their tangent step re-projects the dependent coordinates."""
        import torch

        from .modeldesc import C_FREE, C_LOOP_POSITION, C_TRIG_POLY
        from .states import parse_clusters

        if tuple(q.shape) != tuple(g.shape) or q.shape[-1] != self.nq:
            raise ValueError(f"expected q[..., {self.nq}] and g of the same shape")
        out = g.new_zeros(tuple(g.shape[:-1]) + (self.nv,))
        for c in parse_clusters(self._blob)["clusters"]:
            qi, npos, vi, nvel, ctype = c[3], c[4], c[5], c[6], c[9]
            if ctype in (C_LOOP_POSITION, C_TRIG_POLY):
                raise ValueError("tangent_cotangent does not cover plans with implicit clusters")
            if ctype != C_FREE or npos != 7:  # (a roll-pitch-yaw base steps like explicit coordinates: q + dq)
                out[..., vi:vi + nvel] = g[..., qi:qi + nvel]
                continue
            e0, e1, e2, e3 = q[..., qi + 3:qi + 7].unbind(-1)
            # R(quat)^T, body axes into world axes, as integrate applies it; R g_p is its transpose times g_p
            M = torch.stack([1 - 2 * (e2 * e2 + e3 * e3), 2 * (e1 * e2 - e0 * e3), 2 * (e1 * e3 + e0 * e2),
                             2 * (e1 * e2 + e0 * e3), 1 - 2 * (e1 * e1 + e3 * e3), 2 * (e2 * e3 - e0 * e1),
                             2 * (e1 * e3 - e0 * e2), 2 * (e2 * e3 + e0 * e1), 1 - 2 * (e1 * e1 + e2 * e2)], dim=-1).reshape(tuple(q.shape[:-1]) + (3, 3))
            out[..., vi + 3:vi + 6] = (M * g[..., qi:qi + 3].unsqueeze(-1)).sum(dim=-2)
            w, v = q[..., qi + 3:qi + 4], q[..., qi + 4:qi + 7]
            gw, gv = g[..., qi + 3:qi + 4], g[..., qi + 4:qi + 7]
            out[..., vi:vi + 3] = 0.5 * (w * gv - gw * v + torch.linalg.cross(gv, v, dim=-1))
        return out

    def _step_ad_check(self, q, entry):
        if q.requires_grad and self.nq != self.nv:
            raise ValueError(f"q requires grad on a plan with nq = {self.nq} != nv = {self.nv} (a quaternion base or implicit clusters): a gradient "
                             f"along the tangent step has no unique pull-back to the nq position coordinates -- call {entry} for the tangent gradient")

    def step_ad(self, q, qd, tau, dt: float):
        """step as a differentiable torch function: (q_next, qd_next) with the bits of step; backward is step_vjp for the inputs that
        require grad, the ambient cotangent of q_next pulled back with tangent_cotangent.  A gradient for q only on plans with nq == nv."""
        self._step_ad_check(q, "step_vjp")
        return _step_autograd_function(False).apply(self, q, qd, tau, float(dt), 1)

    def rollout_ad(self, q, qd, tau, dt: float, T: int):
        """rollout(record=True) as a differentiable torch function: (q_traj[T, B, nq], qd_traj[T, B, nv]) with its bits; backward is
        rollout_vjp; q as in step_ad."""
        self._step_ad_check(q, "rollout_vjp")
        return _step_autograd_function(True).apply(self, q, qd, tau, float(dt), int(T))


class _WrenchMethods:
    """Forward and inverse dynamics with sparse body wrenches (include/grbda_hip_wrench.h): kept apart from Plan's own methods as that
    header is kept apart from grbda_hip.h.  They go through Plan._call like every other method; tests/test_wrench_gpu.py holds them to
    the argument rules of the tensor methods (strided inputs, the one exception rule, a side stream)."""

    @staticmethod
    def _wrench_list(bodies, frame):
        """the body list as the entry points take it: (n, bodies[n]), and the frame constant"""
        if frame not in ("body", "world"):
            raise ValueError('frame must be "body" or "world"')
        n = len(bodies)
        return n, (c_int * max(n, 1))(*[int(b) for b in bodies]), 0 if frame == "body" else 1

    def forward_dynamics_wrench(self, q, qd, tau, bodies, wrench, frame="body", out=None, stream=None):
        """Forward dynamics with external wrenches on a short list of bodies (grbda_aba_wrench_*; TreeModel::setExternalForces): returns
        ydd[B, nv].  bodies: up to 16 plan body indices (a body may repeat: its wrenches add); wrench[B, n, 6]: the spatial force
        [moment; force] on bodies[i], in the body's own frame at its origin (frame="body") or with the meaning of a row of f_ext
        (frame="world").  No bodies: the plain forward dynamics, wrench may be None."""
        n, arr, fr = self._wrench_list(bodies, frame)
        return self._call("aba_wrench", stream, dict(self._state(q, qd=qd, tau=tau), wrench=(wrench, (n, 6))), dict(out=self.nv),
                          ("q", "qd", "tau", n, arr, "wrench", fr, "out"), fixed=dict(out=(out, self.nv)))[0]

    def inverse_dynamics_wrench(self, q, qd, ydd, bodies, wrench, frame="body", out=None, stream=None):
        """Inverse dynamics with external wrenches on a short list of bodies (grbda_rnea_wrench_*): returns tau[B, nv]; the arguments
        of forward_dynamics_wrench."""
        n, arr, fr = self._wrench_list(bodies, frame)
        return self._call("rnea_wrench", stream, dict(self._state(q, qd=qd, ydd=ydd), wrench=(wrench, (n, 6))), dict(out=self.nv),
                          ("q", "qd", "ydd", n, arr, "wrench", fr, "out"), fixed=dict(out=(out, self.nv)))[0]

    def wrench_kernel_name(self, algo: str, dtype: str, bodies, frame: str, B: int, device: int = 0) -> str:
        """The kernel the dynamics of forward_dynamics_wrench ("aba") / inverse_dynamics_wrench ("rnea") launch for this body list
        and B states in "f32" / "f64" (grbda_wrench_kernel_name): a wrench-carrying chain kernel, or the interpreter's."""
        n, arr, fr = self._wrench_list(bodies, frame)
        buf = ctypes.create_string_buffer(256)
        _check(lib().grbda_wrench_kernel_name(self._h, 0 if algo == "aba" else 1, 32 if dtype == "f32" else 64, n, arr, fr, B, device, buf, 256))
        return buf.value.decode()

    def _wrench_host(self, name: str, q, qd, x, bodies, wrench, frame, device):
        import numpy as np

        n, arr, fr = self._wrench_list(bodies, frame)
        q, qd, x = (np.ascontiguousarray(a, dtype="float64") for a in (q, qd, x))
        w = None if wrench is None else np.ascontiguousarray(wrench, dtype="float64")
        if w is not None and w.shape != (q.shape[0], n, 6):
            raise ValueError(f"expected wrench[{q.shape[0]},{n},6]")
        out = np.empty_like(x)
        _check(getattr(lib(), "grbda_" + name)(self._h, q.ctypes.data, qd.ctypes.data, x.ctypes.data, n, arr, None if w is None else w.ctypes.data,
                                               fr, out.ctypes.data, q.shape[0], device))
        return out

    def forward_dynamics_wrench_host(self, q, qd, tau, bodies, wrench, frame="body", device: int = 0):
        return self._wrench_host("aba_wrench_host_f64", q, qd, tau, bodies, wrench, frame, device)

    def inverse_dynamics_wrench_host(self, q, qd, ydd, bodies, wrench, frame="body", device: int = 0):
        return self._wrench_host("rnea_wrench_host_f64", q, qd, ydd, bodies, wrench, frame, device)


class _ContactStepMethods:
    """Scheduled contacts (include/grbda_hip_contact_step.h), kept apart like _WrenchMethods: the contacts of contact_dynamics /
    contact_impulse -- bodies[n], offsets[n][3], n in 1..8 -- with a mask per state, active[B] (any integer tensor on the device; bit c
    set: contact c is closed in that state).  They go through Plan._call like every other method; the masks are made int32 and
    contiguous on the call's stream."""

    @staticmethod
    def _mask(stream, device, mask, shape):
        """the mask as the entry points take it (int32, contiguous, on the call's stream), or None"""
        import torch

        if mask is None:
            return None
        if not getattr(mask, "is_cuda", False) or mask.dtype.is_floating_point or mask.device != device or tuple(mask.shape) != tuple(shape):
            raise ValueError(f"expected an integer device tensor active[{','.join(str(d) for d in shape)}] on the device of q")
        with torch.cuda.stream(torch.cuda.current_stream(device) if stream is None else stream):
            m = mask.to(torch.int32).contiguous()
        if stream is not None:
            mask.record_stream(stream)
            m.record_stream(stream)
        return m

    def contact_dynamics_active(self, q, qd, tau, bodies, offsets, active, a_des=None, kd: float = 0.0, damping: float = 0.0, stream=None):
        """contact_dynamics on the contacts whose bit is set in active[B], state by state (grbda_contact_dynamics_active_*), with the
        right-hand side a_des - kd p_dot - p_ddot(ydd_free).  Returns (ydd[B, nv], lambda[B, n, 3] -- exactly 0 for the open contacts --,
        ydd_free[B, nv]); a state with no closed contact has ydd == ydd_free."""
        c = self._contacts(bodies, offsets)
        m = self._mask(stream, q.device, active, (q.shape[0],))
        return self._call("contact_dynamics_active", stream, dict(self._state(q, qd=qd, tau=tau), a_des=(a_des, (c[0], 3))),
                          dict(ydd=self.nv, lam=(c[0], 3), ydd_free=self.nv),
                          ("q", "qd", "tau", *c, m.data_ptr(), "a_des", float(kd), float(damping), "ydd", "lam", "ydd_free"))

    def contact_impulse_active(self, q, qd, bodies, offsets, active, v_des=None, restitution: float = 0.0, damping: float = 0.0, out=None,
                               stream=None):
        """contact_impulse on the contacts whose bit is set in active[B], state by state (grbda_contact_impulse_active_*).  Returns
        (qd_next[B, nv], impulse[B, n, 3] -- exactly 0 for the open contacts); a state with no closed contact keeps the bits of qd.
        out: the tensor qd_next is written to; it may be qd."""
        c = self._contacts(bodies, offsets)
        m = self._mask(stream, q.device, active, (q.shape[0],))
        return self._call("contact_impulse_active", stream, dict(self._state(q, qd=qd), v_des=(v_des, (c[0], 3))),
                          dict(qd_next=self.nv, impulse=(c[0], 3)),
                          ("q", "qd", *c, m.data_ptr(), "v_des", float(restitution), float(damping), "qd_next", "impulse"),
                          fixed=dict(qd_next=(out, self.nv)))

    def contact_step(self, q, qd, tau, bodies, offsets, active, dt: float, prev_active=None, kd: float = 0.0, restitution: float = 0.0,
                     damping: float = 0.0, out=None, stream=None):
        """One contact-aware step (grbda_contact_step_*): where a contact closes against prev_active[B], the impact with every closed
        contact as a constraint (contact_impulse_active, v_des = 0); contact_dynamics_active at the velocities after it; integrate.
        prev_active=None: no impulse stage at all.  Returns (q_next, qd_next, ydd, lambda[B, n, 3], impulse[B, n, 3] or None,
        ok[B] bool).  out: (q_next, qd_next) to write to; they may be q and qd themselves."""
        c = self._contacts(bodies, offsets)
        m = self._mask(stream, q.device, active, (q.shape[0],))
        mp = self._mask(stream, q.device, prev_active, (q.shape[0],))
        qn, vn = (None, None) if out is None else out
        return self._call("contact_step", stream, self._state(q, qd=qd, tau=tau),
                          dict(q_next=self.nq, qd_next=self.nv, ydd=self.nv, lam=(c[0], 3), impulse=None if mp is None else (c[0], 3), ok=bool),
                          ("q", "qd", "tau", *c, m.data_ptr(), None if mp is None else mp.data_ptr(), float(kd), float(restitution), float(damping),
                           float(dt), "ydd", "lam", "impulse", "q_next", "qd_next", "ok"),
                          fixed=dict(q_next=(qn, self.nq), qd_next=(vn, self.nv)))

    def contact_rollout(self, q, qd, tau, bodies, offsets, active, dt: float, T: int, active_prev=None, with_impulses: bool = True,
                        kd: float = 0.0, restitution: float = 0.0, damping: float = 0.0, record: bool = False, stream=None):
        """T contact-aware steps from (q, qd), which are left untouched (grbda_contact_rollout_* on copies).  tau: [B, nv] held, or
        [T, B, nv]; active: [B] held, or [T, B].  Step t closes contacts against active[t - 1], step 0 against active_prev (None:
        nothing closes); with_impulses=False: no impulse stage in any step.  Returns (q_T, qd_T, ok[B] bool -- the AND over the steps),
        and with record=True also (q_traj[T,B,nq], qd_traj[T,B,nv], lambda_traj[T,B,n,3])."""
        import torch

        T = int(T)
        c = self._contacts(bodies, offsets)
        per_step = tau.dim() == 3
        B, dtype, device, _ = self._checked(dict(self._state(q, qd=qd), tau=(tau, (T, "B", self.nv) if per_step else self.nv)))
        s, t = self._contiguous(stream, device, dict(tau=tau))
        masks = active.dim() == 2
        m = self._mask(stream, device, active, (T, B) if masks else (B,))
        mp = self._mask(stream, device, active_prev, (B,))
        self._hold(stream, q, qd, tau, t["tau"])
        with torch.cuda.stream(s):  # (the copies are enqueued, and everything the steps write is allocated, on the call's stream)
            qT, vT = q.clone(memory_format=torch.contiguous_format), qd.clone(memory_format=torch.contiguous_format)
            work = torch.empty_like(vT)
            ok = torch.ones((B,), dtype=torch.int32, device=device)
            qt = torch.empty((T, B, self.nq), dtype=dtype, device=device) if record else None
            vt = torch.empty((T, B, self.nv), dtype=dtype, device=device) if record else None
            lt = torch.empty((T, B, c[0], 3), dtype=dtype, device=device) if record else None
            ptr = lambda a: None if a is None else a.data_ptr()
            self._dispatch("contact_rollout", dtype, qT.data_ptr(), vT.data_ptr(), t["tau"].data_ptr(), T if per_step else 1, *c, m.data_ptr(),
                           T if masks else 1, ptr(mp), 1 if with_impulses else 0, float(kd), float(restitution), float(damping), float(dt), T,
                           work.data_ptr(), ptr(qt), ptr(vt), ptr(lt), ok.data_ptr(), B, device.index or 0, s.cuda_stream)
            return (qT, vT, ok.bool(), qt, vt, lt) if record else (qT, vT, ok.bool())

    def contact_step_host(self, q, qd, tau, bodies, offsets, active, dt: float, prev_active=None, kd: float = 0.0, restitution: float = 0.0,
                          damping: float = 0.0, device: int = 0):
        """contact_step on host arrays (grbda_contact_step_host_f64): returns (q_next, qd_next, ydd, lambda, impulse or None, ok)."""
        import numpy as np

        c = self._contacts(bodies, offsets)
        q, qd, tau = (np.ascontiguousarray(a, dtype="float64") for a in (q, qd, tau))
        B = q.shape[0]
        m = np.ascontiguousarray(active, dtype="int32")
        mp = None if prev_active is None else np.ascontiguousarray(prev_active, dtype="int32")
        qn, vn, ydd = np.empty_like(q), np.empty_like(qd), np.empty_like(qd)
        lam, ok = np.empty((B, c[0], 3)), np.empty((B,), dtype="int32")
        imp = None if mp is None else np.empty((B, c[0], 3))
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(lib().grbda_contact_step_host_f64(self._h, ptr(q), ptr(qd), ptr(tau), *c, ptr(m), ptr(mp), float(kd), float(restitution), float(damping),
                                                 float(dt), ptr(ydd), ptr(lam), ptr(imp), ptr(qn), ptr(vn), ptr(ok), B, device))
        return qn, vn, ydd, lam, imp, ok.astype(bool)


class _BodyListMethods:
    """Poses and twists of a listed few bodies (include/grbda_hip_bodies.h), kept apart like _WrenchMethods.  bodies: up to 16 plan body
    indices in any order; a body may repeat and may stand next to its ancestors.  Slot i of a result is row bodies[i] of body_poses /
    body_twists."""

    @staticmethod
    def _body_list(bodies):
        n = len(bodies)
        return n, (c_int * max(n, 1))(*[int(b) for b in bodies])

    def body_poses_list(self, q, bodies, stream=None):
        """[B, n, 12] = E (9, row-major) then r (3) of the listed bodies (grbda_body_poses_list_*)."""
        n, arr = self._body_list(bodies)
        return self._call("body_poses_list", stream, self._state(q), dict(out=(n, 12)), ("q", n, arr, "out"))[0]

    def body_twists_list(self, q, qd, ydd, bodies, stream=None):
        """[B, n, 12] = v (6) then a (6) of the listed bodies in their own coordinates, the acceleration carrying -gravity
        (grbda_body_twists_list_*)."""
        n, arr = self._body_list(bodies)
        return self._call("body_twists_list", stream, self._state(q, qd=qd, ydd=ydd), dict(out=(n, 12)), ("q", "qd", "ydd", n, arr, "out"))[0]

    def body_list_walk(self, bodies):
        """(walk_len, max_saved, route) of a body list (grbda_body_list_walk; no device): the bodies the kernels visit, the peak number of
        branch-point values held at once, and the route -- 0 the walk, 1 the full kernel and a gather."""
        n, arr = self._body_list(bodies)
        a, b, c = c_int(0), c_int(0), c_int(0)
        _check(lib().grbda_body_list_walk(self._h, n, arr, byref(a), byref(b), byref(c)))
        return a.value, b.value, c.value

    def body_poses_list_host(self, q, bodies, device: int = 0):
        import numpy as np

        n, arr = self._body_list(bodies)
        q = np.ascontiguousarray(q, dtype="float64")
        out = np.empty((q.shape[0], n, 12))
        _check(lib().grbda_body_poses_list_host_f64(self._h, q.ctypes.data, n, arr, out.ctypes.data, q.shape[0], device))
        return out

    def body_twists_list_host(self, q, qd, ydd, bodies, device: int = 0):
        import numpy as np

        n, arr = self._body_list(bodies)
        q, qd, ydd = (np.ascontiguousarray(a, dtype="float64") for a in (q, qd, ydd))
        out = np.empty((q.shape[0], n, 12))
        _check(lib().grbda_body_twists_list_host_f64(self._h, q.ctypes.data, qd.ctypes.data, ydd.ctypes.data, n, arr, out.ctypes.data, q.shape[0],
                                                     device))
        return out


class _JacobianMethods:
    """Frame Jacobians and their drift at a listed few body frames (include/grbda_hip_jacobians.h), kept apart like _WrenchMethods.  A frame
    is the body-fixed point offsets[i] (the reference's body axes; None: the body origins) of body bodies[i], with the body's axes
    (frame="body") or world axes (frame="world"); up to 16 frames, a body may repeat."""

    @staticmethod
    def _frames(bodies, offsets, frame):
        if frame not in ("body", "world"):
            raise ValueError('frame must be "body" or "world"')
        n = len(bodies)
        if offsets is not None and (len(offsets) != n or any(len(o) != 3 for o in offsets)):
            raise ValueError("offsets must hold one (x, y, z) per body")
        off = None if offsets is None else (c_double * max(3 * n, 1))(*[float(x) for o in offsets for x in o])
        return n, (c_int * max(n, 1))(*[int(b) for b in bodies]), off, 0 if frame == "body" else 1

    def frame_jacobians(self, q, bodies, offsets=None, frame="body", qd=None, drift=False, stream=None):
        """J[B, n, 6, nv] with v_frame = J qd, each frame [angular 3; linear 3], structural zeros written (grbda_frame_jacobians_*).
        drift=True (needs qd): returns (J, drift[B, n, 6]), drift = Jdot qd, the frame's acceleration at ydd = 0 without gravity, so that
        a_frame = J ydd + drift."""
        n, arr, off, fr = self._frames(bodies, offsets, frame)
        if drift and qd is None:
            raise ValueError("the drift needs qd")
        ins = self._state(q, qd=qd) if drift else self._state(q)
        outs = self._call("frame_jacobians", stream, ins, dict(J=(n, 6, self.nv), drift=(n, 6) if drift else None),
                          ("q", "qd" if drift else None, n, arr, off, fr, "J", "drift"))
        return outs if drift else outs[0]

    def frame_drift(self, q, qd, bodies, offsets=None, frame="body", stream=None):
        """drift[B, n, 6] alone (grbda_frame_jacobians_* with a NULL J)."""
        n, arr, off, fr = self._frames(bodies, offsets, frame)
        return self._call("frame_jacobians", stream, self._state(q, qd=qd), dict(J=None, drift=(n, 6)), ("q", "qd", n, arr, off, fr, "J", "drift"))[1]

    def frame_jacobians_route(self, bodies):
        """(route, walk_len, max_saved) of a frame list (grbda_frame_jacobians_route; no device): 0 the walk kernel, 1 the expanded batch
        through the listed twists; the bodies the walk visits and the peak number of branch-point values it holds at once."""
        n = len(bodies)
        a, b, c = c_int(0), c_int(0), c_int(0)
        _check(lib().grbda_frame_jacobians_route(self._h, n, (c_int * max(n, 1))(*[int(x) for x in bodies]), byref(a), byref(b), byref(c)))
        return a.value, b.value, c.value

    def frame_jacobians_host(self, q, bodies, offsets=None, frame="body", qd=None, drift=False, device: int = 0):
        import numpy as np

        n, arr, off, fr = self._frames(bodies, offsets, frame)
        if drift and qd is None:
            raise ValueError("the drift needs qd")
        q = np.ascontiguousarray(q, dtype="float64")
        qd = np.ascontiguousarray(qd, dtype="float64") if drift else None
        J, d = np.empty((q.shape[0], n, 6, self.nv)), np.empty((q.shape[0], n, 6)) if drift else None
        _check(lib().grbda_frame_jacobians_host_f64(self._h, q.ctypes.data, qd.ctypes.data if drift else None, n, arr, off, fr, J.ctypes.data,
                                                    d.ctypes.data if drift else None, q.shape[0], device))
        return (J, d) if drift else J


class _JacobianProductMethods:
    """J v and J^T f with the frame Jacobians of a listed few body frames, J never formed (include/grbda_hip_jacobian_products.h), kept
    apart like _JacobianMethods, whose frames (bodies, offsets, frame) these are: J is the J of frame_jacobians for the same arguments."""

    def frame_jacobian_products(self, q, bodies, v=None, f=None, offsets=None, frame="body", stream=None):
        """(Jv, JTf) (grbda_frame_jacobian_products_*): Jv[B, n, 6] = J v for v[B, nv], each frame [angular 3; linear 3], and JTf[B, nv] =
        sum over the frames of J_i^T f[:, i] for f[B, n, 6], per frame [moment 3; force 3] in the frame of J.  v or f may be None, not both;
        the product of the one left out is None and its work is skipped."""
        n, arr, off, fr = self._frames(bodies, offsets, frame)
        if v is None and f is None:
            raise ValueError("v and f cannot both be None")
        ins = dict(self._state(q), v=(v, self.nv), f=(f, (n, 6)))
        outs = dict(Jv=None if v is None else (n, 6), JTf=None if f is None else self.nv)
        return self._call("frame_jacobian_products", stream, ins, outs, ("q", "v", "f", n, arr, off, fr, "Jv", "JTf"))

    def frame_jv(self, q, v, bodies, offsets=None, frame="body", stream=None):
        """Jv[B, n, 6] alone: the frames' velocities for the joint-space direction v."""
        if v is None:
            raise ValueError("v cannot be None")
        return self.frame_jacobian_products(q, bodies, v=v, offsets=offsets, frame=frame, stream=stream)[0]

    def frame_jtf(self, q, f, bodies, offsets=None, frame="body", stream=None):
        """JTf[B, nv] alone: the joint torques of the frames' wrenches f."""
        if f is None:
            raise ValueError("f cannot be None")
        return self.frame_jacobian_products(q, bodies, f=f, offsets=offsets, frame=frame, stream=stream)[1]

    def frame_jacobian_products_host(self, q, bodies, v=None, f=None, offsets=None, frame="body", device: int = 0):
        import numpy as np

        n, arr, off, fr = self._frames(bodies, offsets, frame)
        if v is None and f is None:
            raise ValueError("v and f cannot both be None")
        q = np.ascontiguousarray(q, dtype="float64")
        B = q.shape[0]
        v = None if v is None else np.ascontiguousarray(v, dtype="float64")
        f = None if f is None else np.ascontiguousarray(f, dtype="float64")
        if (v is not None and v.shape != (B, self.nv)) or (f is not None and f.shape != (B, n, 6)):
            raise ValueError(f"expected v[{B},{self.nv}], f[{B},{n},6]")
        Jv = None if v is None else np.empty((B, n, 6))
        JTf = None if f is None else np.empty((B, self.nv))
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(lib().grbda_frame_jacobian_products_host_f64(self._h, q.ctypes.data, ptr(v), ptr(f), n, arr, off, fr, ptr(Jv), ptr(JTf), B, device))
        return Jv, JTf


class _JvpMethods:
    """The Jacobian-vector products of Plan (include/grbda_hip_jvp.h), kept apart like _VjpMethods.  Every tangent is [B, nv]; a position
    tangent lies along the tangent step of fd_dq, the coordinates of the "q" gradients of id_vjp / fd_vjp / step_vjp, so that
    <g, jvp(u)> = <vjp(g), u> without conversion.  A tangent that is None is zero; not all tangents of a call may be None."""

    @staticmethod
    def _tangents(*tangents):
        if all(t is None for t in tangents):
            raise ValueError("the tangents of a call cannot all be None")

    def id_jvp(self, q, qd, ydd, dq=None, dqd=None, dydd=None, step: float = 1e-6, stream=None):
        """d tau / d q dq + d tau / d qd dqd + H dydd of the inverse dynamics at (q, qd, ydd) (grbda_rnea_jvp_*): dtau[B, nv] -- the
        matrices of id_derivatives summed along their rows inside the library, H dydd by two inverse dynamics.  dydd alone runs no
        derivative recursion; `step` as in id_derivatives."""
        self._tangents(dq, dqd, dydd)
        ins = dict(self._state(q, qd=qd, ydd=ydd), dq=(dq, self.nv), dqd=(dqd, self.nv), dydd=(dydd, self.nv))
        return self._call("rnea_jvp", stream, ins, dict(out=self.nv), ("q", "qd", "ydd", "dq", "dqd", "dydd", float(step), "out"), skip_empty=True)[0]

    def fd_jvp(self, q, qd, tau, dq=None, dqd=None, dtau=None, step: float = 1e-6, with_ydd: bool = False, stream=None):
        """d ydd / d q dq + d ydd / d qd dqd + d ydd / d tau dtau of the forward dynamics (grbda_aba_jvp_*): dydd[B, nv], or
        (dydd, ydd) with with_ydd -- ydd = FD(q, qd, tau), which the call computes anyway whenever dq or dqd is given.
        dydd = H^-1 (dtau - d tau / d q dq - d tau / d qd dqd) by two forward dynamics at zero velocity: no factorisation, no solve, no
        [B, nv, nv] tensor."""
        self._tangents(dq, dqd, dtau)
        ins = dict(self._state(q, qd=qd, tau=tau), dq=(dq, self.nv), dqd=(dqd, self.nv), dtau=(dtau, self.nv))
        got = self._call("aba_jvp", stream, ins, dict(out=self.nv, ydd_out=self.nv if with_ydd else None),
                         ("q", "qd", "tau", "dq", "dqd", "dtau", float(step), "out", "ydd_out"), skip_empty=True)
        return got if with_ydd else got[0]

    def integrate_jvp(self, qd_next, dt: float, dq=None, dqd=None, dydd=None, stream=None):
        """The tangents (dq, dqd, dydd) pushed through integrate (grbda_integrate_jvp_*): (dq_next, dqd_next), each [B, nv].
        qd_next[B, nv]: the velocities integrate / step returned.  One kernel launch; q does not enter."""
        self._tangents(dq, dqd, dydd)
        ins = dict(qd_next=(qd_next, self.nv), dq=(dq, self.nv), dqd=(dqd, self.nv), dydd=(dydd, self.nv))
        return self._call("integrate_jvp", stream, ins, dict(dq_next=self.nv, dqd_next=self.nv),
                          ("qd_next", float(dt), "dq", "dqd", "dydd", "dq_next", "dqd_next"), skip_empty=True)

    def step_jvp(self, q, qd, tau, qd_next, dt: float, dq=None, dqd=None, dtau=None, step: float = 1e-6, stream=None):
        """The tangents (dq, dqd, dtau) pushed through step(q, qd, tau, dt) (grbda_step_jvp_*): fd_jvp, then integrate_jvp on its
        result, on one stream -- (dq_next, dqd_next), the product A dx + B du of the step's discrete-time matrices, which are never
        built.  `step` as in fd_jvp."""
        self._tangents(dq, dqd, dtau)
        ins = dict(self._state(q, qd=qd, tau=tau, qd_next=qd_next), dq=(dq, self.nv), dqd=(dqd, self.nv), dtau=(dtau, self.nv))
        return self._call("step_jvp", stream, ins, dict(dq_next=self.nv, dqd_next=self.nv),
                          ("q", "qd", "tau", "qd_next", float(dt), "dq", "dqd", "dtau", float(step), "dq_next", "dqd_next"), skip_empty=True)


class Plan(_VjpMethods, _StepVjpMethods, _WrenchMethods, _ContactStepMethods, _BodyListMethods, _JacobianMethods, _JacobianProductMethods, _JvpMethods):
    """An immutable compiled model (``grbda_plan``)."""

    def __init__(self, blob: bytes):
        self._h = c_void_p()
        self._blob = bytes(blob)
        _check(lib().grbda_plan_from_blob(self._blob, len(self._blob), byref(self._h)))
        nq, nv, nb, nc = c_int(), c_int(), c_int(), c_int()
        _check(lib().grbda_plan_dims(self._h, byref(nq), byref(nv), byref(nb), byref(nc)))
        self.nq, self.nv, self.n_bodies, self.n_clusters = nq.value, nv.value, nb.value, nc.value

    @classmethod
    def from_model(cls, model) -> "Plan":
        return cls(model.serialize())

    @classmethod
    def from_urdf(cls, path, ori_repr: str = "quaternion") -> "Plan":
        return cls(urdf_to_blob(path, ori_repr))

    def __del__(self):
        try:
            if self._h:
                lib().grbda_plan_free(self._h)
                self._h = c_void_p()
        except Exception:
            pass

    @property
    def blob(self) -> bytes:
        p, n = c_void_p(), c_size_t()
        _check(lib().grbda_plan_blob(self._h, byref(p), byref(n)))
        return ctypes.string_at(p, n.value)

    def set_gravity(self, g):
        arr = (c_double * 3)(*[float(x) for x in g])
        _check(lib().grbda_plan_set_gravity(self._h, arr))

    def get_gravity(self):
        arr = (c_double * 3)()
        _check(lib().grbda_plan_get_gravity(self._h, arr))
        return list(arr)

    def release_work(self) -> int:
        """Frees the work buffers the chunked pipelines keep per (device, stream) between calls (grbda_plan_release_work);
        returns the bytes handed back."""
        n = ctypes.c_ulonglong(0)
        _check(lib().grbda_plan_release_work(self._h, byref(n)))
        return int(n.value)

    def info(self) -> PlanInfo:
        info = PlanInfo()
        _check(lib().grbda_plan_info(self._h, byref(info)))
        return info

    def kernel_name(self, algo: str, dtype: str, B: int, device: int = 0) -> str:
        """The kernel forward ("aba") / inverse ("rnea") dynamics launch for B states in "f32" / "f64" (grbda_kernel_name)."""
        buf = ctypes.create_string_buffer(256)
        _check(lib().grbda_kernel_name(self._h, 0 if algo == "aba" else 1, 32 if dtype == "f32" else 64, B, device, buf, 256))
        return buf.value.decode()

    # ---- the one path from torch device tensors to an entry point ----------------------------------
    # A tensor is described as name -> (tensor or None, shape): `shape` is the per-state shape, an int or a tuple, the batch
    # going in front of it -- or the whole shape with "B" where the batch stands.  Bad arguments raise by one rule:
    #   not a HIP device tensor, or not float32 / float64       GrbdaError(-3): there is no CPU fallback
    #   dtype or device differs between the tensors of a call   TypeError
    #   a wrong shape; an `out` / in-place tensor with strides  ValueError naming the expected shapes
    @staticmethod
    def _full(shape, B):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        return tuple(B if d == "B" else d for d in shape) if "B" in shape else (B,) + shape

    def _state(self, q, **velocities):
        """q[B, nq] and the [B, nv] tensors, by name"""
        return dict(q=(q, self.nq), **{k: (t, self.nv) for k, t in velocities.items()})

    def _f_ext(self, f_ext):
        return f_ext, (self.n_bodies, 6)

    def _checked(self, ins, fixed=None):
        """Steps 1-3 of _call.  ins, fixed: name -> (tensor or None, shape); the first tensor is required and gives the batch B.
        `fixed` are tensors the call writes to (a caller's `out`, an in-place argument): they are taken as they are, so they must be
        contiguous.  Returns (B, dtype, device, the tensors by name)."""
        import torch

        spec = {**ins, **(fixed or {})}
        tensors = [t for t, _ in spec.values()]
        held = tensors[:1] + [t for t in tensors[1:] if t is not None]
        for t in held:
            if not getattr(t, "is_cuda", False) or t.dtype not in (torch.float32, torch.float64):
                raise GrbdaError(-3, "every tensor must be a float32 / float64 HIP device tensor (there is no CPU fallback)")
        if any(t.dtype != held[0].dtype or t.device != held[0].device for t in held):
            raise TypeError("all tensors of one call must share dtype and device")
        B = held[0].shape[0] if held[0].dim() else -1
        for name, (t, shape) in spec.items():
            if t is not None and (tuple(t.shape) != self._full(shape, B) or (name in (fixed or ()) and not t.is_contiguous())):
                want = ", ".join(f"{k}[{','.join(str(d) for d in self._full(shp, 'B'))}]" for k, (_, shp) in spec.items())
                raise ValueError(f"expected {want}" + (f", with {' and '.join(fixed)} contiguous" if fixed else ""))
        return B, held[0].dtype, held[0].device, {k: t for k, (t, _) in spec.items()}

    @staticmethod
    def _contiguous(stream, device, tensors):
        """Steps 4 and 6 of _call: (the call's stream -- the caller's, or else the device's current one --, the tensors contiguous).
        The copy of a strided input is enqueued on that stream, ahead of the kernels that read it."""
        import torch

        if stream is None:
            return torch.cuda.current_stream(device), {k: None if t is None else t.contiguous() for k, t in tensors.items()}
        with torch.cuda.stream(stream):
            return stream, {k: None if t is None else t.contiguous() for k, t in tensors.items()}

    @staticmethod
    def _hold(stream, *tensors):
        """Step 7 of _call: on a caller's stream the caching allocator is told of every tensor the call holds -- the inputs as given,
        their contiguous copies and the outputs, which were allocated on other streams"""
        if stream is not None:
            for t in tensors:
                if t is not None:
                    t.record_stream(stream)

    def _dispatch(self, stem: str, dtype, *cargs):
        """Steps 8-9 of _call: grbda_<stem>_<f32|f64>(plan, cargs...), checked"""
        _check(getattr(lib(), f"grbda_{stem}_{_suffix(dtype)}")(self._h, *cargs))

    def _call(self, stem, stream, ins, outs, args, tail=(), fixed=None, skip_empty=False):
        """One entry-point call on device tensors:
        1-3  _checked(ins, fixed): tensor kind, agreement, shapes
        4, 6 _contiguous: the stream, and the inputs made contiguous on it
        5    the outputs are allocated -- outs: name -> shape, or int / bool for int32 flags [B], or None for one that is not
             wanted; a tensor of that name in `fixed` stands in for the output
        7    _hold: record_stream when the stream is the caller's
        8-9  grbda_<stem>_<f32|f64>(plan, *args, B, *tail, device, stream), checked: in `args` a str names a tensor, whose address
             (NULL for None) goes there; everything else is passed as it is.  skip_empty: no call at all for B == 0
        10   returns the outputs in the order of `outs`, flags asked for as bool converted on the call's stream"""
        import torch

        B, dtype, device, given = self._checked(ins, fixed)
        s, t = self._contiguous(stream, device, given)
        for name, shape in outs.items():
            if t.get(name) is None:
                t[name] = (None if shape is None else torch.empty((B,), dtype=torch.int32, device=device) if shape in (int, bool) else
                           torch.empty(self._full(shape, B), dtype=dtype, device=device))
        self._hold(stream, *given.values(), *t.values())
        if not (skip_empty and B == 0):
            ptr = lambda a: a if not isinstance(a, str) else None if t[a] is None else t[a].data_ptr()
            self._dispatch(stem, dtype, *[ptr(a) for a in args], B, *tail, device.index or 0, s.cuda_stream)
        if bool not in outs.values():
            return tuple(t[name] for name in outs)
        with torch.cuda.stream(s):
            return tuple(t[name].bool() if shape is bool else t[name] for name, shape in outs.items())

    @staticmethod
    def _contacts(bodies, offsets):
        """the contact set as the entry points take it: (n, bodies[n], offsets[n][3])"""
        n = len(bodies)
        if len(offsets) != n or any(len(o) != 3 for o in offsets):
            raise ValueError("offsets must hold one (x, y, z) per body")
        return n, (c_int * n)(*[int(b) for b in bodies]), (c_double * (3 * n))(*[float(x) for o in offsets for x in o])

    # ---- batched dynamics on torch device tensors ------------------------------------------------
    def forward_dynamics(self, q, qd, tau, out=None, stream=None, f_ext=None):
        """Batched ClusterTreeModel::forwardDynamics (cluster ABA): returns ydd[B, nv].
        f_ext: optional [B, n_bodies, 6] world-frame spatial forces (TreeModel::setExternalForces)."""
        return self._call("aba", stream, dict(self._state(q, qd=qd, tau=tau), f_ext=self._f_ext(f_ext)), dict(out=self.nv),
                          ("q", "qd", "tau", "f_ext", "out"), fixed=dict(out=(out, self.nv)))[0]

    def inverse_dynamics(self, q, qd, ydd, out=None, stream=None, f_ext=None):
        """Batched ClusterTreeModel::inverseDynamics (cluster RNEA): returns tau[B, nv]."""
        return self._call("rnea", stream, dict(self._state(q, qd=qd, ydd=ydd), f_ext=self._f_ext(f_ext)), dict(out=self.nv),
                          ("q", "qd", "ydd", "f_ext", "out"), fixed=dict(out=(out, self.nv)))[0]

    # ---- quantities derived from the two recursions (include/grbda_hip.h) ---------------------------
    def bias_force(self, q, qd, stream=None, f_ext=None):
        """Batched getBiasForceVector: C(q, qd) = RNEA(q, qd, 0), [B, nv]."""
        return self._call("bias", stream, dict(self._state(q, qd=qd), f_ext=self._f_ext(f_ext)), dict(out=self.nv),
                          ("q", "qd", "f_ext", "out"))[0]

    def mass_matrix(self, q, stream=None):
        """Batched getMassMatrix: H(q), [B, nv, nv]."""
        return self._call("mass_matrix", stream, self._state(q), dict(out=(self.nv, self.nv)), ("q", "out"))[0]

    def fd_dtau(self, q, stream=None):
        """d ydd / d tau = H(q)^-1 through the ABA, [B, nv, nv]."""
        return self._call("fd_dtau", stream, self._state(q), dict(out=(self.nv, self.nv)), ("q", "out"))[0]

    def fd_dqd(self, q, qd, tau, stream=None):
        """d ydd / d qd of the forward dynamics, [B, nv, nv] (exact: the ABA is quadratic in qd)."""
        return self._call("fd_dqd", stream, self._state(q, qd=qd, tau=tau), dict(out=(self.nv, self.nv)), ("q", "qd", "tau", "out"))[0]

    def fd_dq(self, q, qd, tau, step: float = 1e-6, stream=None):
        """d ydd / d q along the reference's tangent step (testHelpers.hpp:50-112), [B, nv, nv].  Explicit models:
        analytic (`step` unused).  Models with implicit loops: central differences, always taken
        in fp64 (fp32 tensors are converted on the device), on the constraint manifold."""
        return self._call("fd_dq", stream, self._state(q, qd=qd, tau=tau), dict(out=(self.nv, self.nv)),
                          ("q", "qd", "tau", step, "out"))[0]

    def fd_derivatives(self, q, qd, tau, want=("dq", "dqd", "dtau"), stream=None):
        """d ydd / d q, d ydd / d qd, d ydd / d tau of the forward dynamics in one pass (grbda_fd_derivatives_*): a dict
        of [B, nv, nv] tensors for the names in `want`.  Explicit models get the analytic recursion + one SPD solve per
        state (deriv_kernels.hip); the others fall back to fd_dtau / fd_dqd / fd_dq."""
        names = ("dq", "dqd", "dtau")
        outs = self._call("fd_derivatives", stream, self._state(q, qd=qd, tau=tau),
                          {k: (self.nv, self.nv) if k in want else None for k in names}, ("q", "qd", "tau") + names, skip_empty=True)
        return {k: o for k, o in zip(names, outs) if o is not None}

    def id_derivatives(self, q, qd, ydd, want=("dq", "dqd", "dydd"), step: float = 1e-6, stream=None):
        """d tau / d q, d tau / d qd, d tau / d ydd (= H) of the inverse dynamics at (q, qd, ydd) (grbda_rnea_derivatives_*): a dict
        of [B, nv, nv] tensors for the names in `want`, out[b, i, j] = d tau_i / d x_j, the columns of "dq" along the tangent step of
        fd_dq.  Explicit models with nv <= 64: the analytic recursion alone, no forward dynamics and no solve (`step` unused); the
        others: difference batches over the inverse dynamics, "dq" with `step`."""
        names = ("dq", "dqd", "dydd")
        if not any(k in want for k in names) or any(k not in names for k in want):
            raise ValueError('want must name at least one of "dq", "dqd", "dydd" and nothing else')
        outs = self._call("rnea_derivatives", stream, self._state(q, qd=qd, ydd=ydd),
                          {k: (self.nv, self.nv) if k in want else None for k in names}, ("q", "qd", "ydd", step) + names, skip_empty=True)
        return {k: o for k, o in zip(names, outs) if o is not None}

    # ---- steps either side of the path ------------------------------------------------------------
    @property
    def n_span_vel(self) -> int:
        n = c_int(0)
        _check(lib().grbda_plan_span_dims(self._h, byref(n)))
        return n.value

    def project_positions(self, q, max_iter: int = 50, tol: float = 1e-8, stream=None):
        """Newton projection of the dependent coordinates of implicit clusters onto phi(q) = 0, IN PLACE
        (GenericJoint.cpp:289-385).  Returns a bool tensor [B]: the state converged to |phi| < tol."""
        return self._call("project_positions", stream, {}, dict(ok=bool), ("q", "ok"), tail=(max_iter, tol), fixed=self._state(q))[0]

    @staticmethod
    def _flag_bytes(flags, n):
        if flags is None:
            return None
        if len(flags) != n:
            raise ValueError(f"expected one flag per cluster ({n})")
        return (ctypes.c_uint8 * n)(*[1 if f else 0 for f in flags])

    def state_input_dims(self, pos_is_spanning=None, vel_is_spanning=None):
        """Row widths (in_nq, in_nv) of a batch whose clusters give spanning / independent coordinates as flagged."""
        a, b = c_int(0), c_int(0)
        _check(lib().grbda_state_input_dims(self._h, self._flag_bytes(pos_is_spanning, self.n_clusters),
                                            self._flag_bytes(vel_is_spanning, self.n_clusters), byref(a), byref(b)))
        return a.value, b.value

    def state_to_independent(self, q_in, qd_in=None, pos_is_spanning=None, vel_is_spanning=None, tol: float = 1e-8,
                             want_gmax: bool = False, stream=None):
        """ClusterTreeModel::setState(ModelState) for a batch (ClusterJoint.cpp:22-71): per-cluster spanning or independent
        coordinates -> the engine's (q[B,nq], qd[B,nv]) plus status[B] (0 = valid; code + 256 * cluster otherwise) and,
        optionally, cond[B, 2] = (max |K_d^-1 K_i|, max |K_d|_F |K_d^-1|_F) over the implicit clusters."""
        wq, wv = self.state_input_dims(pos_is_spanning, vel_is_spanning)
        outs = self._call("state_to_independent", stream, dict(q_in=(q_in, wq), qd_in=(qd_in, wv)),
                          dict(q=self.nq, qd=None if qd_in is None else self.nv, status=int, cond=2 if want_gmax else None),
                          (self._flag_bytes(pos_is_spanning, self.n_clusters), self._flag_bytes(vel_is_spanning, self.n_clusters),
                           "q_in", "qd_in", "q", "qd", "status", "cond"), tail=(tol,))
        return outs if want_gmax else outs[:3]

    def constraint_gain(self, q, tol: float = 1e-8, stream=None):
        """(gmax[B], kcond[B], status[B]) of engine-coordinate positions q[B,nq]: max |K_d^-1 K_i| and max |K_d|_F |K_d^-1|_F
        over the implicit clusters, and the validity status of the positions (|phi| < tol)."""
        _, _, status, cond = self.state_to_independent(q, None, None, None, tol=tol, want_gmax=True, stream=stream)
        return cond[:, 0].contiguous(), cond[:, 1].contiguous(), status

    def spanning(self, q, qd, ydd, stream=None):
        """qd_span = G yd and qdd_span = G ydd + g for every body joint: two tensors [B, n_span_vel]."""
        n = self.n_span_vel
        return self._call("spanning", stream, self._state(q, qd=qd, ydd=ydd), dict(v=n, a=n), ("q", "qd", "ydd", "v", "a"))

    # ---- time stepping (include/grbda_hip.h "time stepping") ---------------------------------------------
    def integrate(self, q, qd, ydd, dt: float, out=None, max_iter: int = 50, tol: float = 1e-8, stream=None):
        """One semi-implicit Euler step on the configuration manifold (first order): yd' = yd + dt ydd, then the positions with yd'
        -- y + dt yd' for explicit clusters, the quaternion base by ori::integrateQuatImplicit, implicit clusters by
        q_span + dt G yd' and the Newton projection of project_positions.  Returns (q_next, qd_next, ok[B] bool).
        out: (q_next, qd_next) to write to; they may be q and qd themselves."""
        qn, vn = (None, None) if out is None else out
        return self._call("integrate", stream, self._state(q, qd=qd, ydd=ydd), dict(q_next=self.nq, qd_next=self.nv, ok=bool),
                          ("q", "qd", "ydd", float(dt), "q_next", "qd_next", "ok", int(max_iter), float(tol)),
                          fixed=dict(q_next=(qn, self.nq), qd_next=(vn, self.nv)))

    def step(self, q, qd, tau, dt: float, f_ext=None, stream=None):
        """forward_dynamics followed by integrate on one stream (grbda_step_*): returns (q_next, qd_next, ydd, ok[B] bool)."""
        return self._call("step", stream, dict(self._state(q, qd=qd, tau=tau), f_ext=self._f_ext(f_ext)),
                          dict(q_next=self.nq, qd_next=self.nv, ydd=self.nv, ok=bool),
                          ("q", "qd", "tau", "f_ext", float(dt), "ydd", "q_next", "qd_next", "ok"))

    def rollout(self, q, qd, tau, dt: float, T: int, record: bool = False, stream=None):
        """T steps from (q, qd), which are left untouched (grbda_rollout_* on copies).  tau: [B, nv], held for all steps, or [T, B, nv].
        Returns (q_T, qd_T, ok[B] bool -- the AND over the steps), and with record=True also (q_traj[T,B,nq], qd_traj[T,B,nv]):
        states 1 .. T."""
        import torch

        T = int(T)
        per_step = tau.dim() == 3
        B, dtype, device, _ = self._checked(dict(self._state(q, qd=qd), tau=(tau, (T, "B", self.nv) if per_step else self.nv)))
        s, t = self._contiguous(stream, device, dict(tau=tau))
        self._hold(stream, q, qd, tau, t["tau"])
        with torch.cuda.stream(s):  # (the copies are enqueued, and everything the steps write is allocated, on the call's stream)
            qT, vT = q.clone(memory_format=torch.contiguous_format), qd.clone(memory_format=torch.contiguous_format)
            work = torch.empty_like(vT)
            ok = torch.ones((B,), dtype=torch.int32, device=device)
            qt = torch.empty((T, B, self.nq), dtype=dtype, device=device) if record else None
            vt = torch.empty((T, B, self.nv), dtype=dtype, device=device) if record else None
            self._dispatch("rollout", dtype, qT.data_ptr(), vT.data_ptr(), t["tau"].data_ptr(), T if per_step else 1, float(dt), T,
                           work.data_ptr(), None if qt is None else qt.data_ptr(), None if vt is None else vt.data_ptr(), ok.data_ptr(), B,
                           device.index or 0, s.cuda_stream)
            return (qT, vT, ok.bool(), qt, vt) if record else (qT, vT, ok.bool())

    # ---- contact side ---------------------------------------------------------------------------------
    def body_poses(self, q, stream=None):
        """Absolute transforms world -> body (TreeNode::Xa_): [B, n_bodies, 12] = E (9, row-major) then r (3)."""
        return self._call("body_poses", stream, self._state(q), dict(out=(self.n_bodies, 12)), ("q", "out"))[0]

    def body_twists(self, q, qd, ydd, stream=None):
        """Spatial velocity and acceleration of every body in its own coordinates (TreeNode::v_ / a_ after
        forwardAccelerationKinematics): [B, n_bodies, 12] = v (6) then a (6), each [angular; linear]; the acceleration
        carries the base's -gravity as in the reference."""
        return self._call("body_twists", stream, self._state(q, qd=qd, ydd=ydd), dict(out=(self.n_bodies, 12)),
                          ("q", "qd", "ydd", "out"))[0]

    def apply_test_force(self, q, body: int, offset, force, stream=None):
        """Batched ClusterTreeModel::applyTestForce: world-frame force[B,3] at the body-fixed point `offset` of
        `body`; returns (lambda_inv[B], dstate[B,nv]) = (f^T J H^-1 J^T f, H^-1 J^T f)."""
        off = (c_double * 3)(*[float(x) for x in offset])
        return self._call("apply_test_force", stream, dict(self._state(q), force=(force, 3)), dict(lambda_inv=(), dstate=self.nv),
                          ("q", body, off, "force", "lambda_inv", "dstate"))

    def inv_osim(self, q, bodies, offsets, with_jacobian: bool = False, stream=None):
        """Batched inverseOperationalSpaceInertiaMatrix for contact frames (body index, body-fixed offset):
        Linv[B, 6n, 6n] (and the frame Jacobians J[B, 6n, nv] when asked)."""
        c = self._contacts(bodies, offsets)
        n = c[0]
        outs = self._call("inv_osim", stream, self._state(q), dict(Linv=(6 * n, 6 * n), J=(6 * n, self.nv) if with_jacobian else None),
                          ("q", *c, "Linv", "J"))
        return outs if with_jacobian else outs[0]

    def contact_points(self, q, bodies, offsets, qd=None, ydd=None, stream=None):
        """World-frame position, velocity and classical acceleration of body-fixed points (grbda_contact_points_*): point offsets[c]
        (body coordinates) of body bodies[c].  Returns (pos, vel, acc), [B, n, 3] each; vel is None without qd, acc is None without qd
        and ydd."""
        c = self._contacts(bodies, offsets)
        shape = (c[0], 3)
        return self._call("contact_points", stream, self._state(q, qd=qd, ydd=ydd),
                          dict(pos=shape, vel=None if qd is None else shape, acc=None if qd is None or ydd is None else shape),
                          ("q", "qd", "ydd", *c, "pos", "vel", "acc"))

    def contact_dynamics(self, q, qd, tau, bodies, offsets, a_des=None, damping: float = 0.0, f_ext=None, stream=None):
        """Forward dynamics with the points offsets[c] of bodies[c] held to the world-frame accelerations a_des[B, n, 3] (None: zero)
        (grbda_contact_dynamics_*): (J_w H^-1 J_w^T + damping I) lambda = a_des - p_ddot(ydd_free).  Returns (ydd[B, nv], lambda[B, n, 3]
        -- world-frame forces on the bodies at the points --, ydd_free[B, nv]).  Redundant contacts need damping > 0; a state whose
        matrix is not positive definite gets NaN and is counted by spd_bad_pivots()."""
        c = self._contacts(bodies, offsets)
        return self._call("contact_dynamics", stream,
                          dict(self._state(q, qd=qd, tau=tau), f_ext=self._f_ext(f_ext), a_des=(a_des, (c[0], 3))),
                          dict(ydd=self.nv, lam=(c[0], 3), ydd_free=self.nv),
                          ("q", "qd", "tau", "f_ext", *c, "a_des", float(damping), "ydd", "lam", "ydd_free"))

    def contact_impulse(self, q, qd, bodies, offsets, v_des=None, restitution: float = 0.0, damping: float = 0.0, stream=None):
        """The instant the points offsets[c] of bodies[c] close (grbda_contact_impulse_*): (J_w H^-1 J_w^T + damping I) Lambda =
        v_des - (1 + restitution) J_w qd, qd_next = qd + H^-1 J_w^T Lambda, with v_des[B, n, 3] (None: zero) in world axes.  Returns
        (qd_next[B, nv], impulse[B, n, 3] -- world-frame impulses on the bodies at the points); the points then move at
        v_des - restitution J_w qd - damping impulse.  q does not change; gravity and tau do not enter.  Redundant contacts need
        damping > 0; a state whose matrix is not positive definite gets NaN and is counted by spd_bad_pivots()."""
        c = self._contacts(bodies, offsets)
        return self._call("contact_impulse", stream, dict(self._state(q, qd=qd), v_des=(v_des, (c[0], 3))),
                          dict(qd_next=self.nv, impulse=(c[0], 3)),
                          ("q", "qd", *c, "v_des", float(restitution), float(damping), "qd_next", "impulse"))

    # ---- energy and centroidal quantities -----------------------------------------------------------
    def total_mass(self) -> float:
        """The sum of the body masses (grbda_plan_total_mass); no device."""
        m = c_double(0.0)
        _check(lib().grbda_plan_total_mass(self._h, byref(m)))
        return m.value

    def energy(self, q, qd=None, stream=None):
        """(kinetic[B], potential[B]) (grbda_energy_*): 1/2 yd^T H yd, None without qd; -g . sum m_i c_i, zero at the world origin."""
        return self._call("energy", stream, self._state(q, qd=qd), dict(kinetic=None if qd is None else (), potential=()),
                          ("q", "qd", "kinetic", "potential"))

    def centroidal(self, q, qd=None, ydd=None, want=("com", "com_vel", "h", "hdot"), stream=None):
        """Centre of mass, its velocity, the centroidal momentum and its rate (grbda_centroidal_*): a dict of the names in `want` --
        com[B, 3], com_vel[B, 3], h[B, 6], hdot[B, 6], world axes, h and hdot [angular about the centre of mass; linear].  com_vel and h
        need qd, hdot needs qd and ydd (the true generalized acceleration); with the default `want`, what the given inputs do not
        allow is left out."""
        names = ("com", "com_vel", "h", "hdot")
        if any(w not in names for w in want):
            raise ValueError(f"want holds names out of {names}")
        default = tuple(want) == names
        need = {"com": (), "com_vel": (qd,), "h": (qd,), "hdot": (qd, ydd)}
        shape = {"com": 3, "com_vel": 3, "h": 6, "hdot": 6}
        ask = {n: n in want and not (default and any(t is None for t in need[n])) for n in names}
        outs = self._call("centroidal", stream, self._state(q, qd=qd, ydd=ydd), {n: shape[n] if ask[n] else None for n in names},
                          ("q", "qd", "ydd") + names)
        return {n: o for n, o in zip(names, outs) if ask[n]}

    def centroidal_matrix(self, q, stream=None):
        """The centroidal momentum matrix A[B, 6, nv], h = A(q) yd (grbda_centroidal_matrix_*)."""
        return self._call("centroidal_matrix", stream, self._state(q), dict(A=(6, self.nv)), ("q", "A"))[0]

    def time_kernel(self, which: str, q, qd, x, out, iters: int = 20, stream=None) -> float:
        """Average kernel duration in ms, hipEvents on the launch stream (grbda_time_kernel)."""
        B, dtype, device, given = self._checked(self._state(q, qd=qd, x=x), dict(out=(out, self.nv)))
        s, t = self._contiguous(stream, device, given)
        self._hold(stream, *given.values(), *t.values())
        ms = c_float(0)
        _check(lib().grbda_time_kernel(self._h, 0 if which == "aba" else 1, int(_suffix(dtype)[1:]), t["q"].data_ptr(), t["qd"].data_ptr(),
                                       t["x"].data_ptr(), out.data_ptr(), B, device.index or 0, s.cuda_stream, iters, byref(ms)))
        return ms.value

    def sharded_device(self, which: str, qs, qds, xs, outs=None, gathered=None, streams=None):
        """grbda_{aba,rnea}_sharded_dev_*: shard g = the device tensors qs[g], qds[g], xs[g] on THEIR device (one process, several
        devices), launched on streams[g] (default: each device's current stream).  outs: per-shard output tensors (made when
        None and no `gathered`); gathered: a [sum B, nv] tensor on the first shard's device that receives every slab over the
        peer links.  Enqueues only.  Returns (outs, gathered)."""
        import torch

        n = len(qs)
        if n < 1 or len(qds) != n or len(xs) != n:
            raise ValueError("one q, qd, x tensor per shard")
        shards = [self._checked(self._state(qs[g], qd=qds[g], x=xs[g]), dict(out=(None if outs is None else outs[g], self.nv)))
                  for g in range(n)]
        Bs, dt, devices = [sh[0] for sh in shards], shards[0][1], [sh[2] for sh in shards]
        if gathered is not None:
            rows, gdt, gdev, _ = self._checked({}, dict(gathered=(gathered, self.nv)))
            if rows != sum(Bs):
                raise ValueError(f"expected gathered[{sum(Bs)},{self.nv}], contiguous")
        if any(sh[1] != dt for sh in shards) or (gathered is not None and (gdt != dt or gdev != devices[0])):
            raise TypeError("every shard, and gathered on the first shard's device, must have one dtype")
        if outs is None and gathered is None:
            outs = [torch.empty((Bs[g], self.nv), dtype=dt, device=devices[g]) for g in range(n)]
        elif outs is None:
            # shards on the gather device write straight into their place; the others need a slab of their own
            outs = [None if devices[g] == gathered.device else torch.empty((Bs[g], self.nv), dtype=dt, device=devices[g]) for g in range(n)]
        on = [self._contiguous(None if streams is None else streams[g], devices[g], shards[g][3]) for g in range(n)]
        for g in range(n):
            self._hold(None if streams is None else streams[g], *shards[g][3].values(), *on[g][1].values(), outs[g], gathered)
        P = c_void_p
        arr = lambda ts: (P * n)(*[None if t is None else t.data_ptr() for t in ts])
        self._dispatch(which + "_sharded_dev", dt, n, (c_int * n)(*[d.index or 0 for d in devices]), arr([t["q"] for _, t in on]),
                       arr([t["qd"] for _, t in on]), arr([t["x"] for _, t in on]), arr(outs), (c_size_t * n)(*Bs),
                       (P * n)(*[s.cuda_stream for s, _ in on]), None if gathered is None else gathered.data_ptr())
        return outs, gathered

    # ---- host convenience (numpy) -----------------------------------------------------------------
    def _host(self, name: str, dt, arrays, *tail):
        """grbda_<name>(plan, arrays..., out, B, *tail) on host arrays (q, qd, x[, f_ext]) of dtype dt; `out` is shaped like x"""
        import numpy as np

        arrays = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a in arrays]
        out = np.empty_like(arrays[2])
        _check(getattr(lib(), "grbda_" + name)(self._h, *[None if a is None else a.ctypes.data for a in arrays], out.ctypes.data,
                                               arrays[0].shape[0], *tail))
        return out

    def sharded_host(self, which: str, q, qd, x, n_gpus: int):
        """Host numpy arrays (float32 or float64), batch split over devices 0 .. n_gpus-1 in this process."""
        import numpy as np

        dt = "float32" if q.dtype == np.float32 else "float64"
        return self._host(f"{which}_sharded_{_suffix(dt)}", dt, (q, qd, x), n_gpus)

    def forward_dynamics_host(self, q, qd, tau, device: int = 0, f_ext=None):
        return self._host("aba_host_f64", "float64", (q, qd, tau, f_ext), device)

    def inverse_dynamics_host(self, q, qd, ydd, device: int = 0, f_ext=None):
        return self._host("rnea_host_f64", "float64", (q, qd, ydd, f_ext), device)


_ad_functions = {}


def _autograd_function(forward: bool):
    """the torch.autograd.Function behind Plan.forward_dynamics_ad (forward) / inverse_dynamics_ad, made on first use (torch is imported
    by the calls, not by the package)"""
    if forward not in _ad_functions:
        import torch
        from torch.autograd.function import once_differentiable

        names = ("q", "qd", "tau" if forward else "ydd")

        class Dynamics(torch.autograd.Function):
            @staticmethod
            def forward(ctx, plan, q, qd, x):
                ctx.plan = plan
                ctx.save_for_backward(q, qd, x)
                return plan.forward_dynamics(q, qd, x) if forward else plan.inverse_dynamics(q, qd, x)

            @staticmethod
            @once_differentiable
            def backward(ctx, g):
                want = tuple(k for k, needed in zip(names, ctx.needs_input_grad[1:]) if needed)
                got = (ctx.plan.fd_vjp if forward else ctx.plan.id_vjp)(*ctx.saved_tensors, g, want=want)
                return (None,) + tuple(got.get(k) for k in names)

        Dynamics.__name__ = Dynamics.__qualname__ = "ForwardDynamics" if forward else "InverseDynamics"
        _ad_functions[forward] = Dynamics
    return _ad_functions[forward]


def _step_autograd_function(rollout: bool):
    """the torch.autograd.Function behind Plan.step_ad / rollout_ad, made on first use like _autograd_function"""
    key = ("step", rollout)
    if key not in _ad_functions:
        import torch
        from torch.autograd.function import once_differentiable

        names = ("q", "qd", "tau")

        class Step(torch.autograd.Function):
            @staticmethod
            def forward(ctx, plan, q, qd, tau, dt, T):
                ctx.plan, ctx.dt = plan, dt
                if rollout:
                    q_out, qd_out = plan.rollout(q, qd, tau, dt, T, record=True)[3:]
                else:
                    q_out, qd_out = plan.step(q, qd, tau, dt)[:2]
                ctx.save_for_backward(q, qd, tau, q_out, qd_out)
                return q_out, qd_out

            @staticmethod
            @once_differentiable
            def backward(ctx, g_q_ambient, g_qd):
                q, qd, tau, q_out, qd_out = ctx.saved_tensors
                plan = ctx.plan
                want = tuple(k for k, needed in zip(names, ctx.needs_input_grad[1:4]) if needed)
                g_q = plan.tangent_cotangent(q_out, g_q_ambient)
                if rollout:
                    got = plan.rollout_vjp(q, qd, tau, ctx.dt, q_out, qd_out, g_q, g_qd, want=want)
                else:
                    got = plan.step_vjp(q, qd, tau, qd_out, ctx.dt, g_q, g_qd, want=want)
                return (None,) + tuple(got.get(k) for k in names) + (None, None)

        Step.__name__ = Step.__qualname__ = "Rollout" if rollout else "Step"
        _ad_functions[key] = Step
    return _ad_functions[key]


def jvp_contract_launch(nv: int, B: int, n_cu: int):
    """(units, grid) of the contraction kernel of id_jvp / fd_jvp for B states on a device with n_cu compute units
    (grbda_jvp_contract_launch; the grid of the float64 launch): units > grid means a workgroup takes a second trip of its grid-stride
    loop"""
    units, grid = c_size_t(), c_size_t()
    _check(lib().grbda_jvp_contract_launch(nv, B, n_cu, byref(units), byref(grid)))
    return units.value, grid.value


def vjp_contract_launch(nv: int, B: int, n_cu: int):
    """(units, grid) of the contraction kernel of id_vjp / fd_vjp for B states on a device with n_cu compute units
    (grbda_vjp_contract_launch): units > grid means a workgroup takes a second trip of its grid-stride loop"""
    units, grid = c_size_t(0), c_size_t(0)
    _check(lib().grbda_vjp_contract_launch(nv, B, n_cu, byref(units), byref(grid)))
    return units.value, grid.value


def device_count() -> int:
    return lib().grbda_device_count()


def spd_bad_pivots(device: int = 0, reset: bool = True) -> int:
    """States whose joint-space inertia was not positive definite in the SPD solves of the derivative entry points since the
    last reset (their results are NaN / Inf); synchronises the device (grbda_spd_bad_pivots)."""
    n = ctypes.c_ulonglong(0)
    _check(lib().grbda_spd_bad_pivots(device, byref(n), 1 if reset else 0))
    return int(n.value)


def contact_solve_launch(n_contacts: int, dtype: str, device: int = -1):
    """(lanes, lds_bytes, grid_cap) of the solve kernel contact_dynamics launches for n_contacts in "f32" / "f64" on `device`
    (grbda_contact_solve_launch); device < 0 touches no device and gives grid_cap for a single CU."""
    lanes, lds, cap = c_int(0), c_size_t(0), c_size_t(0)
    _check(lib().grbda_contact_solve_launch(int(n_contacts), 32 if dtype == "f32" else 64, int(device), byref(lanes), byref(lds), byref(cap)))
    return lanes.value, lds.value, cap.value
