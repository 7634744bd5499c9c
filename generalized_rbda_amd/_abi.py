"""The C signatures of include/grbda_hip.h as ctypes sees them: SIGNATURES, exported name -> (restype, argtypes).

Written by hand, not read from the header: an installed package does not ship include/.  tests/test_abi_table_cpu.py holds
the table to the header, parameter by parameter.  `lib()` applies it to every symbol in one loop.
"""
from ctypes import POINTER, c_char_p, c_double, c_int, c_size_t, c_ulonglong, c_void_p

# P: any pointer ctypes need not look into -- the plan, a device or host array, a stream (an integer address, a ctypes array,
# byref(...), bytes and None all pass)
P, I, Z, D = c_void_p, c_int, c_size_t, c_double
BODIES, OFFSETS = POINTER(c_int), POINTER(c_double)  # the host arrays of a contact set (and the one offset[3] of the test force)
TAIL = (Z, I, P)                                     # size_t B, int device, void *stream

# grbda_<stem>_f64 and grbda_<stem>_f32: the two differ in nothing ctypes can see.  The plan comes first everywhere.
_PAIRS = {
    "aba": (P, P, P, P, P, P, *TAIL),                                    # q qd tau f_ext ydd
    "rnea": (P, P, P, P, P, P, *TAIL),                                   # q qd ydd f_ext tau
    "bias": (P, P, P, P, P, *TAIL),                                      # q qd f_ext out
    "mass_matrix": (P, P, P, *TAIL),                                     # q H
    "fd_dtau": (P, P, P, *TAIL),                                         # q Hinv
    "fd_dqd": (P, P, P, P, P, *TAIL),                                    # q qd tau J
    "fd_dq": (P, P, P, P, D, P, *TAIL),                                  # q qd tau step J
    "fd_derivatives": (P, P, P, P, P, P, P, *TAIL),                      # q qd tau dq dqd dtau
    "rnea_derivatives": (P, P, P, P, D, P, P, P, *TAIL),                 # q qd ydd step dq dqd dydd
    "project_positions": (P, P, P, Z, I, D, I, P),                       # q ok B max_iter tol device stream
    "state_to_independent": (P, P, P, P, P, P, P, P, P, Z, D, I, P),     # pos vel q_in qd_in q qd status cond B tol device stream
    "spanning": (P, P, P, P, P, P, *TAIL),                               # q qd ydd qd_span qdd_span
    "integrate": (P, P, P, P, D, P, P, P, I, D, *TAIL),                  # q qd ydd dt q_next qd_next ok max_iter tol
    "step": (P, P, P, P, P, D, P, P, P, P, *TAIL),                       # q qd tau f_ext dt ydd q_next qd_next ok
    "rollout": (P, P, P, P, I, D, I, P, P, P, P, *TAIL),                 # q qd tau tau_steps dt T ydd_work q_traj qd_traj ok
    "body_poses": (P, P, P, *TAIL),                                      # q Xa
    "body_twists": (P, P, P, P, P, *TAIL),                               # q qd ydd V
    "apply_test_force": (P, P, I, OFFSETS, P, P, P, *TAIL),              # q body offset force lambda_inv dstate
    "inv_osim": (P, P, I, BODIES, OFFSETS, P, P, *TAIL),                 # q n bodies offsets Linv J
    "contact_points": (P, P, P, P, I, BODIES, OFFSETS, P, P, P, *TAIL),  # q qd ydd n bodies offsets pos vel acc
    "contact_dynamics": (P, P, P, P, P, I, BODIES, OFFSETS, P, D, P, P, P, *TAIL),  # q qd tau f_ext n bodies offsets a_des damping ydd lambda ydd_free
    "contact_impulse": (P, P, P, I, BODIES, OFFSETS, P, D, D, P, P, *TAIL),         # q qd n bodies offsets v_des restitution damping qd_next impulse
    "energy": (P, P, P, P, P, *TAIL),                                    # q qd kinetic potential
    "centroidal": (P, P, P, P, P, P, P, P, *TAIL),                       # q qd ydd com com_vel h hdot
    "centroidal_matrix": (P, P, P, *TAIL),                               # q A
    "aba_sharded": (P, P, P, P, P, Z, I),                                # q qd tau ydd B n_gpus (host arrays)
    "rnea_sharded": (P, P, P, P, P, Z, I),
    "aba_sharded_dev": (P, I, P, P, P, P, P, P, P, P),                   # n_gpus devices q qd tau ydd B streams gathered
    "rnea_sharded_dev": (P, I, P, P, P, P, P, P, P, P),
}

# grbda_<stem>_host_f64: the device form without the trailing void *stream
_HOST = ("aba", "rnea", "mass_matrix", "fd_derivatives", "rnea_derivatives", "project_positions", "integrate", "step", "body_poses",
         "body_twists", "apply_test_force", "inv_osim", "contact_points", "contact_dynamics", "contact_impulse", "energy", "centroidal")

_SINGLES = {
    "strerror": (I,),
    "last_error": (),
    "plan_from_blob": (P, Z, POINTER(c_void_p)),
    "plan_from_urdf": (c_char_p, I, POINTER(c_void_p)),
    "urdf_to_blob": (POINTER(c_char_p), I, I, P, Z, POINTER(c_size_t)),
    "plan_free": (P,),
    "plan_release_work": (P, POINTER(c_ulonglong)),
    "plan_dims": (P, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)),
    "plan_set_gravity": (P, POINTER(c_double)),
    "plan_get_gravity": (P, POINTER(c_double)),
    "plan_blob": (P, POINTER(c_void_p), POINTER(c_size_t)),
    "plan_info": (P, P),                                                 # (PlanInfo lives in the package's __init__)
    "plan_span_dims": (P, POINTER(c_int)),
    "plan_total_mass": (P, POINTER(c_double)),
    "state_input_dims": (P, P, P, POINTER(c_int), POINTER(c_int)),
    "state_to_independent_host_f64": (P, P, P, P, P, P, P, Z, D, I),     # (no status, no cond: not the device form)
    "spd_bad_pivots": (I, POINTER(c_ulonglong), I),
    "kernel_name": (P, I, I, Z, I, P, Z),                                # kind precision B device buf cap
    "contact_solve_launch": (I, I, I, POINTER(c_int), POINTER(c_size_t), POINTER(c_size_t)),
    "time_kernel": (P, I, I, P, P, P, P, Z, I, P, I, P),                 # kind precision q qd x out B device stream iters avg_ms
    "device_count": (),
}
_RESTYPE = {"grbda_strerror": c_char_p, "grbda_last_error": c_char_p, "grbda_plan_free": None}  # every other: int

SIGNATURES = {"grbda_" + name: args for name, args in _SINGLES.items()}
for _stem, _args in _PAIRS.items():
    SIGNATURES[f"grbda_{_stem}_f64"] = SIGNATURES[f"grbda_{_stem}_f32"] = _args
for _stem in _HOST:
    SIGNATURES[f"grbda_{_stem}_host_f64"] = _PAIRS[_stem][:-1]
SIGNATURES = {name: (_RESTYPE.get(name, c_int), args) for name, args in SIGNATURES.items()}

# include/grbda_hip_vjp.h, the vector-Jacobian products: a table of its own (SIGNATURES is the table of grbda_hip.h and nothing else);
# `lib()` applies it after SIGNATURES, and tests/test_vjp_args_cpu.py holds it to that header the same way
_VJP_PAIRS = {
    "rnea_vjp": (P, P, P, P, P, D, P, P, P, *TAIL),                      # q qd ydd g_tau step grad_q grad_qd grad_ydd
    "aba_vjp": (P, P, P, P, P, D, P, P, P, P, *TAIL),                    # q qd tau g_ydd step grad_q grad_qd grad_tau ydd
}
VJP_SIGNATURES = {"grbda_vjp_contract_launch": (I, Z, I, POINTER(c_size_t), POINTER(c_size_t))}  # nv nb n_cu units grid
for _stem, _args in _VJP_PAIRS.items():
    VJP_SIGNATURES[f"grbda_{_stem}_f64"] = VJP_SIGNATURES[f"grbda_{_stem}_f32"] = _args
    VJP_SIGNATURES[f"grbda_{_stem}_host_f64"] = _args[:-1]
VJP_SIGNATURES = {name: (c_int, args) for name, args in VJP_SIGNATURES.items()}

# include/grbda_hip_step_vjp.h, the vector-Jacobian products of integrate, step and rollout: the third table, applied by `lib()` after the
# other two; tests/test_step_vjp_args_cpu.py holds it to that header
_STEP_VJP_PAIRS = {
    "integrate_vjp": (P, P, D, P, P, P, P, P, *TAIL),                    # qd_next dt g_q_next g_qd_next grad_q grad_qd grad_ydd
    "step_vjp": (P, P, P, P, P, D, P, P, D, P, P, P, *TAIL),             # q qd tau qd_next dt g_q_next g_qd_next step grad_q grad_qd grad_tau
    "rollout_vjp": (P, P, P, P, P, P, I, D, I, P, P, I, D, P, P, P, *TAIL),  # q0 qd0 q_traj qd_traj tau tau_steps dt T g_q g_qd g_steps step grad_q0 grad_qd0 grad_tau
}
STEP_VJP_SIGNATURES = {}
for _stem, _args in _STEP_VJP_PAIRS.items():
    STEP_VJP_SIGNATURES[f"grbda_{_stem}_f64"] = STEP_VJP_SIGNATURES[f"grbda_{_stem}_f32"] = _args
STEP_VJP_SIGNATURES["grbda_step_vjp_host_f64"] = _STEP_VJP_PAIRS["step_vjp"][:-1]
STEP_VJP_SIGNATURES = {name: (c_int, args) for name, args in STEP_VJP_SIGNATURES.items()}

# include/grbda_hip_wrench.h, forward and inverse dynamics with sparse body wrenches: the fourth table, applied by `lib()` after the other
# three; tests/test_wrench_args_cpu.py holds it to that header
_WRENCH_PAIRS = {
    "aba_wrench": (P, P, P, P, I, BODIES, P, I, P, *TAIL),               # q qd tau n bodies wrench frame ydd
    "rnea_wrench": (P, P, P, P, I, BODIES, P, I, P, *TAIL),              # q qd ydd n bodies wrench frame tau
}
WRENCH_SIGNATURES = {"grbda_wrench_kernel_name": (P, I, I, I, BODIES, I, Z, I, P, Z)}  # algo precision n bodies frame B device buf len
for _stem, _args in _WRENCH_PAIRS.items():
    WRENCH_SIGNATURES[f"grbda_{_stem}_f64"] = WRENCH_SIGNATURES[f"grbda_{_stem}_f32"] = _args
    WRENCH_SIGNATURES[f"grbda_{_stem}_host_f64"] = _args[:-1]
WRENCH_SIGNATURES = {name: (c_int, args) for name, args in WRENCH_SIGNATURES.items()}

# include/grbda_hip_jvp.h, the Jacobian-vector products: a table of its own, applied by `lib()` after the others;
# tests/test_jvp_args_cpu.py holds it to that header
_JVP_PAIRS = {
    "rnea_jvp": (P, P, P, P, P, P, P, D, P, *TAIL),                      # q qd ydd dq dqd dydd step dtau_out
    "aba_jvp": (P, P, P, P, P, P, P, D, P, P, *TAIL),                    # q qd tau dq dqd dtau step dydd_out ydd
    "integrate_jvp": (P, P, D, P, P, P, P, P, *TAIL),                    # qd_next dt dq dqd dydd dq_next dqd_next
    "step_jvp": (P, P, P, P, P, D, P, P, P, D, P, P, *TAIL),             # q qd tau qd_next dt dq dqd dtau step dq_next dqd_next
}
JVP_SIGNATURES = {"grbda_jvp_contract_launch": (I, Z, I, POINTER(c_size_t), POINTER(c_size_t))}  # nv nb n_cu units grid
for _stem, _args in _JVP_PAIRS.items():
    JVP_SIGNATURES[f"grbda_{_stem}_f64"] = JVP_SIGNATURES[f"grbda_{_stem}_f32"] = _args
    if _stem != "integrate_jvp":
        JVP_SIGNATURES[f"grbda_{_stem}_host_f64"] = _args[:-1]
JVP_SIGNATURES = {name: (c_int, args) for name, args in JVP_SIGNATURES.items()}

# include/grbda_hip_bodies.h, poses and twists of a listed few bodies: a table of its own, applied by `lib()` after the others;
# tests/test_body_list_args_cpu.py holds it to that header
_BODIES_PAIRS = {
    "body_poses_list": (P, P, I, BODIES, P, *TAIL),                      # q n bodies Xa_list
    "body_twists_list": (P, P, P, P, I, BODIES, P, *TAIL),               # q qd ydd n bodies V_list
}
BODIES_SIGNATURES = {"grbda_body_list_walk": (P, I, BODIES, POINTER(c_int), POINTER(c_int), POINTER(c_int))}  # n bodies walk_len max_saved route
for _stem, _args in _BODIES_PAIRS.items():
    BODIES_SIGNATURES[f"grbda_{_stem}_f64"] = BODIES_SIGNATURES[f"grbda_{_stem}_f32"] = _args
    BODIES_SIGNATURES[f"grbda_{_stem}_host_f64"] = _args[:-1]
BODIES_SIGNATURES = {name: (c_int, args) for name, args in BODIES_SIGNATURES.items()}

# include/grbda_hip_jacobians.h, frame Jacobians and their drift at a listed few body frames: a table of its own, applied by `lib()` after
# the others; tests/test_frame_jacobians_args_cpu.py holds it to that header
_JACOBIAN_PAIR = (P, P, P, I, BODIES, OFFSETS, I, P, P, *TAIL)           # q qd n bodies offsets frame J drift
JACOBIAN_SIGNATURES = {
    "grbda_frame_jacobians_f64": _JACOBIAN_PAIR,
    "grbda_frame_jacobians_f32": _JACOBIAN_PAIR,
    "grbda_frame_jacobians_host_f64": _JACOBIAN_PAIR[:-1],
    "grbda_frame_jacobians_route": (P, I, BODIES, POINTER(c_int), POINTER(c_int), POINTER(c_int)),  # n bodies route walk_len max_saved
}
JACOBIAN_SIGNATURES = {name: (c_int, args) for name, args in JACOBIAN_SIGNATURES.items()}

# include/grbda_hip_jacobian_products.h, J v and J^T f at a listed few body frames: a table of its own, applied by `lib()` after the others;
# tests/test_jacobian_products_args_cpu.py holds it to that header
_JACOBIAN_PRODUCT_PAIR = (P, P, P, P, I, BODIES, OFFSETS, I, P, P, *TAIL)  # q v f n bodies offsets frame Jv JTf
JACOBIAN_PRODUCT_SIGNATURES = {
    "grbda_frame_jacobian_products_f64": _JACOBIAN_PRODUCT_PAIR,
    "grbda_frame_jacobian_products_f32": _JACOBIAN_PRODUCT_PAIR,
    "grbda_frame_jacobian_products_host_f64": _JACOBIAN_PRODUCT_PAIR[:-1],
}
JACOBIAN_PRODUCT_SIGNATURES = {name: (c_int, args) for name, args in JACOBIAN_PRODUCT_SIGNATURES.items()}

# include/grbda_hip_contact_step.h, scheduled contacts -- per-state active sets, the contact-aware step, the rollout: a table of its own,
# applied by `lib()` after the others; tests/test_contact_step_args_cpu.py holds it to that header
_CONTACT_STEP_PAIRS = {
    "contact_dynamics_active": (P, P, P, P, I, BODIES, OFFSETS, P, P, D, D, P, P, P, *TAIL),  # q qd tau n bodies offsets active a_des kd damping ydd lambda ydd_free
    "contact_impulse_active": (P, P, P, I, BODIES, OFFSETS, P, P, D, D, P, P, *TAIL),         # q qd n bodies offsets active v_des restitution damping qd_next impulse
    # q qd tau n bodies offsets active prev_active kd restitution damping dt ydd lambda impulse q_next qd_next ok
    "contact_step": (P, P, P, P, I, BODIES, OFFSETS, P, P, D, D, D, D, P, P, P, P, P, P, *TAIL),
    # q qd tau tau_steps n bodies offsets active active_steps active_prev with_impulses kd restitution damping dt T ydd_work q_traj qd_traj lambda_traj ok
    "contact_rollout": (P, P, P, P, I, I, BODIES, OFFSETS, P, I, P, I, D, D, D, D, I, P, P, P, P, P, *TAIL),
}
CONTACT_STEP_SIGNATURES = {}
for _stem, _args in _CONTACT_STEP_PAIRS.items():
    CONTACT_STEP_SIGNATURES[f"grbda_{_stem}_f64"] = CONTACT_STEP_SIGNATURES[f"grbda_{_stem}_f32"] = _args
CONTACT_STEP_SIGNATURES["grbda_contact_step_host_f64"] = _CONTACT_STEP_PAIRS["contact_step"][:-1]
CONTACT_STEP_SIGNATURES = {name: (c_int, args) for name, args in CONTACT_STEP_SIGNATURES.items()}
