/* grbda_hip_step_vjp.h -- vector-Jacobian products of a time step and of a trajectory: what a reverse sweep over grbda_integrate_*,
 * grbda_step_* and grbda_rollout_* consumes.  An extension of grbda_hip_vjp.h (same library, same plans, same error codes and conventions).
 *
 * The dense discrete-time matrices of a step are never built: the dynamics part is grbda_aba_vjp_* as it stands, the manifold part a closed
 * form of the six base coordinates, and only [B][nv] vectors enter and leave.
 *
 * Tangent coordinates.  Every cotangent or gradient of a position is [B][nv], along the tangent step grbda_fd_dq_* documents: q_i += d on
 * explicit coordinates; quat += quat x (0, d) / 2 on base entries 0..2 (a rotation by d in body axes); p += R^T d on base entries 3..5 (a
 * translation by d given in body axes).  This is the meaning of grad_q of grbda_aba_vjp_*, so the pieces chain without conversion.
 *
 * One step.  grbda_integrate_* computes qd' = qd + dt ydd and q' = q (+) dt qd'.  With omega' = qd'[base 0..2], v' = qd'[base 3..5],
 * phi = omega' dt, theta = |phi|, E = Exp([phi]x) and J_r(phi) = I - (1 - cos theta) / theta^2 [phi]x + (theta - sin theta) / theta^3 [phi]x^2
 * (the right Jacobian of SO(3)), a tangent perturbation goes through the step as
 *     explicit coordinate   d'   = d + dt dqd'
 *     base rotation         d_r' = E^T d_r + dt J_r dw'
 *     base position         d_p' = E^T (d_p - dt [v']x d_r + dt dv')
 * so the cotangents (g_q', g_qd') of the stepped state pull back to
 *     g_v         = g_qd' + dt g_q'                    explicit coordinates
 *     g_v[omega]  = g_qd'[omega] + dt J_r^T g_r'       base
 *     g_v[v]      = g_qd'[v] + dt E g_p'
 *     grad_ydd    = dt g_v,   grad_qd = g_v
 *     grad_q      = g_q'                               explicit coordinates
 *     grad_q[rot] = E g_r' + dt [v']x E g_p'           base
 *     grad_q[pos] = E g_p'
 * Only qd' and dt enter; q does not.  (1 - cos theta) / theta^2 is evaluated as 2 (sin(theta / 2) / theta)^2; (theta - sin theta) / theta^3 is
 * its series 1/6 - theta^2 / 120 + theta^4 / 5040 below theta = 0.1; at omega' = 0, E = J_r = I (the step is the identity rotation there).
 *
 * All arrays are device arrays, row-major; dt is cast to the precision of the call as grbda_integrate_* casts it.  The calls only enqueue on
 * `stream` and never synchronise.  Every refusal is decided on the host before a device is looked at.  B == 0 (and T == 0 for the rollout):
 * GRBDA_OK with nothing done.
 *
 * grbda_integrate_vjp_*: qd_next[B][nv] holds the velocities AFTER the step, as grbda_integrate_* / grbda_step_* returned them (required).
 * g_q_next, g_qd_next: [B][nv], either may be NULL (zero), not both.  Any output may be NULL, not all.  One kernel launch.
 *
 * grbda_step_vjp_*: exactly this sequence on one stream, bit for bit:
 *     1. grbda_integrate_vjp_*(qd_next, dt, g_q_next, g_qd_next)   -> (i_q, i_qd, g_ydd)
 *     2. grbda_aba_vjp_*(q, qd, tau, g_ydd, step)                  -> (a_q, a_qd, a_tau)
 *     3. grad_q = i_q + a_q, grad_qd = i_qd + a_qd, grad_tau = a_tau   (one rounding per sum, operands in this order)
 * Only the stages the requested outputs need are enqueued: grad_tau alone runs no derivative recursion.  qd_next is an input so that no
 * extra forward dynamics runs to recover omega'.  There is no f_ext, for the reason grbda_aba_vjp_* gives; `step` is used exactly where
 * grbda_aba_vjp_* uses it.  The _host_ variant takes host arrays (allocate, copy and synchronise per call).
 *
 * grbda_rollout_vjp_*: q0[B][nq], qd0[B][nv]: state 0.  q_traj[T][B][nq], qd_traj[T][B][nv]: states 1..T as grbda_rollout_* recorded them.
 * tau, tau_steps in {1, T}: as for grbda_rollout_*.  g_steps in {1, T}: with 1, g_q / g_qd are [B][nv] cotangents of state T only; with T,
 * [T][B][nv] for states 1..T.  Either may be NULL, not both.  Exactly this loop of grbda_step_vjp_*, bit for bit:
 *     lambda_T = (g_q[T], g_qd[T])
 *     for k = T-1 ... 0:  (gamma_q, gamma_qd, gamma_tau_k) = step_vjp(state_k, tau_k, qd_{k+1}, lambda_{k+1})
 *                         lambda_k = (gamma_q + g_q[k], gamma_qd + g_qd[k]) for k >= 1 with g_steps == T, else (gamma_q, gamma_qd)
 * grad_q0 = lambda_0.q, grad_qd0 = lambda_0.qd; grad_tau[tau_steps][B][nv]: row k is gamma_tau_k with tau_steps == T, and the sum
 * ((gamma_tau_{T-1} + gamma_tau_{T-2}) + ...) + gamma_tau_0 in that order with tau_steps == 1.  Any output may be NULL, not all.
 * The running adjoints and intermediate vectors, ten [B][nv] arrays, live in a per-(device, stream) slab of their own next to the one
 * grbda_aba_vjp_* carves for itself; it is not chunked (it is the size of the inputs) and grbda_plan_release_work() hands it back.  The
 * call can be captured after one eager call of the same B and T on the stream; a call that would have to grow the slab while its stream
 * is capturing returns GRBDA_EINVAL, like the others.
 *
 * GRBDA_EINVAL: a NULL plan, a missing required pointer, no output asked for, both cotangents NULL, dt not finite, T < 0, tau_steps or
 * g_steps outside {1, T}, step <= 0 where a difference route needs it, any output overlapping an input or another output.
 * GRBDA_EUNSUPPORTED (text in grbda_last_error()): every plan grbda_step_* refuses (a roll-pitch-yaw base, implicit clusters on the
 * spanning-tree route) and EVERY plan with an implicit-loop cluster: the Jacobian of the Newton re-projection is not built.  Every other
 * plan grbda_step_* and grbda_aba_vjp_* both accept is accepted, explicit plans on the spanning-tree route and nv > 64 included (they take
 * the difference route of grbda_aba_vjp_*). */
#ifndef GRBDA_HIP_STEP_VJP_H
#define GRBDA_HIP_STEP_VJP_H

#include "grbda_hip_vjp.h"

#ifdef __cplusplus
extern "C" {
#endif

int grbda_integrate_vjp_f64(const grbda_plan *plan, const double *qd_next, double dt, const double *g_q_next, const double *g_qd_next,
                            double *grad_q, double *grad_qd, double *grad_ydd, size_t B, int device, void *stream);
int grbda_integrate_vjp_f32(const grbda_plan *plan, const float *qd_next, double dt, const float *g_q_next, const float *g_qd_next,
                            float *grad_q, float *grad_qd, float *grad_ydd, size_t B, int device, void *stream);
int grbda_step_vjp_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *qd_next, double dt,
                       const double *g_q_next, const double *g_qd_next, double step, double *grad_q, double *grad_qd, double *grad_tau,
                       size_t B, int device, void *stream);
int grbda_step_vjp_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, const float *qd_next, double dt,
                       const float *g_q_next, const float *g_qd_next, double step, float *grad_q, float *grad_qd, float *grad_tau,
                       size_t B, int device, void *stream);
int grbda_step_vjp_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *qd_next, double dt,
                            const double *g_q_next, const double *g_qd_next, double step, double *grad_q, double *grad_qd,
                            double *grad_tau, size_t B, int device);
int grbda_rollout_vjp_f64(const grbda_plan *plan, const double *q0, const double *qd0, const double *q_traj, const double *qd_traj,
                          const double *tau, int tau_steps, double dt, int T, const double *g_q, const double *g_qd, int g_steps,
                          double step, double *grad_q0, double *grad_qd0, double *grad_tau, size_t B, int device, void *stream);
int grbda_rollout_vjp_f32(const grbda_plan *plan, const float *q0, const float *qd0, const float *q_traj, const float *qd_traj,
                          const float *tau, int tau_steps, double dt, int T, const float *g_q, const float *g_qd, int g_steps,
                          double step, float *grad_q0, float *grad_qd0, float *grad_tau, size_t B, int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_STEP_VJP_H */
