/* grbda_hip_contact_step.h -- scheduled bilateral contacts: a per-state active set, the contact-aware step and the rollout.  An extension of
 * grbda_hip.h (same library, same plans, same error codes and conventions).
 *
 * grbda_contact_dynamics_* / grbda_contact_impulse_* take ONE contact list for the whole batch; a batch of walking robots has another stance
 * set in every state and at every step.  Here the contacts are described as there -- n_contacts in 1..8, HOST arrays bodies[n] and
 * offsets[n][3] -- and every state carries a mask:
 *
 *     active[B]   device int32 array.  Bit c set: contact c is closed in that state.  Bits at n and above are ignored.
 *
 * All other arrays are device arrays, row-major.  With S the contacts whose bit is set in a state:
 *
 * grbda_contact_dynamics_active_*   the solve of grbda_contact_dynamics_* (no f_ext) on the sub-list S:
 *         (J_S H^-1 J_S^T + damping I) lambda_S = a_des - kd p_dot - p_ddot(ydd_free),     ydd = ydd_free + H^-1 J_S^T lambda_S
 *     p_dot: the points' world velocities at (q, qd); kd >= 0, finite.  a_des[B][n][3] may be NULL (zero).  lambda[B][n][3] is exactly 0 for
 *     the contacts not in S.  An empty S: ydd == ydd_free, bit for bit.  ydd_free may be NULL.
 * grbda_contact_impulse_active_*    grbda_contact_impulse_* on the sub-list S.  impulse[B][n][3] is exactly 0 off S; qd_next has the bits
 *     of qd where S is empty -- it is qd + 0, so a coordinate of qd that holds -0.0 comes back as +0.0 (and a plan on the
 *     spanning-tree route, whose forward dynamics always carry gravity, keeps qd to rounding only).  qd_next == qd
 *     (equal pointers) is allowed.  v_des may be NULL.
 * grbda_contact_step_*              per state, closing = active & ~prev_active:
 *         1  qd+ = contact_impulse_active(q, qd, closing ? active : 0, v_des = 0, restitution, damping)  -- when anything closes, the impact is
 *            solved with EVERY closed contact as a constraint.  prev_active == NULL: the stage is not enqueued at all, qd+ = qd, and
 *            `impulse` must be NULL.  With prev_active given, `impulse` may still be NULL (the impulses are then not kept).
 *         2  (ydd, lambda) = contact_dynamics_active(q, qd+, tau, active, a_des = NULL, kd, damping)
 *         3  (q_next, qd_next, ok) = grbda_integrate_*(q, qd+, ydd, dt) with the max_iter / tol of grbda_step_*
 *     q_next == q and qd_next == qd are allowed; `ok` may be NULL.
 * grbda_contact_rollout_*           T calls of grbda_contact_step_* in place on (q, qd), bit for bit.  tau[tau_steps][B][nv] and
 *     active[active_steps][B], tau_steps and active_steps each 1 (held) or T.  Step t takes prev_active = active[t - 1]; step 0 takes
 *     active_prev, and a NULL active_prev stands for active[0] (nothing closes).  A held mask is its own predecessor after step 0.
 *     with_impulses == 0 gives every step a NULL prev_active.  ydd_work[B][nv] is work space; q_traj[T][B][nq], qd_traj[T][B][nv] and
 *     lambda_traj[T][B][n][3] may each be NULL; ok[B] (may be NULL) is the AND over the steps.
 *
 * Errors are decided on the host before anything is enqueued.  GRBDA_EINVAL: a NULL plan or required array (`active` is required), n outside
 * 1..8, a body index outside the plan, kd or damping negative or not finite, restitution outside [0, 1] or not finite, a dt that is not
 * finite, T < 0, tau_steps or active_steps not in {1, T}, a non-NULL impulse with a NULL prev_active, overlapping arrays.
 * GRBDA_EUNSUPPORTED: exactly what grbda_step_* refuses.  B == 0 or T == 0: GRBDA_OK, nothing done.
 *
 * Per chunk of states the dynamics are: the forward dynamics without wrenches; the poses and twists of the LISTED contact bodies
 * (grbda_hip_bodies.h); the inverse operational-space inertia of the contact frames as grbda_contact_dynamics_* takes it; one solve kernel;
 * the forward dynamics with the sparse body-frame wrench list (grbda_hip_wrench.h), on whatever route that call takes.  No array over all
 * bodies is written.  A state whose matrix is not positive definite gets NaN on its active contacts and is counted by
 * grbda_spd_bad_pivots(); a state with an empty set is never counted.
 *
 * The calls enqueue on `stream` and never synchronise.  Work memory: the scratch slab and a per-(device, stream) pool of their own, which
 * GRBDA_WORK_MAX_MB bounds and grbda_plan_release_work() hands back (a fallback route of the sparse-wrench call takes its chunk from the
 * general work pool, as that call does).  A call can be captured after one eager call of the same B, n (and T) on the stream.  Gravity is
 * read at launch.  grbda_contact_step_host_f64 takes host arrays (allocates, copies and synchronises per call). */
#ifndef GRBDA_HIP_CONTACT_STEP_H
#define GRBDA_HIP_CONTACT_STEP_H

#include <stdint.h>

#include "grbda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int grbda_contact_dynamics_active_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, int n_contacts,
                                      const int *bodies, const double *offsets, const int32_t *active, const double *a_des, double kd,
                                      double damping, double *ydd, double *lambda, double *ydd_free, size_t B, int device, void *stream);
int grbda_contact_dynamics_active_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, int n_contacts,
                                      const int *bodies, const double *offsets, const int32_t *active, const float *a_des, double kd,
                                      double damping, float *ydd, float *lambda, float *ydd_free, size_t B, int device, void *stream);
int grbda_contact_impulse_active_f64(const grbda_plan *plan, const double *q, const double *qd, int n_contacts, const int *bodies,
                                     const double *offsets, const int32_t *active, const double *v_des, double restitution, double damping,
                                     double *qd_next, double *impulse, size_t B, int device, void *stream);
int grbda_contact_impulse_active_f32(const grbda_plan *plan, const float *q, const float *qd, int n_contacts, const int *bodies,
                                     const double *offsets, const int32_t *active, const float *v_des, double restitution, double damping,
                                     float *qd_next, float *impulse, size_t B, int device, void *stream);
int grbda_contact_step_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, int n_contacts, const int *bodies,
                           const double *offsets, const int32_t *active, const int32_t *prev_active, double kd, double restitution,
                           double damping, double dt, double *ydd, double *lambda, double *impulse, double *q_next, double *qd_next,
                           int32_t *ok, size_t B, int device, void *stream);
int grbda_contact_step_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, int n_contacts, const int *bodies,
                           const double *offsets, const int32_t *active, const int32_t *prev_active, double kd, double restitution,
                           double damping, double dt, float *ydd, float *lambda, float *impulse, float *q_next, float *qd_next, int32_t *ok,
                           size_t B, int device, void *stream);
int grbda_contact_step_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, int n_contacts,
                                const int *bodies, const double *offsets, const int32_t *active, const int32_t *prev_active, double kd,
                                double restitution, double damping, double dt, double *ydd, double *lambda, double *impulse, double *q_next,
                                double *qd_next, int32_t *ok, size_t B, int device);
int grbda_contact_rollout_f64(const grbda_plan *plan, double *q, double *qd, const double *tau, int tau_steps, int n_contacts,
                              const int *bodies, const double *offsets, const int32_t *active, int active_steps, const int32_t *active_prev,
                              int with_impulses, double kd, double restitution, double damping, double dt, int T, double *ydd_work,
                              double *q_traj, double *qd_traj, double *lambda_traj, int32_t *ok, size_t B, int device, void *stream);
int grbda_contact_rollout_f32(const grbda_plan *plan, float *q, float *qd, const float *tau, int tau_steps, int n_contacts, const int *bodies,
                              const double *offsets, const int32_t *active, int active_steps, const int32_t *active_prev, int with_impulses,
                              double kd, double restitution, double damping, double dt, int T, float *ydd_work, float *q_traj,
                              float *qd_traj, float *lambda_traj, int32_t *ok, size_t B, int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_CONTACT_STEP_H */
