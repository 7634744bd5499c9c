/* grbda_hip_jvp.h -- Jacobian-vector products of the inverse and the forward dynamics, of integrate and of a time step: the forward-mode
 * half of grbda_hip_vjp.h / grbda_hip_step_vjp.h, what a tangent-linear model, a Gauss-Newton product J^T J v, a Krylov solve on the
 * linearised dynamics or the line-search derivative of a rollout consume.  An extension of grbda_hip_step_vjp.h (same library, same plans,
 * same error codes and conventions).
 *
 * As there, no [B][nv][nv] array leaves the library and the dense discrete-time matrices of a step are never built: A^T lambda is
 * grbda_step_vjp_*, A dx + B du is grbda_step_jvp_*.  The matrices of grbda_rnea_derivatives_* stay inside a chunked work slab of
 * 2 nv^2 + O(nv) scalars per state of the chunk; there is no factorisation and no solve.
 *
 * Every tangent is [B][nv], a device array, row-major.  A position tangent lies along the tangent step grbda_fd_dq_* documents (the
 * coordinates of grad_q in the two VJP headers, so that <g, JVP(u)> = <VJP(g), u> pairs up without conversion).  A tangent pointer may be
 * NULL, meaning zero; not all tangents of a call may be NULL.
 *
 * grbda_rnea_jvp_*: dtau = d tau / d q dq + d tau / d qd dqd + H dydd at (q, qd, ydd).  The two matrices are those of
 * grbda_rnea_derivatives_*, written into the slab and contracted along their rows (jvp_kernels.hip); a matrix is built only when its tangent
 * is given.  H dydd = RNEA(q, 0, dydd) - RNEA(q, 0, 0), both without gravity.  dydd alone runs no derivative recursion; no dydd runs no pair.
 *
 * grbda_aba_jvp_*: chunk by chunk,
 *     ydd  = ABA(q, qd, tau)                                         (into `ydd` when given: a batch that takes one chunk gets the bits of grbda_aba_*)
 *     r    = dtau - d tau / d q dq - d tau / d qd dqd  at ydd
 *     dydd = ABA(q, 0, r) - ABA(q, 0, 0)                             (both without gravity)
 * dtau alone runs neither the first ABA (unless `ydd` is asked for) nor the recursion.  `ydd` is NULL or [B][nv].
 *
 * `step` is used exactly where grbda_rnea_derivatives_* uses it: by plans off the analytic route, when dq is given.  There is no f_ext
 * argument, for the reason given there.
 *
 * grbda_integrate_jvp_*: the forward map of the step whose transpose grbda_hip_step_vjp.h derives.  With omega', v' the base entries of
 * qd_next, phi = omega' dt, E = Exp([phi]x) and J_r as defined there,
 *     dqd'  = dqd + dt dydd
 *     d'    = d + dt dqd'                                explicit coordinates
 *     d_r'  = E^T d_r + dt J_r domega'                   base rotation
 *     d_p'  = E^T (d_p - dt [v']x d_r + dt dv')          base position
 * with the coefficients evaluated by the device function grbda_integrate_vjp_* evaluates them with (the series below theta = 0.1;
 * E = J_r = I at omega' = 0).  qd_next[B][nv]: the velocities AFTER the step (required).  Either output may be NULL, not both.  One launch.
 *
 * grbda_step_jvp_*: exactly grbda_aba_jvp_*(q, qd, tau, dq, dqd, dtau) -> dydd followed by grbda_integrate_jvp_*(qd_next, dt, dq, dqd, dydd)
 * on one stream, bit for bit; dydd lives in a [B][nv] work array.  qd_next is an input so that no extra forward dynamics runs, as in
 * grbda_step_vjp_*.
 *
 * Not here: a rollout JVP (a loop over grbda_step_jvp_* the caller can write); several directions per call (stack them along the batch);
 * torch.autograd.forward_ad hooks; the C++ facade.
 *
 * Errors are decided on the host before a device is looked at.  GRBDA_EINVAL: a NULL plan, a missing state input, all tangents NULL, no
 * output, an output that overlaps an input or another output, dt not finite, step <= 0 where a difference route needs it.
 * GRBDA_EUNSUPPORTED from grbda_integrate_jvp_* / grbda_step_jvp_*: every plan grbda_step_vjp_* refuses (a roll-pitch-yaw base, any implicit
 * cluster).  grbda_rnea_jvp_* / grbda_aba_jvp_* accept every plan their VJP twins accept.  B == 0: GRBDA_OK.
 *
 * The calls enqueue on `stream` and never synchronise; they can be captured after one eager call of the same B on that stream; gravity is
 * read at launch.  Beyond the scratch slab they allocate a work slab per (device, stream), which GRBDA_WORK_MAX_MB bounds and
 * grbda_plan_release_work() hands back.  The _host_ variants take host arrays (allocate, copy and synchronise per call). */
#ifndef GRBDA_HIP_JVP_H
#define GRBDA_HIP_JVP_H

#include "grbda_hip_step_vjp.h"

#ifdef __cplusplus
extern "C" {
#endif

int grbda_rnea_jvp_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, const double *dq, const double *dqd,
                       const double *dydd, double step, double *dtau_out, size_t B, int device, void *stream);
int grbda_rnea_jvp_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, const float *dq, const float *dqd,
                       const float *dydd, double step, float *dtau_out, size_t B, int device, void *stream);
int grbda_rnea_jvp_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, const double *dq, const double *dqd,
                            const double *dydd, double step, double *dtau_out, size_t B, int device);
int grbda_aba_jvp_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *dq, const double *dqd,
                      const double *dtau, double step, double *dydd_out, double *ydd, size_t B, int device, void *stream);
int grbda_aba_jvp_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, const float *dq, const float *dqd,
                      const float *dtau, double step, float *dydd_out, float *ydd, size_t B, int device, void *stream);
int grbda_aba_jvp_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *dq, const double *dqd,
                           const double *dtau, double step, double *dydd_out, double *ydd, size_t B, int device);
int grbda_integrate_jvp_f64(const grbda_plan *plan, const double *qd_next, double dt, const double *dq, const double *dqd, const double *dydd,
                            double *dq_next, double *dqd_next, size_t B, int device, void *stream);
int grbda_integrate_jvp_f32(const grbda_plan *plan, const float *qd_next, double dt, const float *dq, const float *dqd, const float *dydd,
                            float *dq_next, float *dqd_next, size_t B, int device, void *stream);
int grbda_step_jvp_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *qd_next, double dt,
                       const double *dq, const double *dqd, const double *dtau, double step, double *dq_next, double *dqd_next, size_t B,
                       int device, void *stream);
int grbda_step_jvp_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, const float *qd_next, double dt,
                       const float *dq, const float *dqd, const float *dtau, double step, float *dq_next, float *dqd_next, size_t B, int device,
                       void *stream);
int grbda_step_jvp_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *qd_next, double dt,
                            const double *dq, const double *dqd, const double *dtau, double step, double *dq_next, double *dqd_next, size_t B,
                            int device);
/* The launch of the contraction kernel (jvp_kernels.hip) for nb states of a plan with nv velocities on a device with n_cu compute units:
 * `units` of work (packs of floor(64 / nv) states when nv <= 32, one state when nv <= 64, blocks of 64 rows beyond) and the persistent
 * `grid` of one-wavefront workgroups that walks them -- units > grid: some workgroup takes a second trip.  The grid is the fp64 launch's: at
 * most sixteen workgroups per compute unit and no more than its LDS holds tiles of; an fp32 tile is half the bytes, so from nv = 18 on the
 * fp32 launch may be larger (below, the two are the same).  Either pointer may be NULL.  No device call is made. */
int grbda_jvp_contract_launch(int nv, size_t nb, int n_cu, size_t *units, size_t *grid);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_JVP_H */
