/* grbda_hip_vjp.h -- vector-Jacobian products of the inverse and the forward dynamics: what reverse-mode differentiation asks of a
 * dynamics engine.  An extension of grbda_hip.h (same library, same plans, same error codes and conventions).
 *
 * grbda_rnea_derivatives_* and grbda_fd_derivatives_* hand out [B][nv][nv] matrices.  A reverse sweep (a loss on ydd = FD(q, qd, tau) in
 * policy learning, the adjoint of a trajectory optimisation, identification through the inverse dynamics) wants ONE row combination of
 * them per state, g^T d out / d x, and 3 B nv^2 scalars are a lot to allocate for that (a million JVRC-1 states in fp32: 17 GB).  Here the
 * matrices stay inside a chunked work slab of 2 nv^2 + O(nv) scalars per state of the chunk and only [B][nv] vectors leave the library:
 *
 *     inverse dynamics   g^T d tau / d q,  g^T d tau / d qd    the matrices of grbda_rnea_derivatives_* at (q, qd, ydd), contracted
 *                        g^T d tau / d ydd = (H g)^T           H g = RNEA(q, 0, g) - RNEA(q, 0, 0), no matrix at all
 *     forward dynamics   g^T d ydd / d tau = mu^T              mu = H^-1 g = ABA(q, 0, g) - ABA(q, 0, 0) (H is symmetric; the exact
 *                                                              difference form of grbda_fd_dtau_*): no factorisation, no solve
 *                        g^T d ydd / d q  = -mu^T d tau / d q  the inverse-dynamics matrices at ydd = FD(q, qd, tau), contracted with mu
 *                        g^T d ydd / d qd = -mu^T d tau / d qd
 *
 * Arrays are device arrays, row-major.  g_* is [B][nv], the cotangent of the output; grad_* are [B][nv],
 *     grad_x[b][j] = sum_i g[b][i] d out_i / d x_j,
 * grad_q along the tangent step grbda_fd_dq_* documents -- nv entries, not nq: the meaning of the columns of the matrices above.  Any
 * grad_* may be NULL, not all of them (for grbda_aba_vjp_* `ydd` does not count).  grbda_aba_vjp_*: `ydd` is NULL or [B][nv] and receives
 * FD(q, qd, tau), which the call computes anyway whenever grad_q or grad_qd is asked for (chunk by chunk: a batch that takes one chunk gets the
 * bits of grbda_aba_* of that batch).  `step` is used exactly where grbda_rnea_derivatives_* uses it: by plans off the analytic route, for
 * grad_q.  There is no f_ext argument, for the reason given there.
 *
 * Errors are decided on the host before anything is enqueued.  GRBDA_EINVAL: a NULL plan, a NULL input, no output asked for, an output
 * that overlaps an input or another output, step <= 0 where a difference route needs it.  B == 0: GRBDA_OK.
 *
 * The calls enqueue on `stream` and never synchronise; they can be captured after one eager call of the same B on that stream; gravity is
 * read at launch.  Asking for grad_tau (grad_ydd) alone never runs the derivative recursion; asking for neither skips the two H g launches
 * of the inverse-dynamics side.  The work slab is kept per (device, stream) like the others and grbda_plan_release_work() hands it back;
 * GRBDA_WORK_MAX_MB bounds it.  The _host_ variants take host arrays (allocate, copy and synchronise per call). */
#ifndef GRBDA_HIP_VJP_H
#define GRBDA_HIP_VJP_H

#include "grbda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int grbda_rnea_vjp_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, const double *g_tau, double step,
                       double *grad_q, double *grad_qd, double *grad_ydd, size_t B, int device, void *stream);
int grbda_rnea_vjp_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, const float *g_tau, double step,
                       float *grad_q, float *grad_qd, float *grad_ydd, size_t B, int device, void *stream);
int grbda_rnea_vjp_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, const double *g_tau, double step,
                            double *grad_q, double *grad_qd, double *grad_ydd, size_t B, int device);
int grbda_aba_vjp_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *g_ydd, double step,
                      double *grad_q, double *grad_qd, double *grad_tau, double *ydd, size_t B, int device, void *stream);
int grbda_aba_vjp_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, const float *g_ydd, double step,
                      float *grad_q, float *grad_qd, float *grad_tau, float *ydd, size_t B, int device, void *stream);
int grbda_aba_vjp_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *g_ydd, double step,
                           double *grad_q, double *grad_qd, double *grad_tau, double *ydd, size_t B, int device);
/* The launch of the contraction kernel (vjp_kernels.hip) for nb states of a plan with nv velocities on a device with n_cu compute units:
 * `units` of work (packs of floor(64 / nv) states when nv <= 32, one state when nv <= 64, blocks of 64 columns beyond) and the persistent
 * `grid` of one-wavefront workgroups that walks them -- units > grid: some workgroup takes a second trip.  Either pointer may be NULL.
 * No device call is made. */
int grbda_vjp_contract_launch(int nv, size_t nb, int n_cu, size_t *units, size_t *grid);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_VJP_H */
