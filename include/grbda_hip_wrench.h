/* grbda_hip_wrench.h -- forward and inverse dynamics with external wrenches on a short list of bodies.  An extension of grbda_hip.h (same
 * library, same plans, same error codes and conventions).
 *
 * grbda_aba_* / grbda_rnea_* take external forces as a dense array f_ext[B][n_bodies][6], which is more than twice the bytes of q, qd and tau
 * together for a humanoid, and sends every model to the general interpreter kernel.  A simulator has forces on two feet.  The reference's
 * own interface is a short list of (body, force) pairs -- TreeModel::setExternalForces takes ExternalForceAndBodyIndexPair -- and so is this
 * one:
 *
 *     bodies[n]        HOST array of plan body indices: the ones the second axis of f_ext and grbda_contact_* use.  0 <= n <= 16.  A body
 *                      may appear more than once; its wrenches add in list order.
 *     wrench[B][n][6]  device array, row-major: the spatial force [moment 3; force 3] acting on bodies[i], component order of f_ext.
 *     frame            GRBDA_WRENCH_BODY: expressed in the body's own frame, at its origin.
 *                      GRBDA_WRENCH_WORLD: exactly the meaning of a row of f_ext (world axes, moment about the world origin).
 *
 * n == 0 is the plain grbda_aba_* / grbda_rnea_* call with f_ext = NULL, bit for bit; `wrench` and `bodies` may then be NULL.
 *
 * Routes.  A plan whose one-wavefront chain program is plain (no differential, no generic cluster) runs a wrench-carrying instantiation of
 * the chain kernels when every listed body is a link body, a link of a leaf pair or the floating base of that program: a body-frame wrench
 * is one subtraction from a bias force (forward dynamics) or a body force (inverse dynamics) the kernel already holds.  World-frame
 * wrenches are rotated with the body poses first (one poses launch and one small kernel per chunk).  Everything else -- another plan, a
 * listed rotor, GRBDA_NO_CHAIN, a batch the launch rule gives to latency mode -- scatters the list into a dense world-frame chunk of work
 * memory and runs the dense route of grbda_aba_* / grbda_rnea_*.  grbda_wrench_kernel_name() reports the kernel the dynamics of a call would
 * launch (as grbda_kernel_name: algo 0 forward, 1 inverse dynamics; precision 32 or 64); no launch is made.
 *
 * Errors are decided on the host before any device call.  GRBDA_EINVAL: a NULL plan, a NULL q / qd / tau / ydd, n outside 0..16, a frame
 * that is neither constant, NULL bodies or wrench with n > 0, a body index outside the plan, an output that overlaps an input.  B == 0:
 * GRBDA_OK.
 *
 * The calls enqueue on `stream` and never synchronise.  The body list travels by value in the kernel arguments -- no host-to-device copy
 * per call -- so a call can be captured after one eager call of the same B and n on that stream.  The chain route with body-frame wrenches
 * uses no work memory; the other routes take chunks of the per-(device, stream) work slab, which grbda_plan_release_work() hands back and
 * GRBDA_WORK_MAX_MB bounds.  The _host_ variants take host arrays (allocate, copy and synchronise per call). */
#ifndef GRBDA_HIP_WRENCH_H
#define GRBDA_HIP_WRENCH_H

#include "grbda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GRBDA_WRENCH_BODY 0
#define GRBDA_WRENCH_WORLD 1

int grbda_aba_wrench_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, int n, const int *bodies,
                         const double *wrench, int frame, double *ydd, size_t B, int device, void *stream);
int grbda_aba_wrench_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, int n, const int *bodies,
                         const float *wrench, int frame, float *ydd, size_t B, int device, void *stream);
int grbda_rnea_wrench_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, int n, const int *bodies,
                          const double *wrench, int frame, double *tau, size_t B, int device, void *stream);
int grbda_rnea_wrench_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, int n, const int *bodies,
                          const float *wrench, int frame, float *tau, size_t B, int device, void *stream);
int grbda_aba_wrench_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, int n, const int *bodies,
                              const double *wrench, int frame, double *ydd, size_t B, int device);
int grbda_rnea_wrench_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, int n, const int *bodies,
                               const double *wrench, int frame, double *tau, size_t B, int device);
int grbda_wrench_kernel_name(const grbda_plan *plan, int algo, int precision, int n, const int *bodies, int frame, size_t B, int device,
                             char *buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_WRENCH_H */
