/* grbda_hip_bodies.h -- poses and twists of a listed few bodies.  An extension of grbda_hip.h (same library, same plans, same error codes
 * and conventions).
 *
 * grbda_body_poses_* / grbda_body_twists_* write every body of every state: Xa[B][n_bodies][12], 1.8 KB per state for a humanoid.  A contact
 * pipeline, a task-space controller or a reward function wants two feet, or a hand and a head -- the caller grbda_hip_wrench.h was written
 * for -- and so these entry points take the same short list:
 *
 *     bodies[n]          HOST array of plan body indices: the ones the second axis of Xa, V and f_ext use.  0 <= n <= 16, in any order; a
 *                        body may appear more than once, and together with its ancestors.
 *     Xa_list[B][n][12]  device array, row-major: slot i holds row bodies[i] of grbda_body_poses_*, [E 9 row-major | r 3], the transform
 *                        world -> body in the reference's body axes.
 *     V_list[B][n][12]   device array, row-major: slot i holds row bodies[i] of grbda_body_twists_*, [v 6 | a 6] in the body's own axes, the
 *                        acceleration carrying -gravity.  q holds an implicit cluster's spanning positions, as for grbda_body_twists_*.
 *
 * The kernels visit the listed bodies' ancestors only: a WALK over the union of their root paths, each body once, depth first from the
 * roots, the running pose (or twist) of the root path in registers and the values of branch points in LDS; nothing is read back from global
 * memory.  The walk is built on the host per call and travels by value in the kernel arguments -- no host-to-device copy -- so a call can be
 * captured after one eager call of the same B and n on that stream.  A list whose walk is longer than 19 steps or holds more than 4 branch
 * points at once runs the full kernel into work memory and gathers the listed rows.  grbda_body_list_walk() reports, without a device, the
 * walk's length, the peak number of saved values and the route (0 the walk, 1 full-and-gather); any output pointer may be NULL.
 *
 * Errors are decided on the host before any device call.  GRBDA_EINVAL: a NULL plan, a NULL q / qd / ydd, n outside 0..16, NULL bodies or a
 * NULL output with n > 0, a body index outside the plan, an output that overlaps an input.  n == 0 or B == 0: GRBDA_OK, nothing written.  No
 * plan is refused.
 *
 * The calls enqueue on `stream` and never synchronise.  Gravity is read at launch.  The poses of a walk use no work memory; the twists (their
 * spanning rates) and the full-and-gather route take chunks of the per-(device, stream) work slab, which grbda_plan_release_work() hands
 * back and GRBDA_WORK_MAX_MB bounds.  The _host_ variants take host arrays (allocate, copy and synchronise per call). */
#ifndef GRBDA_HIP_BODIES_H
#define GRBDA_HIP_BODIES_H

#include "grbda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int grbda_body_poses_list_f64(const grbda_plan *plan, const double *q, int n, const int *bodies, double *Xa_list, size_t B, int device,
                              void *stream);
int grbda_body_poses_list_f32(const grbda_plan *plan, const float *q, int n, const int *bodies, float *Xa_list, size_t B, int device,
                              void *stream);
int grbda_body_poses_list_host_f64(const grbda_plan *plan, const double *q, int n, const int *bodies, double *Xa_list, size_t B, int device);
int grbda_body_twists_list_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, int n, const int *bodies,
                               double *V_list, size_t B, int device, void *stream);
int grbda_body_twists_list_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, int n, const int *bodies,
                               float *V_list, size_t B, int device, void *stream);
int grbda_body_twists_list_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, int n, const int *bodies,
                                    double *V_list, size_t B, int device);
int grbda_body_list_walk(const grbda_plan *plan, int n, const int *bodies, int *walk_len, int *max_saved, int *route);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_BODIES_H */
