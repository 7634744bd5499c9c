/* grbda_hip_jacobians.h -- frame Jacobians and their drift at a listed few body frames.  An extension of grbda_hip.h (same library, same
 * plans, same error codes and conventions), next to grbda_hip_bodies.h, which gives the VALUES at such a list; this header gives the MAP:
 * J(q) with v_frame = J qd, and the drift Jdot qd that completes a_frame = J ydd + Jdot qd (the reference's contactJacobianBodyFrame,
 * contactJacobianWorldFrame and updateContactPointJacobians).  Pure kinematics: no inertias, no H^-1, no unit-wrench batch.
 *
 *     bodies[n]          HOST array of plan body indices, 0 <= n <= 16, in any order; a body may repeat, also with another offset.
 *     offsets[n][3]      HOST array of doubles: a point fixed in the body, in the reference's body axes, as for grbda_inv_osim_*.  NULL: all
 *                        zero.
 *     frame              GRBDA_WRENCH_BODY (grbda_hip_wrench.h): the body's axes, origin at the point -- the J of grbda_inv_osim_*.
 *                        GRBDA_WRENCH_WORLD: world axes, origin at the point, the rows [E^T w ; E^T (v + w x o)].
 *     J[B][n][6][nv]     device array, row-major, each frame [angular 3 ; linear 3].  Columns of coordinates that are not on the frame's
 *                        root path are structural zeros and are written as 0.0: the caller need not clear the array.
 *     drift[B][n][6]     Jdot qd in the same frame: the frame's acceleration at ydd = 0 without gravity.  Body axes: the spatial
 *                        acceleration moved to the point, [al ; a + al x o].  World axes: [E^T al ; E^T (a + al x o + w x (v + w x o))],
 *                        whose linear rows are the acc of grbda_contact_points_* at ydd = 0 and zero gravity.  The plan's gravity does not
 *                        enter.
 *
 * J or drift may be NULL, not both; qd is read for the drift only and may be NULL without it.  q holds an implicit cluster's spanning
 * positions, as for grbda_body_twists_*.
 *
 * Route 0, the walk: lists whose root paths hold only the floating base and explicit clusters of one to four coordinates (revolute joints,
 * rotors, pairs, triples, generic explicit clusters), with a walk of at most 19 bodies and at most 10 frames and saved branch points
 * together.  One kernel walks the listed bodies' ancestors twice -- the frames' poses, then every ancestor joint's axis in world coordinates,
 * turned into each frame below it -- and writes J once.  Route 1, every other list (an implicit cluster on a root path, the spanning-tree
 * route, a list past those caps): column k is the velocity half of grbda_body_twists_list_* at (q, e_k, 0), over the expanded batch of nv
 * rows per state, and a finishing kernel moves, turns and stores.  The drift comes on both routes from the listed twists at (q, qd, 0)
 * with a zero root acceleration.  grbda_frame_jacobians_route() reports, without a device, the route, the walk's length and the peak number
 * of saved values; any output pointer may be NULL.
 *
 * Errors are decided on the host before any device call.  GRBDA_EINVAL: a NULL plan or q, n outside 0..16, NULL bodies with n > 0, a body
 * index outside the plan, a frame that is neither constant, J and drift both NULL, drift without qd, an output that overlaps an input or
 * the other output.  n == 0 or B == 0: GRBDA_OK, nothing written.  No plan is refused.
 *
 * The calls enqueue on `stream` and never synchronise; the lists travel in the kernel arguments, so a call can be captured after one eager
 * call of the same B and n on that stream.  Route 1 and the drift take chunks of the per-(device, stream) work slab, which
 * grbda_plan_release_work() hands back and GRBDA_WORK_MAX_MB bounds.  The _host_ variant takes host arrays (allocate, copy and synchronise
 * per call). */
#ifndef GRBDA_HIP_JACOBIANS_H
#define GRBDA_HIP_JACOBIANS_H

#include "grbda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int grbda_frame_jacobians_f64(const grbda_plan *plan, const double *q, const double *qd, int n, const int *bodies, const double *offsets,
                              int frame, double *J, double *drift, size_t B, int device, void *stream);
int grbda_frame_jacobians_f32(const grbda_plan *plan, const float *q, const float *qd, int n, const int *bodies, const double *offsets,
                              int frame, float *J, float *drift, size_t B, int device, void *stream);
int grbda_frame_jacobians_host_f64(const grbda_plan *plan, const double *q, const double *qd, int n, const int *bodies, const double *offsets,
                                   int frame, double *J, double *drift, size_t B, int device);
int grbda_frame_jacobians_route(const grbda_plan *plan, int n, const int *bodies, int *route, int *walk_len, int *max_saved);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_JACOBIANS_H */
