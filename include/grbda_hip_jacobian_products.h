/* grbda_hip_jacobian_products.h -- the products J v and J^T f with the frame Jacobians of a listed few body frames, J itself never written.
 * An extension of grbda_hip.h (same library, same plans, same error codes and conventions), next to grbda_hip_jacobians.h: the J here is, by
 * definition, the J of grbda_frame_jacobians_* for the same plan, q, bodies, offsets and frame.  J is 6 n nv scalars per state; its two
 * products are 6 n and nv.
 *
 *     bodies[n], offsets[n][3], frame
 *                        exactly as for grbda_frame_jacobians_*: HOST arrays, 0 <= n <= 16, a body may repeat, offsets in the reference's
 *                        body axes (NULL: all zero), GRBDA_WRENCH_BODY or GRBDA_WRENCH_WORLD (grbda_hip_wrench.h).
 *     v[B][nv]           device array: a joint-space direction, which need not be the state's velocity.
 *     Jv[B][n][6]        Jv[b][i] = J_i(q_b) v_b, [angular 3 ; linear 3]: the velocity of frame i for the joint velocity v.  v and Jv are
 *                        both NULL, or neither is.
 *     f[B][n][6]         device array: per frame a wrench [moment 3 ; force 3] in the same frame as J_i -- at the point, in the body's axes or
 *                        in world axes.
 *     JTf[B][nv]         JTf[b] = sum over i of J_i(q_b)^T f[b][i]: the joint torques that balance the wrenches.  A frame listed twice
 *                        contributes twice.  Every one of the nv entries is written; columns on no listed frame's root path as 0.0.  f and
 *                        JTf are both NULL, or neither is.
 *
 * The plan's gravity does not enter.  q holds an implicit cluster's spanning positions, as for grbda_frame_jacobians_*.
 *
 * The route is the one grbda_frame_jacobians_route() reports for the list: there are no caps of this header's own.  Route 0, the walk: one
 * kernel walks the listed bodies' ancestors in world coordinates about the world origin.  For J v it carries the running twist of the root
 * path next to the running pose and stores a frame's six values when it reaches the frame.  For J^T f it turns each frame's wrench into a
 * world wrench, walks again and takes, per ancestor joint, the dot product of the joint's world-frame axis with the sum of the wrenches
 * below it.  Per lane the walk holds 18 values per saved branch point (pose and twist) and 6 per frame, at most 18 saved + 6 n; the
 * Jacobian walk holds (saved + n) x 12, and fewer branch points are held at once than there are listed frames (saved < n), so the LDS budget
 * of the Jacobian walk -- at most 10 frames and saved values together -- covers this walk too.  Route 0 takes no work memory.  Route 1, every
 * other list: J v is the velocity half of grbda_body_twists_list_* at (q, v, 0), one row per state, moved to the point and turned by a
 * finishing kernel; J^T f forms J chunk by chunk in the work slab by route 1 of grbda_frame_jacobians_* and contracts it there.
 *
 * Errors are decided on the host before any device call.  GRBDA_EINVAL: a NULL plan or q, n outside 0..16, NULL bodies with n > 0, a body
 * index outside the plan, a frame that is neither constant, Jv and JTf both NULL, one of v and Jv without the other, one of f and JTf
 * without the other, an output that overlaps an input or the other output.  n == 0 or B == 0: GRBDA_OK, nothing written.  No plan is refused.
 *
 * The calls enqueue on `stream` and never synchronise; the lists travel in the kernel arguments, so a call can be captured after one eager
 * call of the same B and n on that stream.  Route 1 takes chunks of the per-(device, stream) work slab, which grbda_plan_release_work()
 * hands back and GRBDA_WORK_MAX_MB bounds.  The _host_ variant takes host arrays (allocate, copy and synchronise per call). */
#ifndef GRBDA_HIP_JACOBIAN_PRODUCTS_H
#define GRBDA_HIP_JACOBIAN_PRODUCTS_H

#include "grbda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int grbda_frame_jacobian_products_f64(const grbda_plan *plan, const double *q, const double *v, const double *f, int n, const int *bodies,
                                      const double *offsets, int frame, double *Jv, double *JTf, size_t B, int device, void *stream);
int grbda_frame_jacobian_products_f32(const grbda_plan *plan, const float *q, const float *v, const float *f, int n, const int *bodies,
                                      const double *offsets, int frame, float *Jv, float *JTf, size_t B, int device, void *stream);
int grbda_frame_jacobian_products_host_f64(const grbda_plan *plan, const double *q, const double *v, const double *f, int n, const int *bodies,
                                           const double *offsets, int frame, double *Jv, double *JTf, size_t B, int device);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_JACOBIAN_PRODUCTS_H */
