// devplan.h -- kernel argument block and launcher declarations shared by kernels.hip and capi.cpp
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include "plan.h"
#include "walk.h"

namespace grbda_hip {

// wavefronts (one-wavefront workgroups) whose dynamic LDS fits a CU: gfx950 hands out its 160 KiB in granules of 1 280 bytes, so a
// kernel asking for 13 312 bytes holds 11 workgroups per CU, not 12 -- and a persistent grid sized for 12 leaves every twelfth
// workgroup waiting for a slot until another has finished ALL its tiles (measured: four_bar forward dynamics 0.103 ms at 12 per CU,
// 0.074 ms at 10; profiles/r5_single_cluster_kernels.txt)
inline size_t lds_workgroups_per_cu(size_t lds_bytes)
{
    if (lds_bytes == 0) return 32;
    constexpr size_t granule = 1280;
    return (160u * 1024u) / ((lds_bytes + granule - 1) / granule * granule);
}


template <class T>
struct DevPlan {
    const Step *steps;
    int n_steps;
    const ClusterRec *clusters;
    const BodyRec *bodies;
    const T *consts;
    const int32_t *cints;  // integer payload of implicit constraints
    const int32_t *acc_k;  // ABA: per step, K block to prefetch (Layout::acc_k)
    int nq, nv;
    int n_lds_slots, n_glb_slots;
    int lds_bytes;  // dynamic LDS actually allocated per wave (slot store / input staging area)
    int ori_repr;
    int general;   // launch the general kernel variant: implicit-loop clusters and / or external forces
    int split;     // the layout keeps [K | y0] blocks in the global slab and everything else in LDS (Slots<T, true>)
    int n_bodies;
    const T *fext; // [B][n_bodies][6] world-frame spatial forces or nullptr (TreeModel::setExternalForces)
    unsigned long long *bad_count;  // aba_kernel: per-device counter of states with a pivot of D that is not positive (grbda_spd_bad_pivots)
    T a_root[6];  // -gravity (ClusterTreeDynamics.cpp:147)
};

template <class T>
hipError_t launch_aba(const DevPlan<T> &P, const T *q, const T *qd, const T *tau, T *ydd, size_t B, T *scratch,
                      int grid, size_t lds_bytes, hipStream_t stream, bool two_waves_per_simd);
template <class T>
hipError_t launch_rnea(const DevPlan<T> &P, const T *q, const T *qd, const T *ydd, T *tau, size_t B, T *scratch,
                       int grid, size_t lds_bytes, hipStream_t stream);
template <class T>
hipError_t launch_project(const DevPlan<T> &P, int n_clusters, T *q, int32_t *ok, size_t B, int max_iter, T tol,
                          T *scratch, int grid, size_t lds_bytes, hipStream_t stream);
// bit c of pos / vel: cluster c's positions / velocities are given as SPANNING coordinates (state_kernel)
constexpr int kStateFlagWords = 4;
struct StateFlags {
    uint64_t pos[kStateFlagWords], vel[kStateFlagWords];
};
template <class T>
hipError_t launch_state(const DevPlan<T> &P, int n_clusters, const StateFlags &F, const T *q_in, const T *qd_in, int in_nq, int in_nv,
                        T *q_out, T *qd_out, int32_t *status, T *gmax, size_t B, T tol, T *scratch, int grid, size_t lds_bytes,
                        hipStream_t stream);
template <class T>
hipError_t launch_spanning(const DevPlan<T> &P, int n_clusters, int n_span, const T *q, const T *qd, const T *ydd,
                           T *qd_span, T *qdd_span, size_t B, T *scratch, int grid, size_t lds_bytes,
                           hipStream_t stream);
// integrate_kernel: the wave's slab holds kIntegrateLocalRows rows behind the plan's global slots (per-lane cluster positions)
constexpr int kIntegrateLocalRows = kMaxClusterBodies;
template <class T>
hipError_t launch_integrate(const DevPlan<T> &P, int n_clusters, const T *q, const T *qd, const T *ydd, T dt, T *q_next, T *qd_next,
                            int32_t *ok, int ok_and, size_t B, int max_iter, T tol, T *scratch, int grid, size_t lds_bytes, hipStream_t stream);
template <class T>
hipError_t launch_poses(const DevPlan<T> &P, int n_clusters, const T *q, T *Xa, size_t B, int grid, hipStream_t stream);
template <class T>
hipError_t launch_twists(const DevPlan<T> &P, int n_clusters, int n_span, const T *q, const T *qd_span, const T *qdd_span, T *V, size_t B,
                         int grid, hipStream_t stream);
hipError_t set_max_dynamic_lds();

// kernel argument block of the chain-structured fast path (chain_kernels.hip; plan.h, ChainProgram)
template <class T>
struct ChainDev {
    const ChainSeg *segs;
    const ChainLink *links;
    const ChainPair *pairs;
    const ChainFree *frees;
    const ChainDiff *diffs;
    int n_diffs;
    const ChainGen *gens;          // generic clusters (plan.h, ChainGen; gen_segments.h)
    const ChainGenBody *gbodies;
    int n_gens;
    const int32_t *cints;
    const T *consts;
    int n_segs;
    int nq, nv;
    int n_glb_slots;
    int lds_bytes;
    int ori_repr;
    int sv_global;  // ChainProgram::sv_global
    int out_lds;    // ChainProgram::out_lds
    // aba_chain_kernel only (capi.cpp, run_chain): bit 0 -- the program starts with the floating base's forward segment, whose whole work is
    // "own velocity to LDS slot stage_lds_v": the tile prologue does it from the staged block (no slab round trip) and the segment is
    // skipped; bit 1 -- the base's acceleration segment follows its backward segment directly: the backward segment finishes it with y0
    // in registers (no slab round trip) and the acceleration segment is skipped
    int fuse, stage_lds_v, stage_v_index;
    // per-device counter of states whose D = S^T IA S had a pivot that is not positive (grbda_spd_bad_pivots; deriv_kernels.hip owns the word)
    unsigned long long *bad_count;
    T a_root[6];
};
// aba_chain_kernel<float, 2, kModeInReg>: the plain program (no differentials, no generic clusters) with every lane's q, qd and tau in
// three register arrays of kInRegCols entries instead of slab rows (chain_kernels.hip, ChainMemR).  Which launch runs it -- ONE rule,
// read by launch_aba_chain and by grbda_kernel_name: fp32, [sin, cos, v] blocks in LDS, at most kInRegCols columns per input.
constexpr int kInRegCols = 32;
constexpr int kModeInReg = 3;
inline bool chain_inputs_in_registers(size_t elem, int n_gens, int n_diffs, int sv_global, int nq, int nv)
{
    return elem == 4 && n_gens == 0 && n_diffs == 0 && !sv_global && nq <= kInRegCols && nv <= kInRegCols;
}
// Its lanes fetch their own rows of q, qd and tau from global memory (devmath.h, load_row_regs): 16-byte loads at the element's own
// alignment plus a narrow tail, so any row size and any base offset a tensor of that element type can have will do.
// The rows (of kWave scalars) of a wavefront's slab in a launch of aba_chain_kernel -- ONE rule, read by the kernel for its pointers and by
// the host for the allocation (capi.cpp, run_chain).  Staged inputs: [q: nq][qd: nv][tau: nv, the result rows once tau is dead][global
// slots].  Inputs in registers: no input rows -- [global slots][result rows: nv, only when the plan keeps no result rows in LDS; that kernel
// keeps its results in registers and leaves them unwritten -- the rule and its host-side check, tests/cpp/chain_slab_check.cpp, stand as they were].
struct ChainSlabRows {
    int glb;    // first row of the global slots
    int out;    // first of the result rows (out_lds < 0)
    int total;  // rows per wavefront
};
__host__ __device__ inline ChainSlabRows chain_slab_rows(bool in_registers, int nq, int nv, int n_glb_slots, int out_lds)
{
    if (!in_registers) return {nq + 2 * nv, nq + nv, nq + 2 * nv + n_glb_slots};
    return {0, out_lds < 0 ? n_glb_slots : 0, n_glb_slots + (out_lds < 0 ? nv : 0)};
}
template <class T>
hipError_t launch_aba_chain(const ChainDev<T> &P, const T *q, const T *qd, const T *tau, T *ydd, size_t B, T *scratch, int grid,
                            size_t lds_bytes, hipStream_t stream);
// latency mode: a tile per workgroup of n_waves = 2 (or, fp32, 4) wavefronts (chain_kernels.hip, aba_chain_lm_kernel)
template <class T>
hipError_t launch_aba_chain_lm(const ChainDev<T> &P, const T *q, const T *qd, const T *tau, T *ydd, size_t B, T *scratch, int grid,
                               size_t lds_bytes, hipStream_t stream, int n_waves);
hipError_t set_max_dynamic_lds_chain();
// single-cluster programs (ChainProgram::single_gen; chain_kernels.hip, aba_gen1_kernel): P.lds_bytes = the work area, lds_bytes = work
// area + nq + 2 nv rows of staged inputs
template <class T>
hipError_t launch_aba_gen1(const ChainDev<T> &P, int n, int implicit, const T *q, const T *qd, const T *tau, T *ydd, size_t B, int grid,
                           size_t lds_bytes, hipStream_t stream);
template <class T>
int gen1_waves_per_simd(int n);

template <class T>
struct RneaChainDev {
    const RneaSeg *segs;
    const RneaLink *links;
    const RneaPair *pairs;
    const RneaFree *frees;
    const RneaDiff *diffs;
    int n_diffs;
    const ChainGen *gens;          // generic clusters (gen_rnea_segments.h)
    const ChainGenBody *gbodies;
    int n_gens;
    const int32_t *cints;
    const T *consts;
    int n_segs;
    int nq, nv;
    int n_glb_slots;  // RneaChainProgram::n_glb
    int lds_bytes;
    int ori_repr;
    T a_root[6];
};
template <class T>
hipError_t launch_rnea_chain(const RneaChainDev<T> &P, const T *q, const T *qd, const T *ydd, T *tau, size_t B, T *scratch, int grid,
                             size_t lds_bytes, hipStream_t stream);
// latency mode: a tile per workgroup of n_waves = 2 or 4 wavefronts (chain_kernels.hip, rnea_chain_lm_kernel)
template <class T>
hipError_t launch_rnea_chain_lm(const RneaChainDev<T> &P, const T *q, const T *qd, const T *ydd, T *tau, size_t B, T *scratch, int grid, size_t lds_bytes,
                                hipStream_t stream, int n_waves);

// Sparse body wrenches of one call (include/grbda_hip_wrench.h): capi.cpp builds it from the caller's host list and it travels by value
// in the kernel arguments, like ContactSet.  body[i] is a plan body index, -1 from entry n on; w holds the BODY-frame wrenches
// [B][n][6] ([moment 3; force 3] at the body's origin) in the REFERENCE's body axes; canon: two bits per entry, BodyRec::canon_axis of the
// body -- the plan's frame has that axis on z (plan.cpp, canonical joint axes), component i of a plan-frame vector is component
// (i + canon_axis + 1) % 3 of the reference-frame one, and the chain kernels permute as they load.  The wrench-carrying chain kernels (chain_kernels.hip, unit 4:
// aba_chain_wrench_kernel, rnea_chain_wrench_kernel) run the plain one-wavefront program -- no differentials, no generic clusters, [sin,
// cos, v] blocks in LDS -- and subtract a listed body's wrench from its bias force (forward dynamics) or its body force (inverse dynamics).
constexpr int kMaxWrenches = 16;
template <class T>
struct WrenchList {
    int n;
    int body[kMaxWrenches];
    unsigned canon;
    const T *w;
};
template <class T>
hipError_t launch_aba_chain_wrench(const ChainDev<T> &P, const WrenchList<T> &W, const T *q, const T *qd, const T *tau, T *ydd, size_t B, T *scratch,
                                   int grid, size_t lds_bytes, hipStream_t stream);
template <class T>
hipError_t launch_rnea_chain_wrench(const RneaChainDev<T> &P, const WrenchList<T> &W, int base_body, const T *q, const T *qd, const T *ydd, T *tau,
                                    size_t B, T *scratch, int grid, size_t lds_bytes, hipStream_t stream);  // base_body: ChainFree::body or -1
hipError_t set_max_dynamic_lds_chain_wrench();
// The frames of the sparse wrenches (wrench_kernels.hip), over nb states with the poses Xa [nb][n][12] of the listed bodies in list order:
// to_body: out[nb][n][6] = Xa_body w (world -> body, in front of the chain route); otherwise the fallback's dense world-frame chunk
// fext[nb][n_bodies][6] (zeroed by the caller) += w, rotated body -> world when from_body is set (Xa may be null when it is not).
template <class T>
hipError_t launch_wrench_to_body(const WrenchList<T> &W, const T *Xa, size_t nb, T *out, hipStream_t stream);
template <class T>
hipError_t launch_wrench_scatter(const WrenchList<T> &W, const T *Xa, int from_body, int n_bodies, size_t nb, T *fext, hipStream_t stream);

// Poses and twists of a listed few bodies (include/grbda_hip_bodies.h; body_list_kernels.hip): the walk of walk.h (BodyWalkStep, the caps) with
// what the kernels need beside the steps.
template <class T>
struct BodyWalk {
    int n_steps, n_list, n_saved;  // steps, outputs per state, peak number of saved values
    int nq, n_span, ori_repr;
    const T *consts;
    T a_root[6];  // -gravity
    uint8_t slot[kMaxBodyList];
    BodyWalkStep step[kMaxWalk];
};
static_assert(sizeof(BodyWalk<double>) <= 2048, "the walk travels in the kernel arguments");
// out[nb][n_list][12]; qd_span / qdd_span: the spanning rates of spanning_kernel, [nb][n_span]
template <class T>
hipError_t launch_body_poses_list(const BodyWalk<T> &W, const T *q, T *out, size_t nb, int grid, hipStream_t stream);
template <class T>
hipError_t launch_body_twists_list(const BodyWalk<T> &W, const T *q, const T *qd_span, const T *qdd_span, T *out, size_t nb, int grid, hipStream_t stream);
// the walk's fallback (walk.h, BodyList): out[nb][n][12] = full[nb][n_bodies][12] at the listed bodies
template <class T>
hipError_t launch_body_gather(const BodyList &L, const T *full, int n_bodies, size_t nb, T *out, hipStream_t stream);

// Frame Jacobians and their drift at a listed few body frames (include/grbda_hip_jacobians.h; frame_jacobian_kernels.hip).  A frame is the
// body-fixed point off[i] of body bodies[i]; FrameSet travels by value like ContactSet: the offsets in the REFERENCE's body axes, and per
// frame the bit mask of the velocity columns on its root path (every other column of J is a structural zero; all ones when nv > 128).
template <class T>
struct FrameSet {
    int n, world;  // world: 0 the body's axes, 1 world axes (origin at the point either way)
    T off[kMaxBodyList][3];
    uint64_t cols[kMaxBodyList][kJacMaskWords];
};
// The walk of route 0 (walk.h, JacWalkStep).  off: the offsets in the PLAN's (canonical) body axes.
template <class T>
struct JacWalk {
    int n_steps, n_list, n_saved;
    int nq, nv, ori_repr, world;
    const T *consts;
    T off[kMaxBodyList][3];
    uint64_t cols[kMaxBodyList][kJacMaskWords];
    uint8_t canon[kMaxBodyList];
    JacWalkStep step[kMaxWalk];
};
static_assert(sizeof(JacWalk<double>) <= 2048, "the walk travels in the kernel arguments");
// J[nb][n][6][nv], every entry written once (route 0)
template <class T>
hipError_t launch_frame_jacobian_walk(const JacWalk<T> &W, const T *q, T *J, size_t nb, int grid, hipStream_t stream);
// route 1: Vx[nb * nv][n][12], the listed twists of the expanded batch (row (b, k): state b at the unit velocity e_k); Xa[nb][n][12] the
// listed poses (read for world frames only, may be null otherwise) -> J[nb][n][6][nv]
template <class T>
hipError_t launch_frame_jacobian_columns(const FrameSet<T> &F, const T *Vx, const T *Xa, int nv, size_t nb, T *J, hipStream_t stream);
// V[nb][n][12], the listed twists at (q, qd, 0) without gravity; Xa as above -> drift[nb][n][6]
template <class T>
hipError_t launch_frame_drift(const FrameSet<T> &F, const T *V, const T *Xa, size_t nb, T *drift, hipStream_t stream);

// The products with those Jacobians, J never formed (include/grbda_hip_jacobian_products.h; frame_product_kernels.hip).  Route 0: the
// walk of JacWalk again; v[nb][nv] -> Jv[nb][n][6], f[nb][n][6] -> JTf[nb][nv], every entry written; either pair may be null.  Its LDS is
// (18 n_saved + 6 n_list) rows of kWave lanes, never more than the (n_saved + n_list) x 12 of the Jacobian walk: n_saved < n_list.
template <class T>
hipError_t launch_frame_product_walk(const JacWalk<T> &W, const T *q, const T *v, const T *f, T *Jv, T *JTf, size_t nb, int grid, hipStream_t stream);
// route 1: V[nb][n][12], the listed twists at (q, v, 0); Xa as above -> Jv[nb][n][6]
template <class T>
hipError_t launch_frame_jv(const FrameSet<T> &F, const T *V, const T *Xa, size_t nb, T *Jv, hipStream_t stream);
// route 1: J[nb][n][6][nv], f[nb][n][6] -> JTf[nb][nv]
template <class T>
hipError_t launch_frame_jtf(const T *J, const T *f, int n, int nv, size_t nb, T *JTf, hipStream_t stream);

// single-cluster programs (RneaChainProgram::single_gen; chain_kernels.hip, rnea_gen1_kernel): P.lds_bytes = the work area, lds_bytes =
// work area + nq + 2 nv rows of staged inputs
template <class T>
hipError_t launch_rnea_gen1(const RneaChainDev<T> &P, int n, int implicit, const T *q, const T *qd, const T *ydd, T *tau, size_t B, int grid,
                            size_t lds_bytes, hipStream_t stream);
template <class T>
int rnea_gen1_waves_per_simd(int n);

// inverse operational-space inertia by force propagation along the contacts' ancestor paths (chain_kernels.hip,
// osim_chain_kernel).  Built per call on the host (capi.cpp) and passed by value.
constexpr int kOsimMaxContacts = 8;
constexpr int kOsimMaxPath = 12;  // clusters between a contact body and the root
enum OsimStepKind : int32_t { OSIM_LINK = 0, OSIM_PAIR_LINK1 = 1, OSIM_PAIR_LINK2 = 2, OSIM_FREE = 3, OSIM_DIFF_LINK1 = 4, OSIM_DIFF_LINK2 = 5 };
struct OsimStep {
    int16_t kind;
    int16_t rec;      // index into links[] / pairs[] / frees[]
    int16_t v_index;  // first velocity coordinate of the cluster
    int16_t w_row;    // first of the cluster's rows in the contact's W block (n rows)
};
template <class T>
struct OsimArgs {
    int n_contacts;
    int want_J;
    int path_len[kOsimMaxContacts];
    int n_rows[kOsimMaxContacts];                        // rows of W of each contact (sum of n over its path)
    int common[kOsimMaxContacts][kOsimMaxContacts];      // number of trailing W rows two contacts share (their common ancestors)
    OsimStep path[kOsimMaxContacts][kOsimMaxPath];       // leaf side first
    T K0[kOsimMaxContacts][36];                          // wrench on the contact body (plan frame) per unit contact wrench, row-major
    int w_base;                                          // first slab row (after the chain program's rows) of the W blocks
    int w_stride;                                        // rows per contact
    // applyTestForce mode (one contact): a force per state, given in world coordinates at the contact point; results
    // lambda_inv[B] = f^T (J H^-1 J^T) f and dstate[B][nv] = H^-1 J^T f.  perm: plan-frame axis i of the contact body is the
    // reference's axis perm[i] (canonical joint axes, plan.cpp)
    int test_force;
    int perm[3];
    const T *force;
    T *lambda_inv;
    T *dstate;
};
template <class T>
hipError_t launch_osim_chain(const ChainDev<T> &P, const OsimArgs<T> &A, const T *q, const T *zeros, T *Linv, T *J, size_t B,
                             T *scratch, int grid, size_t lds_bytes, hipStream_t stream);

// contact points of one call (capi.cpp builds it from the caller's host arrays; passed to the kernels by value): point off[c], body
// coordinates, fixed in body body[c]
constexpr int kMaxContacts = 8;
template <class T>
struct ContactSet {
    int n;
    int body[kMaxContacts];
    T off[kMaxContacts][3];
};
// contact-point kinematics and the per-state contact solve (contact_kernels.hip).  Xa: body poses, V: body twists, g: the plan's gravity
// (linear part).  launch_contact_points: pos / vel / acc [nb][n][3], any of them null (V may be null when only pos is asked for).
// launch_contact_solve: Linv [nb][6 n][6 n], V the twists at the unconstrained accelerations, a_des [nb][n][3] or null, fext_in
// [nb][n_bodies][6] or null; writes lambda [nb][n][3] and the wrench rows fext_out [nb][n_bodies][6].
template <class T>
hipError_t launch_contact_points(const ContactSet<T> &cs, const T *Xa, const T *V, int n_bodies, const T g[3], size_t nb, T *pos, T *vel, T *acc,
                                 hipStream_t stream);
template <class T>
hipError_t launch_contact_solve(const ContactSet<T> &cs, const T *Linv, const T *Xa, const T *V, const T *a_des, const T *fext_in, int n_bodies,
                                T mu, const T g[3], size_t nb, T *lambda, T *fext_out, unsigned long long *bad_count, int n_cu,
                                hipStream_t stream);
size_t contact_solve_lds_bytes(int n_contacts, size_t elem, int lanes);
int contact_solve_lanes(int n_contacts, size_t elem);
struct ContactSolveLaunch {
    int lanes;         // states per workgroup (0: nothing fits)
    size_t lds_bytes;  // dynamic LDS per workgroup
    size_t per_cu;     // workgroups per CU the grid is capped at
};
ContactSolveLaunch contact_solve_launch(int n_contacts, size_t elem);
// launch_impulse_solve: the velocity-level solve on the same launch record -- V the twists at qd (velocity halves only), v_des [nb][n][3]
// or null; writes impulse [nb][n][3] and the wrench rows [nb][n_bodies][6].  launch_impulse_finish: qd_next = qd + (y1 - y0) over `total`
// elements (qd_next may be qd).
template <class T>
hipError_t launch_impulse_solve(const ContactSet<T> &cs, const T *Linv, const T *Xa, const T *V, const T *v_des, int n_bodies, T mu, T restitution,
                                size_t nb, T *impulse, T *wrench, unsigned long long *bad_count, int n_cu, hipStream_t stream);
template <class T>
hipError_t launch_impulse_finish(const T *qd, const T *y1, const T *y0, size_t total, T *qd_next, hipStream_t stream);
hipError_t set_max_dynamic_lds_contact();
// Scheduled contacts (contact_step_kernels.hip; include/grbda_hip_contact_step.h).  launch_contact_active_solve: the solve of the contacts
// whose bit is set in active[nb], on the launch record above -- Xl, Vl the LISTED poses and twists [nb][n][12] (slot c: the body of contact
// c), des = a_des / v_des [nb][n][3] or null, c_vel = kd (vel = false) or 1 + e (vel = true); writes out = lambda / impulse [nb][n][3],
// exactly 0 off the set, and the body-frame wrench list [nb][n][6].  launch_impact_mask: out[b] = active[b] where a contact closes against
// prev[b], else 0.  launch_free_states_copy: ydd[b] = ydd_free[b] for the states whose set is empty.
template <class T>
hipError_t launch_contact_active_solve(bool vel, const ContactSet<T> &cs, const T *Linv, const T *Xl, const T *Vl, const T *des, const int *active,
                                       T mu, T c_vel, const T g[3], size_t nb, T *out, T *wrench, unsigned long long *bad_count, int n_cu,
                                       hipStream_t stream);
hipError_t launch_impact_mask(const int *active, const int *prev, int n, size_t nb, int *out, hipStream_t stream);
template <class T>
hipError_t launch_free_states_copy(const int *active, int n, const T *ydd_free, int nv, size_t nb, T *ydd, hipStream_t stream);
hipError_t set_max_dynamic_lds_contact_step();

// energy, centre of mass and centroidal momentum (centroidal_kernels.hip).  A body with children keeps its pose (12), velocity (6) and
// acceleration (6) in kCentroidalBodyRows rows [value][kWave] of the wavefront's scratch; `rows` holds per body (its first row or -1 for
// a leaf, its tree parent's first row or -1), built on the host (capi.cpp, ensure_device).
constexpr int kCentroidalBodyRows = 24;
// Outputs of one launch, device arrays over the nb rows of the launch, any of them null: kinetic[nb], potential[nb], com[nb][3],
// com_vel[nb][3], h[nb][6], hdot[nb][6] ([angular 3 about the centre of mass; linear 3], world axes).  The momentum matrix runs the
// expanded batch (nv rows per state, row (b, j) = state b at unit velocity j): h_cols = nv sends the h of row r to column r % nv of
// A[r / nv][6][nv] (h_cols = 0: h[r][6]).
template <class T>
struct CentroidalOut {
    T *kinetic, *potential, *com, *com_vel, *h, *hdot;
    int h_cols;
};
// what one launch is made of: the kernel variant (0 positions, 1 + velocities, 2 + accelerations), the grid, the scratch rows per wavefront
struct CentroidalLaunch {
    int level;
    size_t grid;
    size_t slab_rows;
};
CentroidalLaunch centroidal_launch(bool velocities, bool rates, int n_parent_bodies, int n_cu, size_t nb);
// qd_span / qdd_span: the spanning rates of spanning_kernel (null below the level that reads them); g: the plan's gravity (linear part)
template <class T>
hipError_t launch_centroidal(const DevPlan<T> &P, int n_clusters, int n_span, const int32_t *rows, const CentroidalLaunch &L, const T *q,
                             const T *qd_span, const T *qdd_span, const T g[3], T mass, const CentroidalOut<T> &out, size_t nb, T *scratch,
                             hipStream_t stream);

// the contraction of the vector-Jacobian products (vjp_kernels.hip): out_q[b][j] = sign sum_i w[b][i] Mq[b][i][j] and the same for Mqd,
// w = w_add - w_sub (w_sub may be null), over nb states of row-major [nv][nv] matrices; Mq / out_q and Mqd / out_qd may be null; out_w
// (may be null) receives w.  One launch rule, read by the launcher and by grbda_vjp_contract_launch.
constexpr size_t kVjpWavesPerCu = 16;
struct VjpLaunch {
    size_t units;      // packs of states x column blocks
    size_t grid;       // one-wavefront workgroups
    size_t lds_bytes;  // the weights of one unit
};
VjpLaunch vjp_contract_launch(int nv, size_t elem, int n_cu, size_t nb);
template <class T>
hipError_t launch_vjp_contract(const VjpLaunch &L, const T *Mq, const T *Mqd, const T *w_add, const T *w_sub, T sign, int nv, size_t nb, T *out_q,
                               T *out_qd, T *out_w, hipStream_t stream);

// the contraction of the Jacobian-vector products (jvp_kernels.hip): out[b][i] = w_add[b][i] + sign (sum_j Mq[b][i][j] uq[b][j] + sum_j
// Mqd[b][i][j] uqd[b][j]) over nb states of row-major [nv][nv] matrices; Mq / uq and Mqd / uqd may be null (as pairs), and so may w_add
// (zero).  One launch rule, read by the launcher and by grbda_jvp_contract_launch.
constexpr size_t kJvpWavesPerCu = 16;
constexpr size_t kJvpMaxLdsBytes = 64 * 1024;  // what a launch gets without asking for more: nv up to some 1 900 in fp64
struct JvpLaunch {
    size_t units;      // packs of states x row blocks
    size_t grid;       // one-wavefront workgroups
    size_t lds_bytes;  // two staged vectors and one tile of rows
};
JvpLaunch jvp_contract_launch(int nv, size_t elem, int n_cu, size_t nb);
template <class T>
hipError_t launch_jvp_contract(const JvpLaunch &L, const T *Mq, const T *Mqd, const T *uq, const T *uqd, const T *w_add, T sign, int nv, size_t nb,
                               T *out, hipStream_t stream);

// the manifold part of the step's vector-Jacobian product (step_vjp_kernels.hip, include/grbda_hip_step_vjp.h): the cotangents of the stepped
// state pulled back through q' = q (+) dt qd', qd' = qd + dt ydd, over nb states.  `base`: the device record of the quaternion base's cluster
// (its v_index is read there) or null for a plan without one.  g_q / g_qd may be null (zero), and so may every output.
template <class T>
hipError_t launch_integrate_vjp(const ClusterRec *base, const T *qd_next, T dt, const T *g_q, const T *g_qd, T *grad_q, T *grad_qd, T *grad_ydd,
                                int nv, size_t nb, hipStream_t stream);
// its forward map (include/grbda_hip_jvp.h): the tangents (dq, dqd, dydd) of a state and its acceleration pushed through the same step.  Any
// tangent may be null (zero); either output may be null.
template <class T>
hipError_t launch_integrate_jvp(const ClusterRec *base, const T *qd_next, T dt, const T *dq, const T *dqd, const T *dydd, T *dq_next, T *dqd_next,
                                int nv, size_t nb, hipStream_t stream);
// out[i] = a[i] + b[i] over n scalars: one rounding, operands in this order (out may be a or b)
template <class T>
hipError_t launch_vjp_add(const T *a, const T *b, T *out, size_t n, hipStream_t stream);

// composite-rigid-body algorithm (crba_kernels.hip)
template <class T>
hipError_t launch_crba(const DevPlan<T> &P, const CrbaBody *cb, int n_clusters, int n_rows, const T *q, T *H, size_t B, T *scratch,
                       int grid, hipStream_t stream, bool packed, int interleave);
// (in place; B a multiple of il; il nv (nv + 1) / 2 elements of LDS: unpack_symmetric_lds_bytes <= 60 KiB)
template <class T>
hipError_t launch_unpack_symmetric(T *H, const uint64_t *related, int nv, size_t B, int grid, hipStream_t stream, int il);
size_t unpack_symmetric_lds_bytes(int nv, size_t elem, int il);

// inverse-dynamics derivatives and the batched SPD solve behind d ydd / d (q, qd, tau) (deriv_kernels.hip)
// states per group of the interleaved derivative workspace ([group][entry][kDerivGroup]) = wavefronts per workgroup of the
// matrix-core solve (deriv_kernels.hip)
constexpr int kDerivGroup = 4;
template <class T>
hipError_t launch_rnea_deriv(const DevPlan<T> &P, const DerivBody *db, int n_clusters, int n_rows, int n_max, const T *q, const T *qd,
                             const T *ydd, T *Dq, T *Dqd, T *H, size_t B, T *scratch, int grid, hipStream_t stream, int interleave);
template <class TIO, class TC>
hipError_t launch_spd_solve(const TIO *H, int h_packed, const TIO *P1, const TIO *P2, TIO *Hinv, TIO *X1, TIO *X2, const uint64_t *related,
                            int nv, size_t B, int grid, hipStream_t stream, int interleave);
size_t spd_solve_lds_bytes(int nv, size_t elem, int n_rhs);
// rnea_deriv_kernel's run layout (state-major, or groups of kDerivGroup states where unpack_runs_interleave says so) -> row-major nv x nv in
// place, structural zeros written; D1 may be null; B a multiple of il (deriv_kernels.hip, unpack_runs_kernel)
template <class T>
hipError_t launch_unpack_runs(T *D0, T *D1, const uint64_t *related, int nv, size_t B, int grid, hipStream_t stream, int il);
int unpack_runs_interleave(int nv, size_t elem);
size_t unpack_runs_lds_bytes(int nv, size_t elem, int il);

// analytic derivatives of models with implicit clusters through the spanning tree (manifold_kernels.hip)
template <class T>
hipError_t launch_manifold_constraint(const DevPlan<T> &P, int n_clusters, const int32_t *span_q, const int32_t *span_v, const int32_t *crow,
                                      int nq_s, int nv_s, int n_cpl_rows, int want_d, const T *q, const T *qd, const T *ydd, T *q_s, T *qd_s,
                                      T *qdd_s, T *cpl, size_t B, int grid, hipStream_t stream, int shape = false, bool trig = true);
template <class T>
hipError_t launch_manifold_apply(const DevPlan<T> &P, int n_clusters, const int32_t *span_v, const int32_t *crow, int nv_s, int n_cpl_rows, int mode,
                                 const T *x_s, const T *tau, const T *Hinv, const T *cpl, T *out, size_t B, int grid, hipStream_t stream,
                                 bool big = false);
template <class T>
hipError_t launch_manifold_project(const DevPlan<T> &P, int n_clusters, const int32_t *span_v, const int32_t *crow, const uint64_t *rel,
                                   const uint64_t *rel_s, int nv_s, int n_cpl_rows, int mode, const T *Aq, const T *Av, const T *Hs,
                                   const T *tau_s, const T *cpl, T *Dq, T *Dqd, T *H, size_t B, int grid, hipStream_t stream, int interleave,
                                   bool big = false);
// (plans with clusters beyond the structured limits: H only, one-word masks or nv x nv tables; the solve for up to 128 velocities)
template <class T>
hipError_t launch_manifold_project_wide(const DevPlan<T> &P, int n_clusters, const int32_t *span_v, const int32_t *crow, const uint64_t *rel,
                                        const uint64_t *rel_s, const int32_t *relt, const int32_t *relt_s, int nv_s, int n_cpl_rows, const T *Hs,
                                        const T *cpl, T *H, size_t B, int grid, hipStream_t stream);
template <class T>
hipError_t launch_manifold_state(const DevPlan<T> &P, int n_clusters, const StateFlags &F, const T *q_in, const T *qd_in, int in_nq, int in_nv,
                                 T *q_out, T *qd_out, int32_t *status, T *cond, size_t B, T tol, int grid, hipStream_t stream);
template <class T>
hipError_t launch_manifold_newton(const DevPlan<T> &P, int n_clusters, T *q, int32_t *ok, size_t B, int max_iter, T tol, int grid, hipStream_t stream);
template <class T>
hipError_t launch_spd_wide_solve(const T *H, const int32_t *relt, const T *rhs, T *out, int nv, size_t B, int n_cu, hipStream_t stream,
                                 unsigned long long *bad_count);
// device address of the bad-pivot counter of the SPD solves (deriv_kernels.hip; nullptr when it cannot be resolved): the solve of the wide
// route (manifold_kernels.hip, another translation unit) counts into the same word
unsigned long long *spd_bad_count_address();
int spd_mfma_workgroups_per_cu(int nv);
bool spd_solve_on_mfma(size_t elem, int nv, int n_rhs);
hipError_t set_max_dynamic_lds_deriv();
// H^-1 = W^T W from the articulated-body quantities (minv_kernels.hip; plan.h, MinvProgram): the record blocks (one state per lane, the
// slab rows and processing order of rnea_deriv_kernel), then the walk + the two products on the matrix cores (one state per wavefront;
// records and right-hand sides interleaved by groups of kDerivGroup states)
template <class T>
hipError_t launch_abi_factor(const DevPlan<T> &P, const DerivBody *db, const MinvBody *mb, int n_clusters, int n_rows, int n_max, int n_entries,
                             const T *q, T *rec, size_t B, T *scratch, int grid, hipStream_t stream, int interleave,
                             unsigned long long *bad_count);
template <class T>
hipError_t launch_minv_solve(const T *rec, int n_entries, int r_il, const int32_t *coltab, int max_depth, int base_off, int n_max, const T *P1,
                             const T *P2, int p_il, T *Hinv, T *X1, T *X2, const uint64_t *related, int nv, size_t B, int grid,
                             hipStream_t stream);
size_t minv_solve_lds_bytes(int nv, int n_rhs, int n_entries, size_t elem);
template <class T>
int minv_workgroups_per_cu(int nv, int n_max, int n_rhs, int n_entries);  // (registers of the instantiation and LDS granules; needs the current device)
hipError_t set_max_dynamic_lds_minv();
hipError_t spd_bad_pivots(unsigned long long *count, int reset);

}  // namespace grbda_hip
