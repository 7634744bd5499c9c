/*
 * grbda_hip.h -- C ABI of the MI355X batched cluster-ABA / cluster-RNEA engine.
 *
 * The reference (ROAM-Lab-ND/generalized_rbda) has no FFI: its boundary is the C++ class
 * grbda::ClusterTreeModel (include/grbda/Dynamics/ClusterTreeModel.h:24-165,
 * include/grbda/Dynamics/TreeModel.h:15-143).  Each entry point below cites the member it
 * replaces; the C++17 facade in generalized_rbda_amd/include/grbda keeps the reference's class
 * names and calls these functions, and INTEGRATION.md shows the few lines a maintainer of the
 * reference would add to route ClusterTreeModel::forwardDynamics through them.
 *
 * Conventions
 *   - all batched arrays are row-major: q[B][nq], qd[B][nv], tau[B][nv], ydd[B][nv];
 *     positions are *independent* coordinates for explicit clusters and *spanning* positions
 *     for implicit-loop clusters (GenericJoint.cpp:246-249); velocities / accelerations /
 *     torques are always independent (TreeModel.h:83-84);
 *   - `_f32/_f64` device entry points take DEVICE pointers on `device`, enqueue on `stream`
 *     (a hipStream_t, may be NULL) and return without synchronising;
 *   - the caller owns every buffer; a plan is immutable after creation and may be shared by
 *     threads and streams (the reference model is a stateful cache and is not thread safe,
 *     TreeModel.h:138-142);
 *   - functions return 0 (GRBDA_OK) or a negative error code and never throw;
 *   - there is NO CPU fallback: every compute entry point fails with GRBDA_ENODEVICE when no
 *     HIP device is usable.
 */
#ifndef GRBDA_HIP_H
#define GRBDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GRBDA_OK = 0,
    GRBDA_EINVAL = -1,       /* bad argument / malformed blob                                  */
    GRBDA_EUNSUPPORTED = -2, /* model uses a topology / constraint the kernels do not cover yet */
    GRBDA_ENODEVICE = -3,    /* no usable HIP device                                           */
    GRBDA_EHIP = -4,         /* a HIP runtime call failed (see grbda_last_error)               */
    GRBDA_ENOMEM = -5,
    GRBDA_EPARSE = -6,       /* URDF+ file could not be parsed                                 */
    GRBDA_ESTATE = -7        /* invalid spanning state (ClusterJoint.cpp:43-46,62-65)          */
};

typedef struct grbda_plan grbda_plan;

/* human-readable text for an error code; thread-local detail of the last failure */
const char *grbda_strerror(int code);
const char *grbda_last_error(void);

/* ---- model -> plan ------------------------------------------------------------------------ */

/* Replaces the state held by a constructed ClusterTreeModel (ClusterTreeModel.cpp:10-67):
 * `blob` is a model description (include/grbda_model_desc.h) written by the C++ facade
 * (grbda::ClusterTreeModel::serialize) or by grbda_urdf_to_blob.  Host-only: needs no GPU. */
int grbda_plan_from_blob(const void *blob, size_t bytes, grbda_plan **out);

/* Replaces ClusterTreeModel::buildModelFromURDF(path) (ClusterTreeModel.h:41-46,
 * src/Dynamics/ClusterTreeParsing.cpp:5-440).  ori_repr: 0 quaternion, 1 roll-pitch-yaw. */
int grbda_plan_from_urdf(const char *path, int ori_repr, grbda_plan **out);

/* URDF+ file(s) -> model description blob (buildModelFromURDF(vector<path>),
 * ClusterTreeModel.h:48-53).  Call with buf = NULL to query *needed. */
int grbda_urdf_to_blob(const char *const *paths, int n_paths, int ori_repr, void *buf, size_t cap,
                       size_t *needed);

void grbda_plan_free(grbda_plan *plan);

/* Hands the work buffers of the chunked pipelines (derivatives, mass matrix / derivatives on the constraint manifold, position
 * projection) back to the device allocator.  They are kept per (device, stream) between calls -- up to a few GiB after a
 * million-state derivative call (16 GiB on the manifold route) -- and otherwise live until grbda_plan_free; the next call that
 * needs one allocates it again.  Waits for the work enqueued on them; refused (GRBDA_EINVAL) while one of the plan's streams is
 * capturing.  *bytes_released (may be NULL): what was freed.  No counterpart in the reference: its temporaries are Eigen
 * objects of one state (ClusterTreeModel.h:150-170). */
int grbda_plan_release_work(grbda_plan *plan, unsigned long long *bytes_released);

/* getNumPositions / getNumDegreesOfFreedom / getNumBodies / clusters().size()
 * (TreeModel.h:25-26, ClusterTreeModel.h:98,113); any out pointer may be NULL */
int grbda_plan_dims(const grbda_plan *plan, int *nq, int *nv, int *n_bodies, int *n_clusters);

/* TreeModel::setGravity / getGravity (TreeModel.h:56-57): linear part of the gravity vector.
 * Not thread safe against concurrent launches on the same plan.  Gravity is a kernel argument read at launch: every call after
 * set_gravity uses the new value, and a captured graph keeps the gravity of its capture. */
int grbda_plan_set_gravity(grbda_plan *plan, const double g[3]);
int grbda_plan_get_gravity(const grbda_plan *plan, double g[3]);

/* the model description the plan was built from (for serialisation / the oracle in tests) */
int grbda_plan_blob(const grbda_plan *plan, const void **blob, size_t *bytes);

/* kernel resource / cost figures: per-state slots, LDS bytes per wave, global scratch bytes per
 * wave, flops per forward-dynamics and inverse-dynamics evaluation (counted by the plan
 * compiler from the operation list the kernel executes) */
typedef struct {
    int n_slots;
    int n_lds_slots_f32, n_lds_slots_f64;
    size_t lds_bytes_f32, lds_bytes_f64;
    size_t scratch_bytes_per_wave_f32, scratch_bytes_per_wave_f64;
    double flops_aba, flops_rnea;
    double bytes_aba_f32, bytes_aba_f64; /* algorithmic bytes per evaluation: (nq+2nv+nv)*s */
    int n_axisym_bodies;  /* leaf bodies evaluated at q = 0 (rotors), see plan.h */
    int n_carry_clusters; /* clusters whose projected inertia is handed over in registers */
    int split_aba_f32, split_rnea_f32; /* 1: the f32 kernel runs the split layout ([K | y0] blocks in the global slab,
                                          every other object in LDS, plan.h Layout::split_*) */
    int n_lds_slots_split_f32;
    int chain_aba_f32;         /* 1: the f32 forward dynamics run the chain-structured kernel (plan.h, ChainProgram) */
    int n_lds_slots_chain_f32, n_chain_segments;
    int chain_aba_f64;
    int chain_rnea_f32, chain_rnea_f64; /* inverse dynamics on the chains (rnea_chain_kernel) */
    int analytic_derivatives;           /* grbda_fd_d* / grbda_fd_derivatives_* take the analytic route (deriv_kernels.hip) */
    int n_chain_differentials;          /* implicit two-rotor differential clusters inside the f32 chain program */
    int latency_mode_f32, latency_mode_f64; /* 1: batches of at most one tile per SIMD run a tile on two wavefronts (plan.h, ChainProgram::n_waves) */
    int n_chain_generic;                /* generic clusters inside the f32 chain program (plan.h, ChainGen): URDF+ position loops, triple / Generic clusters */
    int spanning_tree_route;            /* 1: a cluster attaches to several bodies of its parent cluster, or has more than 8 bodies / 4 independent
                                           coordinates (up to 48 / 48; models up to 128 velocities) -- forward / inverse dynamics (with external
                                           forces), mass matrix and d ydd / d tau run through the spanning tree and the per-state G
                                           (H = G^T H_s G; capi.cpp projection_run), no sweep programs; INTEGRATION.md 3 lists what the route refuses */
} grbda_plan_info_t;
int grbda_plan_info(const grbda_plan *plan, grbda_plan_info_t *info);

/* ---- batched dynamics (device pointers) ----------------------------------------------------- */
/* The device entry points only enqueue work on the stream they are given and may be captured into a hipGraph as they are.
 * The library keeps one scratch slab per (device, stream) and grows it on demand (hipFree + hipMalloc): a captured launch
 * holds the slab's address, so (i) call once with the largest batch on that stream BEFORE capturing -- a call that would have
 * to grow the slab while its stream is capturing returns GRBDA_EINVAL -- and (ii) do not make a larger eager call on the same
 * (device, stream) while the graph is alive.
 * Batches of at most one 64-state tile per SIMD (4 x the CU count) take the latency-mode forward-dynamics kernel when the
 * plan has one (grbda_plan_info: latency_mode_f32 / _f64): same results to rounding, 20-35 % less time per call. */

/* ClusterTreeModel::setState + forwardDynamics(tau) over B independent states
 * (ClusterTreeModel.cpp:256-308, ClusterTreeDynamics.cpp:85-191): cluster ABA.
 * f_ext: NULL, or [B][n_bodies][6] world-frame spatial forces (TreeModel::setExternalForces,
 * TreeModel.cpp:214-239). */
int grbda_aba_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau,
                  const double *f_ext, double *ydd, size_t B, int device, void *stream);
int grbda_aba_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau,
                  const float *f_ext, float *ydd, size_t B, int device, void *stream);

/* ClusterTreeModel::setState + inverseDynamics(ydd) (ClusterTreeDynamics.cpp:79-83,
 * TreeModel.cpp:34-57,173-212): cluster RNEA. */
int grbda_rnea_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd,
                   const double *f_ext, double *tau, size_t B, int device, void *stream);
int grbda_rnea_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd,
                   const float *f_ext, float *tau, size_t B, int device, void *stream);

/* ---- quantities derived from the two recursions ---------------------------------- */
/* All take DEVICE pointers like grbda_aba_* / grbda_rnea_*.  They are evaluated with the same kernels over
 * an expanded batch (one extra row per unit vector), chunked so that the work space stays below 256 MiB:
 * RNEA is affine in ydd and ABA is affine in tau and quadratic in qd, so the differences below are exact
 * (no step size enters), not finite-difference approximations.
 *
 * grbda_bias_*        C(q, qd) = RNEA(q, qd, 0)                  TreeModel::updateBiasForceVector
 *                     out[B][nv]                                   (TreeModel.cpp:162-171), getBiasForceVector
 *                                                                  (ClusterTreeModel.cpp:106-110)
 * grbda_mass_matrix_* H(q) e_j = RNEA(q, 0, e_j) - RNEA(q, 0, 0) ClusterTreeModel::getMassMatrix
 *                     out[B][nv][nv], row-major, symmetric         (ClusterTreeModel.cpp:99-104; the reference runs
 *                                                                  the CRBA, TreeModel.cpp:115-160)
 * grbda_fd_dtau_*     d ydd / d tau = H^-1:                       the exact identity the reference's derivative
 *                     column j = ABA(q, 0, e_j) - ABA(q, 0, 0)     tests check (SURVEY 8c viii)
 *                     out[B][nv][nv]
 * grbda_fd_dqd_*      d ydd / d qd, column j =                     central difference with unit step, exact
 *                     (ABA(qd + e_j) - ABA(qd - e_j)) / 2          because ABA is quadratic in qd
 *                     out[B][nv][nv]                               (testRigidBodyDynamicsAlgosDerivatives.cpp:309-380)
 * grbda_fd_dq_*       d ydd / d q along the tangent step the         central difference with the caller's step: NOT
 *                     reference's derivative test uses                exact (truncation + rounding, the reference
 *                     (testHelpers.hpp:50-112: q_i += d; free base    uses step 1e-8 in fp64 and accepts 2e-5,
 *                     pos += R^T d, quat += quat x (0, d) / 2):       testRigidBodyDynamicsAlgosDerivatives.cpp:
 *                     column j = (ABA(q + h e_j) - ABA(q - h e_j))    309-335).  Implicit-loop models: an INDEPENDENT
 *                     / (2 h), out[B][nv][nv]                         position moves, the dependent ones are re-projected
 *                                                                     onto phi(q) = 0; a roll-pitch-yaw base: plain q + dq.
 *
 * Models made of explicit (constant G) clusters with nv <= 64 -- every URDF robot of
 * the reference without <loop> elements -- do not go through those batches: the mass matrix comes from the
 * composite-rigid-body kernel, and the three derivatives from the ANALYTIC recursion of deriv_kernels.hip
 * (d ID / d q and d ID / d qd of the spanning tree projected with G, then one batched SPD solve per state:
 * d ydd / d tau = H^-1, d ydd / d q = -H^-1 dID/dq, d ydd / d qd = -H^-1 dID/dqd at ydd = FD(q, qd, tau)); `step` is then
 * not used.  grbda_fd_derivatives_* returns any subset of the three matrices from ONE pass (NULL = not wanted) and falls
 * back to the three entry points above for the other models.  The analytic route keeps its intermediate matrices in a
 * device workspace owned by the plan, one per (device, stream), of at most 2 GiB (the batch goes through in chunks of that
 * size); the output arrays must not overlap the inputs or each other.  The f32 analytic route factors H per state by Cholesky
 * on the matrix-core kernel: a state whose H is not positive definite in single precision (massless chains, garbage input)
 * gets NaN / Inf in its three matrices while the call returns GRBDA_OK -- check the outputs, or use the _f64 entry points
 * (GRBDA_SOLVE_F64=1 keeps fp32 storage with an fp64 solve).
 */
int grbda_bias_f64(const grbda_plan *plan, const double *q, const double *qd, const double *f_ext, double *out,
                   size_t B, int device, void *stream);
int grbda_bias_f32(const grbda_plan *plan, const float *q, const float *qd, const float *f_ext, float *out,
                   size_t B, int device, void *stream);
int grbda_mass_matrix_f64(const grbda_plan *plan, const double *q, double *H, size_t B, int device, void *stream);
int grbda_mass_matrix_f32(const grbda_plan *plan, const float *q, float *H, size_t B, int device, void *stream);
int grbda_fd_dtau_f64(const grbda_plan *plan, const double *q, double *Hinv, size_t B, int device, void *stream);
int grbda_fd_dtau_f32(const grbda_plan *plan, const float *q, float *Hinv, size_t B, int device, void *stream);
int grbda_fd_dqd_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, double *J,
                     size_t B, int device, void *stream);
int grbda_fd_dqd_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, float *J,
                     size_t B, int device, void *stream);
int grbda_fd_dq_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, double step,
                    double *J, size_t B, int device, void *stream);
int grbda_fd_dq_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, double step, float *J,
                    size_t B, int device, void *stream);
int grbda_fd_derivatives_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, double *dydd_dq,
                             double *dydd_dqd, double *dydd_dtau, size_t B, int device, void *stream);
int grbda_fd_derivatives_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, float *dydd_dq,
                             float *dydd_dqd, float *dydd_dtau, size_t B, int device, void *stream);
/* ---- first-order derivatives of the INVERSE dynamics -----------------------------------------------------------------------
 * tau = ID(q, qd, ydd) = H(q) ydd + C(q, qd).  For B states at (q, qd, ydd), each output [B][nv][nv] row-major with
 * out[b][i][j] = d tau_i / d x_j:
 *     dtau_dq    d ID / d q     columns along the tangent step grbda_fd_dq_* documents (testHelpers.hpp:50-112: a quaternion base takes
 *                               pos += R^T d, quat += quat x (0, d) / 2; a roll-pitch-yaw base plain q + dq; implicit-loop models move an
 *                               INDEPENDENT position and re-project the dependent ones onto phi(q) = 0)
 *     dtau_dqd   d ID / d qd
 *     dtau_dydd  d ID / d ydd = H(q), full and symmetric: asked for alone, the call IS grbda_mass_matrix_*; asked for with the
 *                               others it is computed by that entry point too (the same bits either way)
 * Any output may be NULL, not all three; the outputs must not overlap the inputs or each other (GRBDA_EINVAL).  These are the
 * matrices of inverse-dynamics-based trajectory optimisation, computed-torque linearisation and identification (Pinocchio:
 * computeRNEADerivatives); with ydd = FD(q, qd, tau) they are related to grbda_fd_derivatives_* by d ydd / d q = -H^-1 d tau / d q,
 * d ydd / d qd = -H^-1 d tau / d qd, but nothing is inverted or factorised here, and no forward dynamics runs.
 *
 * Plans with grbda_plan_info.analytic_derivatives == 1 made of explicit clusters (nv <= 64): the analytic recursion of
 * deriv_kernels.hip, ONE pass per state, writes d ID / d q and d ID / d qd projected with G into the caller's arrays and a second
 * kernel puts them into row-major order in place (entries between coordinates that are not on one root path are structural zeros and
 * are written as 0.0); `step` is not used and the call needs no work space beyond the per-stream scratch slab.  Every other plan
 * (implicit clusters, nv > 64, the spanning-tree route, GRBDA_NO_ANALYTIC=1): difference batches over grbda_rnea_* -- d tau / d qd
 * by central differences with unit step (exact: the inverse dynamics are quadratic in qd), d tau / d q by central differences with
 * `step` (> 0; 1e-6 suits fp64) along the tangent step above, implicit clusters re-projected by Newton; the _f32 entry point takes those
 * position differences in fp64 on the converted inputs, as grbda_fd_dq_f32 does.
 *
 * Device pointers; the call enqueues on `stream` and does not synchronise; it can be captured after one eager call of the same B on
 * that stream; gravity is read at launch.  There is NO f_ext argument: world-frame external forces make d tau / d q depend on the
 * body poses (the force on a body turns with every joint between it and the world), which the recursion does not carry.
 * B == 0: GRBDA_OK.  The _host_ variant takes host arrays (allocates, copies and synchronises per call). */
int grbda_rnea_derivatives_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double step,
                               double *dtau_dq, double *dtau_dqd, double *dtau_dydd, size_t B, int device, void *stream);
int grbda_rnea_derivatives_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, double step,
                               float *dtau_dq, float *dtau_dqd, float *dtau_dydd, size_t B, int device, void *stream);
int grbda_rnea_derivatives_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double step,
                                    double *dtau_dq, double *dtau_dqd, double *dtau_dydd, size_t B, int device);
/* States whose joint-space inertia matrix H was not positive definite to working precision in the SPD solves behind
 * grbda_fd_dtau_* / grbda_fd_dq_* / grbda_fd_dqd_* / grbda_fd_derivatives_* (a pivot of the factorisation <= 0 or not finite: massless
 * chains, a singular pose of an implicit cluster) get NaN / Inf results; the reference's ColPivHouseholderQR would return some
 * least-squares answer there (src/Dynamics/ClusterTreeNode.cpp:33-37).  The solve kernels COUNT such states per device: this call
 * synchronises the device, returns the count since the last reset and (reset != 0) clears it.  The contact solve of
 * grbda_contact_dynamics_* counts into the same word: a state whose J_w H^-1 J_w^T + damping I had such a pivot (redundant contacts
 * with damping = 0) has NaN in its lambda and ydd.  So does the solve of grbda_contact_impulse_* (NaN in impulse and qd_next). */
int grbda_spd_bad_pivots(int device, unsigned long long *count, int reset);
/* The name of the kernel grbda_aba_* (kind 0) / grbda_rnea_* (kind 1) launches for a batch of B states in this precision (32 | 64) on
 * this device, without external forces -- as rocprofv3 prints it (template arguments included; the chain kernels' inverse dynamics
 * may append a wave-count variant).  bench.py reports it next to the roofline figures instead of re-deriving the selection. */
int grbda_kernel_name(const grbda_plan *plan, int kind, int precision, size_t B, int device, char *buf, size_t cap);

/* host-array variants (allocate, copy and synchronise per call: for the facade's single-state calls and small batches) */
int grbda_mass_matrix_host_f64(const grbda_plan *plan, const double *q, double *H, size_t B, int device);
int grbda_fd_derivatives_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, double *dydd_dq,
                                  double *dydd_dqd, double *dydd_dtau, size_t B, int device);

/* ---- steps either side of the path ------------------------------------------ */
/* Newton projection of the DEPENDENT spanning coordinates of every implicit-loop cluster onto phi(q) = 0, in
 * place, the independent ones held fixed: q_d <- q_d - K_d^-1 phi until |phi| < 1e-12 or max_iter steps; a
 * state is reported valid (ok[b] = 1) when every cluster ends with |phi| < tol.  This is what the reference
 * does per state when it draws random states of a GenericImplicit joint (GenericJoint.cpp:289-385 with
 * Utilities.h:124-140; it accepts |phi| < 1e-8) and what a simulator calls against constraint drift.
 * q: [B][nq] device array, updated; ok: [B] device int32 or NULL.  Models without implicit clusters: no-op. */
int grbda_project_positions_f64(const grbda_plan *plan, double *q, int32_t *ok, size_t B, int max_iter, double tol,
                                int device, void *stream);
int grbda_project_positions_f32(const grbda_plan *plan, float *q, int32_t *ok, size_t B, int max_iter, double tol,
                                int device, void *stream);
/* The same with HOST arrays (copied to the device and back; synchronises): what the C++ facade's randomJointState() of an implicit
 * cluster of a URDF-built model runs (GenericJoint.cpp:289-348: independent coordinates U(-1, 1), dependent guess U(-0.1, 0.1), Newton,
 * at most 45 draws). */
int grbda_project_positions_host_f64(const grbda_plan *plan, double *q, int32_t *ok, size_t B, int max_iter, double tol, int device);

/* State input in the reference's conventions: ClusterJoints::Base::toSpanningTreeState (ClusterJoint.cpp:22-71) behind
 * ClusterTreeModel::setState(const ModelState&) (ClusterTreeModel.cpp:256-276).  Every JointState of a ModelState flags
 * its position and its velocity as independent or SPANNING coordinates (JointCoordinate::isSpanning(),
 * StateRepresentation.h:10-36); half of the reference's dynamics tests feed spanning states
 * (testRigidBodyDynamicsAlgos.cpp:45-72,195-196).  The compute entry points take the engine's own coordinates --
 * independent ones for explicit clusters, spanning POSITIONS for implicit clusters, independent velocities -- and these
 * calls convert a batch to them, with the reference's validity checks:
 *   pos_is_spanning[c], vel_is_spanning[c]  (n_clusters bytes each; NULL = the engine's convention / all independent)
 *   q_in  [B][in_nq], qd_in [B][in_nv]      the clusters' segments back to back, each n or k entries wide
 *                                           (free base: 7 or 6 positions, 6 velocities); widths: grbda_state_input_dims
 *   q [B][nq], qd [B][nv]                   engine coordinates (either may be NULL; qd_in may be NULL with qd)
 *   status[B]                               0, or code + 256 * cluster of the first failure in cluster order:
 *                                           1 "Spanning position is not valid"  (implicit cluster, |phi(q)|_2 >= tol;
 *                                             LoopConstraint.cpp:15-19.  Explicit clusters are taken as they are, like
 *                                             the reference: ClusterJoint.cpp:37-41),
 *                                           2 "Spanning velocity is not valid"  (|K qd_span|_2 >= tol, LoopConstraint.cpp:22-26)
 *   cond[B][2] (or NULL)                    maxima over the implicit clusters of [0] |K_d^-1 K_i| (the state-dependent
 *                                           entries of G: how strongly the loop amplifies rates) and [1] |K_d|_F |K_d^-1|_F
 *                                           (condition number of the inverted block; NaN where K_d is singular) -- what
 *                                           the synthetic-state generator gates on
 *   tol                                     the reference's nearZero tolerance is 1e-8 (Utilities.h:124-130)
 * Independent positions for an implicit cluster are refused with GRBDA_ESTATE before anything is launched
 * (ClusterJoint.cpp:32-35).  Device arrays; the _host_ variant takes host arrays, synchronises and returns GRBDA_ESTATE
 * with the reference's message in grbda_last_error() if any state is invalid (what the facade's setState throws). */
int grbda_state_input_dims(const grbda_plan *plan, const uint8_t *pos_is_spanning, const uint8_t *vel_is_spanning, int *in_nq,
                           int *in_nv);
int grbda_state_to_independent_f64(const grbda_plan *plan, const uint8_t *pos_is_spanning, const uint8_t *vel_is_spanning,
                                   const double *q_in, const double *qd_in, double *q, double *qd, int32_t *status, double *cond,
                                   size_t B, double tol, int device, void *stream);
int grbda_state_to_independent_f32(const grbda_plan *plan, const uint8_t *pos_is_spanning, const uint8_t *vel_is_spanning,
                                   const float *q_in, const float *qd_in, float *q, float *qd, int32_t *status, float *cond,
                                   size_t B, double tol, int device, void *stream);
int grbda_state_to_independent_host_f64(const grbda_plan *plan, const uint8_t *pos_is_spanning, const uint8_t *vel_is_spanning,
                                        const double *q_in, const double *qd_in, double *q, double *qd, size_t B, double tol,
                                        int device);

/* Spanning-tree velocities and accelerations of every body joint from the independent ones:
 * qd_span = G yd, qdd_span = G ydd + g (ClusterJoint.cpp:55-58, GenericJoint.cpp:57-90; what the reference's
 * benchmarks do with the result of forwardDynamics, pinocchioBenchmark.cpp:168-176).  Order: clusters in model
 * order, bodies by sub-index; the free base contributes its 6 components unchanged.
 * qd_span (may be NULL), qdd_span: [B][n_span_vel] device arrays (grbda_plan_span_dims). */
int grbda_plan_span_dims(const grbda_plan *plan, int *n_span_vel);
int grbda_spanning_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double *qd_span,
                       double *qdd_span, size_t B, int device, void *stream);
int grbda_spanning_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, float *qd_span,
                       float *qdd_span, size_t B, int device, void *stream);

/* ---- time stepping ---------------------------------------------------------------------------------------- */
/* One semi-implicit (symplectic) Euler step on the configuration manifold, in the engine's coordinates.  The step is FIRST ORDER in dt:
 *
 *     yd'   = yd + dt ydd                                              all nv entries
 *     y'    = y + dt yd'                                               explicit clusters (Revolute, rotor, pair, triple, Generic: constant G)
 *     p'    = p + dt R(quat)^T v'                                      free base: q = [p 3 | quat 4, scalar first], qd = [omega; v] in body
 *     quat' = normalise(quat x [cos(a/2), sin(a/2) omega'/|omega'|])   coordinates, R of the OLD orientation, a = |omega'| dt; axis (1,0,0)
 *                                                                      when omega' = 0 (ori::integrateQuatImplicit, OrientationTools.h:431-458)
 *     q_s'  = q_s + dt G(q_s) yd', then the dependent entries          implicit clusters: G at the OLD positions, then the Newton projection
 *             back onto phi(q) = 0, the independent ones fixed         of grbda_project_positions_* (GenericJoint.cpp:289-385)
 *
 * grbda_integrate_*: q [B][nq], qd, ydd [B][nv] in; q_next [B][nq], qd_next [B][nv] out, which may BE q and qd (equal pointers; any other
 *   overlap of an output with an input is GRBDA_EINVAL).  ok: NULL or [B] int32, 1 when every implicit cluster of the state ended with
 *   |phi| < tol (always 1 for models without implicit clusters); max_iter, tol: as for grbda_project_positions_*.
 * grbda_step_*: exactly grbda_aba_* (tau, f_ext or NULL -> ydd) followed by grbda_integrate_* with max_iter = 50, tol = 1e-8 (the
 *   reference's nearZero) on the same stream.  ydd [B][nv] is written: the accelerations of this step.  The caller owns it.
 * grbda_rollout_*: exactly T calls of grbda_step_* in place on q, qd (in: state 0, out: state T), bit for bit.  tau_steps = 1: tau [B][nv]
 *   held for all steps; tau_steps = T: tau [T][B][nv].  ydd_work [B][nv]: the caller's work array (the last step's accelerations on return).
 *   q_traj [T][B][nq], qd_traj [T][B][nv] (each may be NULL): states 1 .. T, copied device-to-device after every step.  ok: NULL or [B],
 *   the AND over the steps.
 * All of them only enqueue (kernels and copies on `stream`, one after the other), never synchronise, and allocate nothing beyond the
 * per-(device, stream) scratch slab: capturable after one eager call of the same B on the stream; dt and gravity are read at launch.
 * Errors: GRBDA_EINVAL for NULL required pointers, a dt that is not finite, T < 0, tau_steps not in {1, T}, overlapping arrays;
 * GRBDA_EUNSUPPORTED (text in grbda_last_error()) for a roll-pitch-yaw floating base -- its rate map is not built -- and for plans on the
 * spanning-tree route that contain implicit clusters; explicit plans on that route are covered.  All of these are decided on the host
 * before anything is enqueued.  B == 0 or T == 0: GRBDA_OK, nothing done.
 * In fp32 |phi| < 1e-8 is out of reach: grbda_step_f32 / grbda_rollout_f32 report ok = 0 for states with implicit clusters (the positions
 * are still projected, to fp32 accuracy); pass a tolerance that fits the precision to grbda_integrate_f32. */
int grbda_integrate_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double dt, double *q_next,
                        double *qd_next, int32_t *ok, int max_iter, double tol, size_t B, int device, void *stream);
int grbda_integrate_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, double dt, float *q_next,
                        float *qd_next, int32_t *ok, int max_iter, double tol, size_t B, int device, void *stream);
int grbda_step_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *f_ext, double dt,
                   double *ydd, double *q_next, double *qd_next, int32_t *ok, size_t B, int device, void *stream);
int grbda_step_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, const float *f_ext, double dt, float *ydd,
                   float *q_next, float *qd_next, int32_t *ok, size_t B, int device, void *stream);
int grbda_rollout_f64(const grbda_plan *plan, double *q, double *qd, const double *tau, int tau_steps, double dt, int T, double *ydd_work,
                      double *q_traj, double *qd_traj, int32_t *ok, size_t B, int device, void *stream);
int grbda_rollout_f32(const grbda_plan *plan, float *q, float *qd, const float *tau, int tau_steps, double dt, int T, float *ydd_work,
                      float *q_traj, float *qd_traj, int32_t *ok, size_t B, int device, void *stream);
/* The same with HOST arrays (copied to the device and back; synchronise): the C++ facade's integrateBatch / stepBatch. */
int grbda_integrate_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double dt, double *q_next,
                             double *qd_next, int32_t *ok, int max_iter, double tol, size_t B, int device);
int grbda_step_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *f_ext, double dt,
                        double *ydd, double *q_next, double *qd_next, int32_t *ok, size_t B, int device);

/* ---- contact side --------------------------------------------------------------------- */
/* Absolute transform world -> body of every body, TreeNode::Xa_ after TreeModel::forwardKinematics
 * (TreeModel.cpp:6-32): Xa[B][n_bodies][12] = rotation E (9, row-major: v_body = E v_world) then the position r
 * of the body origin in world coordinates (spatial::Transform, SpatialTransforms.cpp:13-40).  A point fixed in
 * the body at `offset` sits at r + E^T offset in the world (contact-point kinematics, TreeModel.cpp:59-76). */
int grbda_body_poses_f64(const grbda_plan *plan, const double *q, double *Xa, size_t B, int device, void *stream);
int grbda_body_poses_f32(const grbda_plan *plan, const float *q, float *Xa, size_t B, int device, void *stream);

/* Spatial velocity and acceleration of every body in its own coordinates, TreeNode::v_ / a_ after
 * TreeModel::forwardAccelerationKinematics(ydd) (TreeModel.cpp:6-57): V[B][n_bodies][12] = [v 6 | a 6], each [angular 3;
 * linear 3].  As in the reference the acceleration is the one the recursions carry -- the base starts from -gravity, so a
 * body at rest has a = X (0, 0, 0, 0, 0, 9.81) -- which is what ClusterTreeModel::getLinearAcceleration /
 * getAngularAcceleration (ClusterTreeModel.cpp:376-404) rotate into world axes and what
 * TreeModel::contactPointForwardAccelerationKinematics (TreeModel.cpp:78-99) adds gravity back to.  q, qd, ydd as for the
 * inverse dynamics (implicit clusters: spanning positions on the manifold). */
int grbda_body_twists_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double *V, size_t B,
                          int device, void *stream);
int grbda_body_twists_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, float *V, size_t B,
                          int device, void *stream);

/* ClusterTreeModel::applyTestForce (ClusterTreeDynamics.cpp:194-233) for B states: a world-frame Cartesian force
 * force[B][3] acts at the point `offset` (host, body coordinates) of body `body`;
 * dstate[B][nv] = H^-1 J^T f and lambda_inv[B] = f^T J H^-1 J^T f.  Evaluated with the two kernels (ABA and RNEA
 * with and without the force as an external wrench), not with the reference's force propagators. */
int grbda_apply_test_force_f64(const grbda_plan *plan, const double *q, int body, const double offset[3],
                               const double *force, double *lambda_inv, double *dstate, size_t B, int device,
                               void *stream);
int grbda_apply_test_force_f32(const grbda_plan *plan, const float *q, int body, const double offset[3],
                               const float *force, float *lambda_inv, float *dstate, size_t B, int device,
                               void *stream);

/* ClusterTreeModel::inverseOperationalSpaceInertiaMatrix (ClusterTreeDynamics.cpp:295-435) and the contact
 * Jacobians for B states and up to 8 contact frames per call: frame c sits on body bodies[c] (host array) at the
 * body-fixed point offsets[c][3] (host) with the body's axes -- the frame of the reference's end-effector force
 * propagators (createSXform(1, local_offset), :316-320).
 *   Linv[B][6 n][6 n] = J H^-1 J^T, rows / columns ordered frame by frame, [moment 3, force 3] each;
 *   J[B][6 n][nv] (may be NULL): the 6-D Jacobians of the frames in their own coordinates.
 * Evaluated from unit wrenches through the ABA and RNEA kernels (6 n + 1 rows per state each), not with the
 * reference's extended-force-propagator recursion; the results are the same matrices. */
int grbda_inv_osim_f64(const grbda_plan *plan, const double *q, int n_contacts, const int *bodies,
                       const double *offsets, double *Linv, double *J, size_t B, int device, void *stream);
int grbda_inv_osim_f32(const grbda_plan *plan, const float *q, int n_contacts, const int *bodies,
                       const double *offsets, float *Linv, float *J, size_t B, int device, void *stream);

/* ---- contact points and contact-constrained forward dynamics ------------------------------------------------------------------
 * Contacts are described as for grbda_inv_osim_*: n_contacts in 1 .. 8, host arrays bodies[n] and offsets[n][3] (a point fixed in the
 * body, body coordinates).  Every other array is a device array, row-major; the calls only enqueue on `stream`.
 *
 * grbda_contact_points_*: world-frame position, velocity and classical acceleration of the points -- cp.position_ / velocity_ /
 * acceleration_ after TreeModel::contactPointForwardKinematics / contactPointForwardAccelerationKinematics (TreeModel.cpp:59-100), what
 * getPosition / getLinearVelocity / getLinearAcceleration return for a body with an offset.  pos, vel, acc: [B][n][3] each, world axes;
 * any may be NULL, not all three.  vel needs qd, acc needs qd and ydd; otherwise those inputs may be NULL.  With E, r of
 * grbda_body_poses_* and [omega; v | alpha; a] of grbda_body_twists_* (body axes, a carrying -gravity), o the offset and g the plan's
 * gravity:
 *     p      = r + E^T o
 *     p_dot  = E^T (v + omega x o)
 *     p_ddot = E^T (a + alpha x o + omega x (v + omega x o)) + g          (a point of a body at rest: 0)
 *
 * grbda_contact_dynamics_*: the forward dynamics subject to "these points have this acceleration" (Pinocchio:
 * forwardDynamics(q, v, tau, J, gamma, inv_damping)); the reference leaves this solve to the simulator that calls
 * inverseOperationalSpaceInertiaMatrix and the contact-point kinematics.  With J_w [3 n][nv] the world-frame Jacobian of the points
 * (E^T times the force rows of the frame Jacobians of grbda_inv_osim_*):
 *     ydd_free = FD(q, qd, tau, f_ext)
 *     (J_w H^-1 J_w^T + damping I) lambda = a_des - p_ddot(q, qd, ydd_free)
 *     ydd      = FD(q, qd, tau, f_ext + world wrenches [p x lambda_c ; lambda_c] on bodies[c])
 *   a_des     NULL (zero) or [B][n][3]: the world-frame acceleration each point shall have (the caller puts a Baumgarte term here)
 *   damping   mu >= 0, finite
 *   ydd [B][nv], lambda [B][n][3]   outputs; lambda: world-frame forces ON the bodies at the points
 *   ydd_free  NULL or [B][nv]: the unconstrained accelerations
 * The result satisfies p_ddot(ydd) = a_des - mu lambda: the rigid constraint for mu = 0 and independent contacts.  Redundant contacts
 * (several points on one foot) make the matrix singular and need mu > 0.  The matrix is factored per state by Cholesky
 * (contact_kernels.hip): a pivot that is not positive or not finite gives NaN in that state's lambda and ydd (ydd_free is not
 * affected), the call still returns GRBDA_OK, and the state is counted in the counter behind grbda_spd_bad_pivots.
 * Per chunk of the batch: forward dynamics, poses, twists, inverse OSIM, one solve kernel, forward dynamics -- on every plan that
 * grbda_inv_osim_*, grbda_body_twists_* and grbda_aba_* with f_ext accept.
 *
 * Errors, all decided on the host before anything is enqueued: GRBDA_EINVAL for NULL required pointers, n_contacts outside 1 .. 8, a
 * body index out of range, a damping that is negative or not finite, no output asked for, outputs that overlap inputs or each other.
 * B == 0: GRBDA_OK.  No synchronisation, no allocation beyond the scratch slab and the work slab (chunked like the other pipelines,
 * GRBDA_WORK_MAX_MB): capturable after one eager call of the same B and n_contacts on the stream; gravity is read at launch.
 * The _host_ variants take host arrays (allocate, copy and synchronise per call). */
int grbda_contact_points_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, int n_contacts,
                             const int *bodies, const double *offsets, double *pos, double *vel, double *acc, size_t B, int device,
                             void *stream);
int grbda_contact_points_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, int n_contacts, const int *bodies,
                             const double *offsets, float *pos, float *vel, float *acc, size_t B, int device, void *stream);
int grbda_contact_dynamics_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *f_ext,
                               int n_contacts, const int *bodies, const double *offsets, const double *a_des, double damping, double *ydd,
                               double *lambda, double *ydd_free, size_t B, int device, void *stream);
int grbda_contact_dynamics_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, const float *f_ext,
                               int n_contacts, const int *bodies, const double *offsets, const float *a_des, double damping, float *ydd,
                               float *lambda, float *ydd_free, size_t B, int device, void *stream);
/* What grbda_contact_dynamics_* launches its solve kernel with for n_contacts (1 .. 8) in this precision (32 | 64): the states per
 * workgroup (64, 32 or 16), the dynamic LDS of a workgroup in bytes, and the most workgroups one launch has -- the CUs of `device` times
 * the workgroups a CU holds; batches beyond grid_cap * lanes states take further trips of the grid.  device < 0 touches no device and
 * reports grid_cap for a single CU.  The launch reads the same record (contact_kernels.hip, contact_solve_launch).  The solve of
 * grbda_contact_impulse_* (below) launches from that record too: its LDS footprint is the same triangle plus one right-hand side. */
int grbda_contact_solve_launch(int n_contacts, int precision, int device, int *lanes, size_t *lds_bytes, size_t *grid_cap);
int grbda_contact_points_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, int n_contacts,
                                  const int *bodies, const double *offsets, double *pos, double *vel, double *acc, size_t B, int device);
int grbda_contact_dynamics_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, const double *f_ext,
                                    int n_contacts, const int *bodies, const double *offsets, const double *a_des, double damping,
                                    double *ydd, double *lambda, double *ydd_free, size_t B, int device);

/* ---- contact impulses: the instant a contact closes -----------------------------------------------------------------------------
 * A point that touches down with a velocity loses it in one instant: the velocity-level twin of the solve above (Pinocchio:
 * impulseDynamics; Crocoddyl's impulse models).  Contacts are described as for grbda_contact_dynamics_*: n_contacts in 1 .. 8, host
 * arrays bodies[n] and offsets[n][3]; every other array is a device array, row-major.  With J_w [3 n][nv] the world-frame Jacobian of
 * the points, v- = J_w qd their velocities before the impact (the vel of grbda_contact_points_*), e = restitution and mu = damping:
 *     (J_w H^-1 J_w^T + mu I) Lambda = v_des - (1 + e) v-
 *     qd_next = qd + H^-1 J_w^T Lambda
 *   v_des        NULL (zero) or [B][n][3]: world-frame velocity the points shall have after the impact (before restitution)
 *   restitution  e in [0, 1], finite;  damping  mu >= 0, finite
 *   qd_next [B][nv], impulse [B][n][3]   outputs; impulse: world-frame impulses ON the bodies at the points
 * The result satisfies J_w qd_next = v_des - e v- - mu Lambda: for e = 0, mu = 0 and independent contacts the plastic impact (the points
 * stop); e = 1, mu = 0, v_des = 0 conserves the kinetic energy.  q is not changed by an impact.  Gravity and tau do not enter: finite
 * forces give no impulse over an instant.  Redundant contacts need mu > 0.  The matrix is the one of the solve above, factored per state
 * by the same Cholesky: a pivot that is not positive or not finite gives NaN in that state's impulse and qd_next, the call still returns
 * GRBDA_OK, and the state is counted in the counter behind grbda_spd_bad_pivots.
 * Per chunk of the batch: poses, twists, inverse OSIM, one solve kernel, two forward dynamics at rest (with and without the impulses'
 * wrenches: their difference is H^-1 J_w^T Lambda) and one element-wise kernel -- on every plan grbda_contact_dynamics_* accepts.
 *
 * Errors, all decided on the host before anything is enqueued: GRBDA_EINVAL for a NULL plan, q, qd, qd_next or impulse, n_contacts
 * outside 1 .. 8, a body index out of range, a damping that is negative or not finite, a restitution that is not finite or outside
 * [0, 1], outputs that overlap inputs or each other -- except qd_next == qd (equal pointers), which is allowed as in grbda_integrate_*:
 * a chunk reads its rows of qd before it writes them.  B == 0: GRBDA_OK.  No synchronisation, no allocation beyond the scratch slab and
 * the work slab (chunked like the other pipelines, GRBDA_WORK_MAX_MB): capturable after one eager call of the same B and n_contacts on
 * the stream.  The _host_ variant takes host arrays (allocates, copies and synchronises per call). */
int grbda_contact_impulse_f64(const grbda_plan *plan, const double *q, const double *qd, int n_contacts, const int *bodies,
                              const double *offsets, const double *v_des, double restitution, double damping, double *qd_next,
                              double *impulse, size_t B, int device, void *stream);
int grbda_contact_impulse_f32(const grbda_plan *plan, const float *q, const float *qd, int n_contacts, const int *bodies,
                              const double *offsets, const float *v_des, double restitution, double damping, float *qd_next, float *impulse,
                              size_t B, int device, void *stream);
int grbda_contact_impulse_host_f64(const grbda_plan *plan, const double *q, const double *qd, int n_contacts, const int *bodies,
                                   const double *offsets, const double *v_des, double restitution, double damping, double *qd_next,
                                   double *impulse, size_t B, int device);

/* ---- energy and centroidal quantities ------------------------------------------------------------------------------------------
 * What a trajectory is judged and controlled by (Pinocchio: computeKineticEnergy, computePotentialEnergy, centerOfMass,
 * computeCentroidalMomentumTimeVariation, ccrba), from ONE kernel per chunk (centroidal_kernels.hip) instead of grbda_body_poses_* +
 * grbda_body_twists_* and a reduction of 24 values per body outside the library.  Device arrays, row-major; all outputs in world axes.
 *
 * grbda_plan_total_mass: M = the sum of the body masses (rotors included).  Host only, no device.
 * grbda_energy_*:        kinetic[B] = 1/2 yd^T H(q) yd;  potential[B] = -g . sum_i m_i c_i, zero at the world origin, g the plan's gravity.
 * grbda_centroidal_*:    com[B][3], com_vel[B][3];  h[B][6] = [angular 3 about the centre of mass; linear 3], the centroidal momentum;
 *                        hdot[B][6], its rate at the generalized acceleration ydd (the true one, as for grbda_body_twists_*).  Without
 *                        external forces and with ydd = FD(q, qd, tau), a floating-base model has hdot = [0; M g]; external forces add
 *                        their wrenches about the centre of mass.  There is no f_ext argument: they enter through ydd.
 * grbda_centroidal_matrix_*: A[B][6][nv] with h = A(q) yd (the centroidal momentum matrix).  Momentum is linear in yd, so column j is
 *                        the h of the state (q, e_j): evaluated over the expanded batch (nv rows per state) with the same kernel -- the
 *                        exact difference form of grbda_mass_matrix_* above (no step size enters), chunked so that the work slab
 *                        (nv (nq + nv + 2 span_vel) scalars per state) stays within GRBDA_WORK_MAX_MB.
 *
 * Any output may be NULL, not all of them.  kinetic, com_vel and h need qd; hdot needs qd and ydd; inputs no requested output needs may
 * be NULL (positions alone never touch qd).  q, qd, ydd as for the inverse dynamics (implicit clusters: spanning positions on the
 * manifold).  Accepted on every plan that grbda_body_twists_* accepts (roll-pitch-yaw base, implicit clusters, the spanning-tree route).
 * Errors, all decided on the host before anything is enqueued: GRBDA_EINVAL for a NULL plan, a missing required pointer, no output asked
 * for, outputs that overlap inputs or each other; GRBDA_EUNSUPPORTED (text in grbda_last_error()) for com, com_vel, h, hdot or A when the
 * total mass is not positive.  B == 0: GRBDA_OK.  The calls only enqueue: no synchronisation, no allocation beyond the scratch slab and
 * the work slab (the spanning rates; chunked like the other pipelines) -- capturable after one eager call of the same B on the stream;
 * gravity is read at launch.  The _host_ variants take host arrays (allocate, copy and synchronise per call). */
int grbda_plan_total_mass(const grbda_plan *plan, double *mass);
int grbda_energy_f64(const grbda_plan *plan, const double *q, const double *qd, double *kinetic, double *potential, size_t B, int device,
                     void *stream);
int grbda_energy_f32(const grbda_plan *plan, const float *q, const float *qd, float *kinetic, float *potential, size_t B, int device,
                     void *stream);
int grbda_centroidal_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double *com, double *com_vel,
                         double *h, double *hdot, size_t B, int device, void *stream);
int grbda_centroidal_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, float *com, float *com_vel, float *h,
                         float *hdot, size_t B, int device, void *stream);
int grbda_centroidal_matrix_f64(const grbda_plan *plan, const double *q, double *A, size_t B, int device, void *stream);
int grbda_centroidal_matrix_f32(const grbda_plan *plan, const float *q, float *A, size_t B, int device, void *stream);
int grbda_energy_host_f64(const grbda_plan *plan, const double *q, const double *qd, double *kinetic, double *potential, size_t B,
                          int device);
int grbda_centroidal_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double *com, double *com_vel,
                              double *h, double *hdot, size_t B, int device);

/* ---- convenience: host pointers (single-state facade calls, small batches) ------------------ */
/* allocate, copy in, run on `device`, copy out, synchronise.  Still the HIP path. */
int grbda_aba_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau,
                       const double *f_ext, double *ydd, size_t B, int device);
int grbda_rnea_host_f64(const grbda_plan *plan, const double *q, const double *qd,
                        const double *ydd, const double *f_ext, double *tau, size_t B, int device);

/* the same on HOST arrays (allocate, copy in, run, copy out, synchronise): single-state calls of the C++ facade */
int grbda_body_poses_host_f64(const grbda_plan *plan, const double *q, double *Xa, size_t B, int device);
int grbda_body_twists_host_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double *V, size_t B,
                               int device);
int grbda_apply_test_force_host_f64(const grbda_plan *plan, const double *q, int body, const double offset[3],
                                    const double *force, double *lambda_inv, double *dstate, size_t B, int device);
int grbda_inv_osim_host_f64(const grbda_plan *plan, const double *q, int n_contacts, const int *bodies,
                            const double *offsets, double *Linv, double *J, size_t B, int device);

/* ---- one process, several devices --------------------------------------------------------------- */
/* HOST arrays, batch split into n_gpus contiguous shards on devices 0 .. n_gpus-1 (states are independent, the
 * plan is replicated, no collective): per shard allocate, copy in, run, copy out on its own stream, all shards
 * in flight together; returns when every shard is back.  A convenience for callers that are not one process per
 * GPU (bench.py is: torch.distributed over RCCL); the copies cross PCIe, so this is never the benchmarked rate. */
int grbda_aba_sharded_f32(const grbda_plan *plan, const float *q, const float *qd, const float *tau, float *ydd,
                          size_t B, int n_gpus);
int grbda_aba_sharded_f64(const grbda_plan *plan, const double *q, const double *qd, const double *tau, double *ydd,
                          size_t B, int n_gpus);
int grbda_rnea_sharded_f32(const grbda_plan *plan, const float *q, const float *qd, const float *ydd, float *tau,
                           size_t B, int n_gpus);
int grbda_rnea_sharded_f64(const grbda_plan *plan, const double *q, const double *qd, const double *ydd, double *tau,
                           size_t B, int n_gpus);

/* The same split for shards that are ALREADY RESIDENT on their devices ("batches of independent states shard
 * trivially across the GPUs of one node with a gather of results only"; the reference has no counterpart -- one
 * ClusterTreeModel::forwardDynamics call is one state on one core, ClusterTreeDynamics.cpp:85-152).  One process, n_gpus
 * shards: shard g = B[g] states in DEVICE arrays q[g], qd[g], tau[g] on device devices[g] (devices == NULL: 0 .. n_gpus-1),
 * launched on streams[g] (streams == NULL or a NULL entry: that device's default stream; two shards on one device need
 * distinct streams).  The plan is replicated per device on first use; there is no data-path collective.
 *   gathered == NULL: every shard writes ydd[g] (its own device); nothing else happens.
 *   gathered != NULL: a DEVICE array [sum B][nv] on devices[0]; the slab of shard g lands at row offset B[0] + .. + B[g-1] by
 *     hipMemcpyPeerAsync on streams[g] (peer access is enabled where the devices allow it: the copy then crosses xGMI with no
 *     host hop); a shard on devices[0] computes straight into its place when ydd is NULL or ydd[g] is NULL.  Shards on other
 *     devices need their own output slab ydd[g].  streams[0] is made to wait for every shard's copy (events), so work enqueued
 *     on streams[0] after the call sees the whole gathered array.
 * Enqueues only, like every device-pointer entry point: no synchronisation, no host copies.  GRBDA_EINVAL for null / out of
 * range arguments, GRBDA_ENODEVICE without a HIP device. */
int grbda_aba_sharded_dev_f32(const grbda_plan *plan, int n_gpus, const int *devices, const float *const *q, const float *const *qd,
                              const float *const *tau, float *const *ydd, const size_t *B, void *const *streams, float *gathered);
int grbda_aba_sharded_dev_f64(const grbda_plan *plan, int n_gpus, const int *devices, const double *const *q, const double *const *qd,
                              const double *const *tau, double *const *ydd, const size_t *B, void *const *streams, double *gathered);
int grbda_rnea_sharded_dev_f32(const grbda_plan *plan, int n_gpus, const int *devices, const float *const *q, const float *const *qd,
                               const float *const *ydd, float *const *tau, const size_t *B, void *const *streams, float *gathered);
int grbda_rnea_sharded_dev_f64(const grbda_plan *plan, int n_gpus, const int *devices, const double *const *q, const double *const *qd,
                               const double *const *ydd, double *const *tau, const size_t *B, void *const *streams, double *gathered);

/* ---- measurement hook -------------------------------------------------------------------------- */
/* Average duration in milliseconds of `iters` back-to-back launches of the ABA (kind 0) or RNEA
 * (kind 1) kernel, measured with hipEvents recorded on `stream` around the launches (the stream
 * the kernel runs on).  precision: 32 or 64. */
int grbda_time_kernel(const grbda_plan *plan, int kind, int precision, const void *q, const void *qd,
                      const void *x, void *out, size_t B, int device, void *stream, int iters,
                      float *avg_ms);

/* number of usable HIP devices (0 when there is none); never fails */
int grbda_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* GRBDA_HIP_H */
