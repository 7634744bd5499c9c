// capi.cpp -- implementation of include/grbda_hip.h on top of plan.cpp and kernels.hip.
#include <hip/hip_runtime.h>

#include <array>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/grbda_hip.h"
#include "../../include/grbda_hip_vjp.h"
#include "../../include/grbda_hip_step_vjp.h"
#include "../../include/grbda_hip_jvp.h"
#include "../../include/grbda_hip_wrench.h"
#include "../../include/grbda_hip_contact_step.h"
#include "../../include/grbda_hip_bodies.h"
#include "../../include/grbda_hip_jacobians.h"
#include "../../include/grbda_hip_jacobian_products.h"
#include "../../include/grbda_model_desc.h"
#include "devplan.h"

namespace grbda_hip {
int urdf_to_blob(const char *const *paths, int n_paths, int ori_repr, std::vector<unsigned char> &blob,
                 std::string &err);

}  // namespace grbda_hip

using namespace grbda_hip;

namespace {

thread_local std::string g_last_error;

int set_err(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}
int hip_err(hipError_t e, const char *what)
{
    return set_err(GRBDA_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// device copies of the tables of one chain program (plan.h, ChainProgram / RneaChainProgram)
struct ChainTables {
    ChainSeg *segs = nullptr;
    ChainLink *links = nullptr;
    ChainPair *pairs = nullptr;
    ChainFree *frees = nullptr;
    ChainDiff *diffs = nullptr;
    ChainGen *gens = nullptr;
    ChainGenBody *gbodies = nullptr;
};
struct RneaChainTables {
    RneaSeg *segs = nullptr;
    RneaLink *links = nullptr;
    RneaPair *pairs = nullptr;
    RneaFree *frees = nullptr;
    RneaDiff *diffs = nullptr;
    ChainGen *gens = nullptr;
    ChainGenBody *gbodies = nullptr;
};
// per-(device) copies of the plan tables; per-(device, stream) scratch slabs
struct DeviceTables {
    Step *aba_steps = nullptr, *rnea_steps = nullptr;
    // [0] f32, [1] f64, [2] f32 + external forces, [3] f64 + external forces, [4] f32 split layout
    ClusterRec *clusters[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ClusterRec *rnea_clusters[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t *cints = nullptr;
    int32_t *acc_k[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t *dq_map = nullptr;  // per velocity index: (kind, position index, component), see grbda_fd_dq_*
    BodyRec *bodies[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};       // ABA slots
    BodyRec *rnea_bodies[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // RNEA slots
    double *consts64 = nullptr;
    float *consts32 = nullptr;
    // the chain programs HostPlan::chain[s] / rchain[s] that are ok, by ChainSlot (plan.h).  chain[SLOT_F32_WIDE] stays empty: forward
    // dynamics at four wavefronts per SIMD has no route
    ChainTables chain[kChainSlots];
    RneaChainTables rchain[kChainSlots];
    CrbaBody *crba_bodies = nullptr;
    DerivBody *deriv_bodies = nullptr;
    uint64_t *deriv_related = nullptr;  // DerivProgram::related
    MinvBody *minv_bodies = nullptr;    // DerivProgram::minv (plan.h, MinvProgram): record offsets per body ...
    int32_t *minv_coltab = nullptr;     // ... and the column programs of minv_mfma_kernel
    int32_t *related_table = nullptr;   // HostPlan::related_table (plans of the wide route with more than 64 velocities)
    int32_t *span_q = nullptr, *span_v = nullptr, *crow = nullptr;  // grbda_plan::span_q / span_v / crow
    int32_t *centroidal_rows = nullptr;  // per body (own first scratch row or -1, parent's first row or -1): centroidal_kernels.hip
    int n_cu = 0;
    unsigned long long *bad_count = nullptr;  // this device's counter of states with a pivot that is not positive (deriv_kernels.hip)
};
struct Scratch {
    void *ptr = nullptr;
    size_t bytes = 0;
};
using SlabPool = std::map<std::pair<int, void *>, Scratch>;  // by (device, stream)

// every entry point that may switch the calling thread's HIP device puts it back on return (torch and other users of the
// runtime in the same thread keep their current device)
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define GRBDA_CALL_SCOPE(p) DeviceGuard device_guard_; std::unique_lock<std::recursive_mutex> plan_lock_((p)->mu)

int env_int(const char *name, int dflt)
{
    const char *v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}

constexpr int kLayouts = 5;
const Layout &layout_of(const HostPlan &h, int w)
{
    return w == 0 ? h.lay32 : (w == 1 ? h.lay64 : (w == 2 ? h.lay32x : (w == 3 ? h.lay64x : h.lay32s)));
}

}  // namespace

struct grbda_plan {
    HostPlan host;
    std::vector<unsigned char> blob;
    // Held from the moment a call sizes its scratch / work buffers until its last kernel is ENQUEUED: a second thread
    // that needs a bigger buffer for the same (device, stream) can then only free the old one after the first thread's
    // launches are in the stream (hipFree waits for them).  Recursive: the derived entry points call run().
    mutable std::recursive_mutex mu;
    mutable std::map<int, DeviceTables> dev;
    mutable SlabPool scratch;
    mutable SlabPool work;       // expanded batches of the derived quantities
    mutable SlabPool work_cvt;   // fp64 copies of fp32 inputs (through_f64)
    mutable SlabPool work_proj;  // projection_run (called from inside the users of `work`)
    mutable SlabPool work_vjp;   // vjp_run (its id_derivs stage carves `work` on the difference routes)
    mutable SlabPool work_step_vjp;  // step_vjp_run / rollout_vjp (they call vjp_run, which carves work_vjp)
    mutable SlabPool work_jvp;       // jvp_run (its id_derivs stage carves `work` on the difference routes)
    mutable SlabPool work_step_jvp;  // step_jvp_run: dydd between jvp_run and the integrate kernel
    mutable SlabPool work_contact;   // the scheduled contacts (their sparse-wrench stage carves `work` on its fallback routes)
    // the chunk decision of the last eager analytic_derivs call per (device, stream): a capture of the same call replays it
    struct DerivChunk {
        size_t B = 0, per_state_bytes = 0, chunk = 0;
        bool need_d = false, ydd_all = false;
    };
    mutable std::map<std::pair<int, void *>, DerivChunk> deriv_chunk;
    PlanOptions opt;  // read once, when the plan is made (plan_options_from_env)
    // Models with implicit clusters: the spanning-tree model as a plan of its own (plan.cpp, make_spanning_blob) -- the analytic
    // derivatives and the mass matrix are taken on it and projected with the per-state G (manifold_kernels.hip).  span_q / span_v:
    // spanning position / velocity index of every body; crow: first row of every implicit cluster in the coupling slab.
    grbda_plan *span = nullptr;
    ~grbda_plan() { if (span) grbda_plan_free(span); }
    std::vector<int32_t> span_q, span_v, crow;
    int n_cpl_rows = 0;
    bool has_trig = false;     // some implicit cluster is a trig-polynomial constraint (its sine / cosine cache takes dynamic LDS of the manifold constraint kernel)
    int constraint_shape = 0;  // manifold_kernels.hip, launch_manifold_constraint: 0 structured, 1 beyond the limits, 2 at most 4 bodies / 2 coordinates
};

namespace {

hipError_t up(const void *src, size_t bytes, void **dst)
{
    hipError_t e = hipMalloc(dst, bytes ? bytes : 16);
    if (e != hipSuccess) return e;
    return bytes ? hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
}
template <class R>
hipError_t up(const std::vector<R> &src, R **dst)
{
    return up(src.data(), src.size() * sizeof(R), reinterpret_cast<void **>(dst));
}
// upload and release of the tables of one chain program (either family) on the current device
template <class Program, class Tables>
int upload_chain_program(const Program &cp, Tables &ct)
{
    hipError_t e;
    if ((e = up(cp.segs, &ct.segs)) != hipSuccess || (e = up(cp.links, &ct.links)) != hipSuccess || (e = up(cp.pairs, &ct.pairs)) != hipSuccess ||
        (e = up(cp.frees, &ct.frees)) != hipSuccess || (e = up(cp.diffs, &ct.diffs)) != hipSuccess || (e = up(cp.gens, &ct.gens)) != hipSuccess ||
        (e = up(cp.gbodies, &ct.gbodies)) != hipSuccess)
        return hip_err(e, "plan upload");
    if ((e = set_max_dynamic_lds_chain()) != hipSuccess) return hip_err(e, "hipFuncSetAttribute");
    if ((e = set_max_dynamic_lds_chain_wrench()) != hipSuccess) return hip_err(e, "hipFuncSetAttribute");
    return 0;
}
template <class Tables>
void free_chain_tables(Tables &ct)
{
    for (void *ptr : {static_cast<void *>(ct.segs), static_cast<void *>(ct.links), static_cast<void *>(ct.pairs), static_cast<void *>(ct.frees),
                      static_cast<void *>(ct.diffs), static_cast<void *>(ct.gens), static_cast<void *>(ct.gbodies)})
        (void)hipFree(ptr);
}

// the CU count every persistent grid is sized by
hipError_t device_cu_count(int device, int *n_cu)
{
    hipDeviceProp_t prop;
    if (hipError_t e = hipGetDeviceProperties(&prop, device); e != hipSuccess) return e;
    *n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return hipSuccess;
}

// Scratch rows of centroidal_kernel (devplan.h): bodies with children get kCentroidalBodyRows rows each, in body order; leaves none.
struct CentroidalRows {
    std::vector<int32_t> rows;  // per body: own first row or -1, the tree parent's first row or -1
    int n_parent_bodies = 0;
};
CentroidalRows centroidal_rows(const HostPlan &h)
{
    CentroidalRows r;
    const std::vector<BodyRec> &bodies = h.lay64.bodies;
    r.rows.assign(2 * bodies.size(), -1);
    for (size_t b = 0; b < bodies.size(); b++)
        if (bodies[b].has_child) r.rows[2 * b] = kCentroidalBodyRows * r.n_parent_bodies++;
    for (size_t b = 0; b < bodies.size(); b++)
        if (bodies[b].parent >= 0) r.rows[2 * b + 1] = r.rows[2 * static_cast<size_t>(bodies[b].parent)];
    return r;
}

int ensure_device(const grbda_plan *p, int device, DeviceTables **out)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return set_err(GRBDA_ENODEVICE, "no HIP device available (there is no CPU fallback)");
    if (device < 0 || device >= count) return set_err(GRBDA_EINVAL, "device index out of range");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_err(e, "hipSetDevice");
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    auto it = p->dev.find(device);
    if (it != p->dev.end()) {
        *out = &it->second;
        return 0;
    }
    DeviceTables t;
    const HostPlan &h = p->host;
    std::vector<float> c32(h.consts.begin(), h.consts.end());
    if ((e = up(h.aba_steps.data(), h.aba_steps.size() * sizeof(Step), (void **)&t.aba_steps)) != hipSuccess ||
        (e = up(h.rnea_steps.data(), h.rnea_steps.size() * sizeof(Step), (void **)&t.rnea_steps)) != hipSuccess ||
        (e = up(h.consts.data(), h.consts.size() * sizeof(double), (void **)&t.consts64)) != hipSuccess ||
        (e = up(c32.data(), c32.size() * sizeof(float), (void **)&t.consts32)) != hipSuccess ||
        (e = up(h.cints.data(), h.cints.size() * sizeof(int32_t), (void **)&t.cints)) != hipSuccess)
        return hip_err(e, "plan upload");
    {
        // tangent-space perturbation of the positions (UnitTests/testHelpers.hpp:50-112): kind 0 q[i] += d,
        // 1 free-base rotation (quat += quat x (0, d e_a) / 2), 2 free-base translation (pos += R^T d e_a),
        // (implicit-loop clusters: kind 0 on the independent spanning position + re-projection of the dependent ones)
        std::vector<int32_t> map(static_cast<size_t>(h.nv) * 3, 0);
        for (const ClusterRec &c : h.lay64.clusters)
            for (int a = 0; a < c.n; a++) {
                int32_t *e = &map[static_cast<size_t>(c.v_index + a) * 3];
                if (c.kind == CK_FREE && h.ori_repr == 0) {
                    e[0] = a < 3 ? 1 : 2;
                    e[1] = c.q_index;
                    e[2] = a % 3;
                } else if (c.kind == CK_FREE) {
                    // roll-pitch-yaw base: the reference's plus() only special-cases the quaternion (testHelpers.hpp:49-74);
                    // every other position vector is q + dq
                    e[0] = 0;
                    e[1] = c.q_index + a;
                } else if (c.kind == CK_LOOP) {
                    // implicit cluster: the a-th INDEPENDENT spanning position moves, the dependent ones are put back on
                    // phi(q) = 0 by the Newton projection (derived(), DM_DQ): the derivative on the constraint manifold
                    e[0] = 0;
                    e[1] = c.q_index + h.cints[c.iofs + 2 + a];
                } else {
                    e[0] = 0;
                    e[1] = c.q_index + a;
                }
            }
        if ((e = up(map.data(), map.size() * sizeof(int32_t), (void **)&t.dq_map)) != hipSuccess) return hip_err(e, "plan upload");
    }
    for (int w = 0; w < kLayouts; w++) {
        const Layout &L = layout_of(h, w);
        if ((e = up(L.clusters.data(), L.clusters.size() * sizeof(ClusterRec), (void **)&t.clusters[w])) != hipSuccess ||
            (e = up(L.rnea_clusters.data(), L.rnea_clusters.size() * sizeof(ClusterRec), (void **)&t.rnea_clusters[w])) != hipSuccess ||
            (e = up(L.bodies.data(), L.bodies.size() * sizeof(BodyRec), (void **)&t.bodies[w])) != hipSuccess ||
            (e = up(L.rnea_bodies.data(), L.rnea_bodies.size() * sizeof(BodyRec), (void **)&t.rnea_bodies[w])) != hipSuccess ||
            (e = up(L.acc_k.data(), L.acc_k.size() * sizeof(int32_t), (void **)&t.acc_k[w])) != hipSuccess)
            return hip_err(e, "plan upload");
    }
    for (int s = 0; s < kChainSlots; s++) {
        if (h.rchain[s].ok)
            if (int rc = upload_chain_program(h.rchain[s], t.rchain[s])) return rc;
        if (h.chain[s].ok && s != SLOT_F32_WIDE)
            if (int rc = upload_chain_program(h.chain[s], t.chain[s])) return rc;
    }
    if (h.crba.ok && (e = up(h.crba.bodies.data(), h.crba.bodies.size() * sizeof(CrbaBody), (void **)&t.crba_bodies)) != hipSuccess)
        return hip_err(e, "plan upload");
    if (h.deriv.ok) {
        if ((e = up(h.deriv.bodies.data(), h.deriv.bodies.size() * sizeof(DerivBody), (void **)&t.deriv_bodies)) != hipSuccess)
            return hip_err(e, "plan upload");
    }
    if (!h.deriv.related.empty() &&
        (e = up(h.deriv.related.data(), h.deriv.related.size() * sizeof(uint64_t), (void **)&t.deriv_related)) != hipSuccess)
        return hip_err(e, "plan upload");
    if (!h.related_table.empty() &&
        (e = up(h.related_table.data(), h.related_table.size() * sizeof(int32_t), (void **)&t.related_table)) != hipSuccess)
        return hip_err(e, "plan upload");
    if (h.deriv.ok && h.deriv.minv.ok &&
        ((e = up(h.deriv.minv.bodies.data(), h.deriv.minv.bodies.size() * sizeof(MinvBody), (void **)&t.minv_bodies)) != hipSuccess ||
         (e = up(h.deriv.minv.coltab.data(), h.deriv.minv.coltab.size() * sizeof(int32_t), (void **)&t.minv_coltab)) != hipSuccess))
        return hip_err(e, "plan upload");
    if (p->span) {
        if ((e = up(p->span_q.data(), p->span_q.size() * sizeof(int32_t), (void **)&t.span_q)) != hipSuccess ||
            (e = up(p->span_v.data(), p->span_v.size() * sizeof(int32_t), (void **)&t.span_v)) != hipSuccess ||
            (e = up(p->crow.data(), p->crow.size() * sizeof(int32_t), (void **)&t.crow)) != hipSuccess)
            return hip_err(e, "plan upload");
    }
    if ((e = up(centroidal_rows(h).rows, &t.centroidal_rows)) != hipSuccess) return hip_err(e, "plan upload");
    if ((e = device_cu_count(device, &t.n_cu)) != hipSuccess) return hip_err(e, "hipGetDeviceProperties");
    if ((e = set_max_dynamic_lds()) != hipSuccess) return hip_err(e, "hipFuncSetAttribute");
    if ((e = set_max_dynamic_lds_deriv()) != hipSuccess) return hip_err(e, "hipFuncSetAttribute");
    if ((e = set_max_dynamic_lds_minv()) != hipSuccess) return hip_err(e, "hipFuncSetAttribute");
    if ((e = set_max_dynamic_lds_contact()) != hipSuccess) return hip_err(e, "hipFuncSetAttribute");
    if ((e = set_max_dynamic_lds_contact_step()) != hipSuccess) return hip_err(e, "hipFuncSetAttribute");
    t.bad_count = spd_bad_count_address();
    auto ins = p->dev.emplace(device, t);
    *out = &ins.first->second;
    return 0;
}

bool is_capturing(void *stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return stream && hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// The slab of `pool` for (device, stream), grown on demand; `noun` names it in the refusal.
// (Growing frees first, and hipFree waits for every stream of the device.  An entry point that sizes the slab more than once -- the
// derivatives: the forward dynamics' share, then the recursion's -- grows it inside ONE call when the stream is new to the plan, so that
// stream's first call is a device-wide synchronisation; later calls of the same or a smaller batch allocate nothing.)
int ensure_slab(const grbda_plan *p, SlabPool &pool, const char *noun, int device, void *stream, size_t bytes, void **out)
{
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    Scratch &s = pool[{device, stream}];
    if (s.bytes < bytes) {
        // A stream under capture must not see hipFree / hipMalloc, and a graph captured earlier on this (device, stream)
        // holds the slab's address: growing is refused while the stream captures (reserve with one eager call of the
        // largest batch first, include/grbda_hip.h "Graph capture")
        if (is_capturing(stream))
            return set_err(GRBDA_EINVAL, std::string(noun) + " would have to grow during stream capture: run the largest batch once on "
                                                             "this stream before capturing");
        hipError_t e;
        if (s.ptr && (e = hipFree(s.ptr)) != hipSuccess) return hip_err(e, "hipFree");
        s.ptr = nullptr;
        s.bytes = 0;
        if ((e = hipMalloc(&s.ptr, bytes)) != hipSuccess) return hip_err(e, "hipMalloc(slab)");
        s.bytes = bytes;
    }
    *out = s.ptr;
    return 0;
}
int ensure_scratch(const grbda_plan *p, int device, void *stream, size_t bytes, void **out)
{
    return ensure_slab(p, p->scratch, "the per-stream scratch slab", device, stream, bytes, out);
}
// The per-(device, stream) work slab of the derived quantities, grown on demand under the same rule as the scratch slab: never
// while the stream captures (a graph captured earlier holds the old address).
int ensure_work(const grbda_plan *p, SlabPool &pool, int device, void *stream, size_t bytes, void **out)
{
    return ensure_slab(p, pool, "a per-stream work buffer", device, stream, bytes, out);
}

// Upper bound of a work-slab request of the chunked pipelines (derivatives, projection): what the call site asks for (1-16 GiB, sized so that a
// million states go through in a few chunks), cut to GRBDA_WORK_MAX_MB when that is set and to
//     max(the slab this (device, stream) already holds, a quarter of the memory that is FREE on the device right now, 256 MiB)
// so that (a) a call never shrinks below what it already owns -- the chunk, and with it the timing, of a repeated call is reproducible whatever
// else has been allocated since -- and (b) a stream that is being CAPTURED derives its chunk from the held slab alone (no hipMemGetInfo, no
// growth: INTEGRATION.md's rule "run the largest batch once on the stream before capturing" then always suffices).  The slabs are kept per
// (device, stream) and never shrink by themselves; grbda_plan_release_work() hands them back.
size_t work_budget(const grbda_plan *p, const SlabPool &pool, int device, void *stream, size_t want)
{
    size_t cap = want;
    size_t held = 0;
    {
        std::lock_guard<std::recursive_mutex> lk(p->mu);
        const auto it = pool.find({device, stream});
        if (it != pool.end()) held = it->second.bytes > 256 ? it->second.bytes - 256 : 0;
    }
    const bool capturing = is_capturing(stream);
    if (capturing && held > 0) return cap < held ? cap : held;
    size_t free_b = 0, total_b = 0;
    if (!capturing && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
        size_t limit = free_b / 4;
        if (limit < (256ull << 20)) limit = 256ull << 20;
        if (limit < held) limit = held;
        if (cap > limit) cap = limit;
    }
    const int mb = env_int("GRBDA_WORK_MAX_MB", 0);
    if (mb > 0 && cap > (static_cast<size_t>(mb) << 20)) cap = static_cast<size_t>(mb) << 20;
    return cap;
}

template <class T>
DevPlan<T> make_dev_plan(const grbda_plan *p, const DeviceTables &t, bool rnea, bool fext)
{
    DevPlan<T> d;
    const HostPlan &h = p->host;
    d.bad_count = t.bad_count;
    d.steps = rnea ? t.rnea_steps : t.aba_steps;
    d.n_steps = static_cast<int>(rnea ? h.rnea_steps.size() : h.aba_steps.size());
    int w = (sizeof(T) == 4 ? 0 : 1) + (fext ? 2 : 0);
    // f32 fast path: the split layout when it exists for this kernel
    const bool split = w == 0 && (rnea ? h.lay32s.split_rnea : h.lay32s.split_aba);
    if (split) w = 4;
    const Layout &L = layout_of(h, w);
    d.clusters = rnea ? t.rnea_clusters[w] : t.clusters[w];
    d.cints = t.cints;
    d.acc_k = t.acc_k[w];
    d.bodies = rnea ? t.rnea_bodies[w] : t.bodies[w];
    d.consts = sizeof(T) == 4 ? reinterpret_cast<const T *>(t.consts32) : reinterpret_cast<const T *>(t.consts64);
    d.nq = h.nq;
    d.nv = h.nv;
    d.n_lds_slots = rnea ? L.n_lds_rnea : L.n_lds_aba;
    d.n_glb_slots = rnea ? L.n_glb_rnea : L.n_glb_aba;
    d.ori_repr = h.ori_repr;
    d.general = fext ? 1 : 0;
    for (const ClusterRec &cr : L.clusters) d.general |= cr.kind == CK_LOOP;
    d.split = split ? 1 : 0;
    d.n_bodies = h.n_bodies;
    for (int i = 0; i < 6; i++) d.a_root[i] = static_cast<T>(-h.gravity[i]);
    return d;
}

template <class T>
const T *consts_of(const DeviceTables &t)
{
    return sizeof(T) == 4 ? reinterpret_cast<const T *>(t.consts32) : reinterpret_cast<const T *>(t.consts64);
}

// ---- kernel argument blocks of the chain kernels: everything that follows from (plan, device, program slot) -----------------------
// The call sites state only what is special to them.  The generic-cluster tables of a program without generic clusters are passed as
// null (no_gens), the segment tables of a single-cluster launch likewise (gen1_only): the values these paths have always passed.
template <class Dev, class Program, class Tables>
void fill_chain_tables(Dev &d, const Program &cp, const Tables &ct)
{
    d.segs = ct.segs;
    d.links = ct.links;
    d.pairs = ct.pairs;
    d.frees = ct.frees;
    d.diffs = ct.diffs;
    d.n_diffs = static_cast<int>(cp.diffs.size());
    d.gens = ct.gens;
    d.gbodies = ct.gbodies;
    d.n_gens = static_cast<int>(cp.gens.size());
    d.n_segs = static_cast<int>(cp.segs.size());
    d.n_glb_slots = cp.n_glb;
}
template <class T, class Dev>
void fill_chain_model(Dev &d, const HostPlan &h, const DeviceTables &t)
{
    d.cints = t.cints;
    d.consts = consts_of<T>(t);
    d.nq = h.nq;
    d.nv = h.nv;
    d.ori_repr = h.ori_repr;
    for (int i = 0; i < 6; i++) d.a_root[i] = static_cast<T>(-h.gravity[i]);
}
template <class T>
ChainDev<T> chain_dev(const grbda_plan *p, const DeviceTables &t, ChainSlot slot)
{
    const ChainProgram &cp = p->host.chain[slot];
    ChainDev<T> d{};  // (fuse, stage_*: 0)
    fill_chain_tables(d, cp, t.chain[slot]);
    fill_chain_model<T>(d, p->host, t);
    d.sv_global = cp.sv_global ? 1 : 0;
    d.out_lds = cp.out_lds;
    d.bad_count = t.bad_count;
    return d;
}
template <class T>
RneaChainDev<T> rnea_chain_dev(const grbda_plan *p, const DeviceTables &t, ChainSlot slot)
{
    RneaChainDev<T> d{};
    fill_chain_tables(d, p->host.rchain[slot], t.rchain[slot]);
    fill_chain_model<T>(d, p->host, t);
    return d;
}
template <class Dev>
void no_gens(Dev &d)
{
    d.gens = nullptr;
    d.gbodies = nullptr;
    d.n_gens = 0;
}
// the single-cluster kernels take their one cluster from gens[0]: no segment tables, no slab
template <class Dev>
void gen1_only(Dev &d)
{
    d.segs = nullptr;
    d.links = nullptr;
    d.pairs = nullptr;
    d.frees = nullptr;
    d.diffs = nullptr;
    d.n_diffs = d.n_segs = d.n_glb_slots = 0;
    d.n_gens = 1;
}

// ---- launch shapes ------------------------------------------------------------------------------------------------------------------
template <class T>
size_t stage_all_bytes(const HostPlan &h)  // the staging area of a tile's whole input: q, qd and tau / ydd transposed at once
{
    return static_cast<size_t>(kWave) * static_cast<size_t>(h.nq + 2 * h.nv) * sizeof(T);
}
// Persistent launch of one-wavefront workgroups, wavefronts_per_cu per CU and at most one per tile.  LDS per wavefront: the slot store, at
// least the staging area of the longest input array, and that of all three at once when the budget holds it (stage_all_fits).
// clamp_to_lds_fit: never more wavefronts than a CU's 160 KiB keep resident at once.  grid_unclamped is the grid before that clamp.
struct LaunchShape {
    size_t grid, grid_unclamped, lds_bytes;
    bool stage_all_fits;
};
LaunchShape launch_shape(int n_cu, size_t n_tiles, size_t waves_per_cu, size_t store_bytes, int nq, int nv, size_t elem, size_t lds_budget,
                         bool clamp_to_lds_fit)
{
    LaunchShape s;
    s.grid = std::min(static_cast<size_t>(n_cu) * waves_per_cu, n_tiles);
    s.grid_unclamped = s.grid;
    const size_t stage_one = static_cast<size_t>(kWave) * static_cast<size_t>(nq > nv ? nq : nv) * elem;
    const size_t stage_all = static_cast<size_t>(kWave) * static_cast<size_t>(nq + 2 * nv) * elem;
    s.lds_bytes = std::max(store_bytes, stage_one);
    if (s.lds_bytes < stage_all && stage_all <= lds_budget) s.lds_bytes = stage_all;
    s.stage_all_fits = s.lds_bytes >= stage_all;
    const size_t fit = lds_workgroups_per_cu(s.lds_bytes);
    if (clamp_to_lds_fit && fit >= 1 && fit < waves_per_cu) s.grid = std::min(s.grid, static_cast<size_t>(n_cu) * fit);
    return s;
}
// the per-stream slab: rows of kWave scalars per resident wavefront (a program's global slots + the nq + 2 nv staged input rows)
size_t scratch_bytes(size_t grid, size_t rows, size_t elem) { return grid * rows * kWave * elem + 256; }
// grid of the single-cluster kernels: what registers (waves_per_simd) and LDS hold per CU, GRBDA_GEN1_WAVES_PER_CU / _TILES_PER_WAVE
size_t gen1_grid(const grbda_plan *p, int n_cu, size_t n_tiles, int waves_per_simd, size_t lds_total)
{
    size_t per_cu = std::min(static_cast<size_t>(waves_per_simd) * 4, lds_workgroups_per_cu(lds_total));
    if (p->opt.gen1_waves_cap > 0) per_cu = std::min(per_cu, static_cast<size_t>(p->opt.gen1_waves_cap));
    size_t grid = static_cast<size_t>(n_cu) * per_cu;
    if (p->opt.gen1_tiles_per_wave > 0) grid = (n_tiles + p->opt.gen1_tiles_per_wave - 1) / p->opt.gen1_tiles_per_wave;
    return std::min(grid, n_tiles);
}
// grid of the element-wise kernels of this file: 256 threads per block in a grid-stride loop over n elements
int blocks_for(size_t n) { return static_cast<int>((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535); }
// persistent launch of an auxiliary kernel: per_cu one-wavefront workgroups per CU, at most one per tile of the B states
size_t tile_grid(int n_cu, size_t per_cu, size_t B) { return std::min(static_cast<size_t>(n_cu) * per_cu, (B + kWave - 1) / kWave); }

// ---- chunks: a batch goes through its work slab so many states at a time ----------------------------------------------------------
struct Chunk {
    size_t chunk;  // states per pass
    size_t bytes;  // the slab that holds them
};
// as many states as `cap_bytes` hold, at least one, at most the batch
Chunk fixed_chunk(size_t cap_bytes, size_t per_state_bytes, size_t B)
{
    size_t chunk = cap_bytes / per_state_bytes;
    if (chunk < 1) chunk = 1;
    if (chunk > B) chunk = B;
    return {chunk, chunk * per_state_bytes + 256};
}
size_t whole_tiles(size_t chunk)  // rounded down to tiles of kWave states, at least one
{
    chunk &= ~static_cast<size_t>(kWave - 1);
    return chunk < static_cast<size_t>(kWave) ? kWave : chunk;
}
// as many whole tiles as the budget of `pool` gives a request of `want_bytes` (work_budget), at most the batch rounded up to tiles
Chunk budgeted_chunk(const grbda_plan *p, const SlabPool &pool, int device, void *stream, size_t want_bytes, size_t per_state_bytes, size_t B)
{
    size_t chunk = whole_tiles(work_budget(p, pool, device, stream, want_bytes) / per_state_bytes);
    const size_t b_round = (B + kWave - 1) / kWave * kWave;
    if (chunk > b_round) chunk = b_round;
    return {chunk, chunk * per_state_bytes + 256};
}
// for (const auto [b0, nb] : ChunkWalk{B, chunk}): the passes over a batch of B states, nb of them from state b0 on
struct ChunkWalk {
    size_t B, chunk;
    struct Pass {
        size_t b0, nb;
    };
    struct Iter {
        size_t b0, B, chunk;
        Pass operator*() const { return {b0, B - b0 < chunk ? B - b0 : chunk}; }
        void operator++() { b0 += chunk; }
        bool operator!=(const Iter &) const { return b0 < B; }
    };
    Iter begin() const { return {0, B, chunk}; }
    Iter end() const { return {B, B, chunk}; }
};
// Typed cursor over a slab sized for `cap` scalars: take(count) hands out the next `count` of them.  A site whose per-state size is the sum
// of what it takes ends with assert(w.taken == w.cap), so that the size and the pointers cannot drift apart.
template <class T>
struct Carver {
    T *base;
    size_t cap, taken = 0;
    Carver(void *slab, size_t cap_) : base(static_cast<T *>(slab)), cap(cap_) {}
    T *take(size_t count)
    {
        assert(taken + count <= cap);
        T *r = base + taken;
        taken += count;
        return r;
    }
};

// ---- routes -------------------------------------------------------------------------------------------------------------------------
// Which kernel a batch of B states runs on a device with n_cu compute units, and on which program: ONE definition per algorithm
// (choose_aba, choose_rnea), which run() dispatches on, the launch functions take, and grbda_kernel_name formats (bench.py and the
// tests read the name to know what they exercised).
enum RoutePath { ROUTE_GEN1, ROUTE_LM, ROUTE_CHAIN, ROUTE_INTERPRETER };
struct Route {
    RoutePath path;
    ChainSlot slot;  // the program of HostPlan::chain / rchain (not ROUTE_INTERPRETER)
    int lm_waves;    // ROUTE_LM: wavefronts per tile, 2 or 4
};
// LDS of a latency-mode tile / of a single-cluster wavefront (work area + the staged input rows)
template <class T, class Program>
size_t lm_lds_bytes(const HostPlan &h, const Program &lp)
{
    return std::max(static_cast<size_t>(lp.n_lds) * kWave * sizeof(T), stage_all_bytes<T>(h));
}
template <class T, class Program>
size_t gen1_lds_bytes(const HostPlan &h, const Program &sp)
{
    return static_cast<size_t>(sp.n_lds) * kWave * sizeof(T) + stage_all_bytes<T>(h);
}
// the single-cluster kernels prefetch a state's positions into min(n + 3, 8) registers (implicit cluster: one per body) or n (explicit)
template <class T, class Program>
bool gen1_usable(const HostPlan &h, const Program &sp)
{
    if (!sp.ok || !sp.single_gen || gen1_lds_bytes<T>(h, sp) > 65536) return false;
    const ChainGen &g = sp.gens[0];
    return h.nq <= (g.kind ? std::min(g.n + 3, kMaxClusterBodies) : g.n) && g.n <= 4;
}
// Latency mode: a batch of at most one tile per SIMD would leave every SIMD with a single wavefront; a tile then goes to a workgroup of two
// wavefronts that split its limbs, and to four while that still leaves at most two wavefronts per SIMD (two tiles per CU; GRBDA_LM_WAVES=2
// keeps two).  Only the fp32 latency-mode kernels carry the differential segments.  GRBDA_NO_LATENCY_MODE=1 keeps the ordinary kernels
// (A/B runs); results agree to rounding (the base sums one partial inertia per wavefront).
template <class T, class Program>
bool lm_serves(const grbda_plan *p, const Program &lp, int waves, int n_cu, size_t n_tiles)
{
    return lp.ok && (sizeof(T) == 4 || lp.diffs.empty()) && !p->opt.no_latency_mode && !(waves == 4 && p->opt.lm_waves == 2) && n_tiles > 0 &&
           n_tiles <= static_cast<size_t>(n_cu) * (waves == 4 ? 2 : 4) && lm_lds_bytes<T>(p->host, lp) <= static_cast<size_t>(lm_lds_limit(waves));
}
template <class T>
Route choose_aba(const grbda_plan *p, int n_cu, size_t B, bool f_ext)
{
    const HostPlan &h = p->host;
    constexpr bool f64 = sizeof(T) == 8;
    const ChainSlot base = chain_slot(f64);
    if (f_ext || p->opt.no_chain || !h.chain[base].ok) return {ROUTE_INTERPRETER, base, 0};
    const size_t n_tiles = (B + kWave - 1) / kWave;
    if (gen1_usable<T>(h, h.chain[base])) return {ROUTE_GEN1, base, 0};
    for (const int waves : {4, 2})
        if (lm_serves<T>(p, h.chain[chain_slot(f64, waves)], waves, n_cu, n_tiles)) return {ROUTE_LM, chain_slot(f64, waves), waves};
    return {ROUTE_CHAIN, base, 0};
}
template <class T>
Route choose_rnea(const grbda_plan *p, int n_cu, size_t B, bool f_ext)
{
    const HostPlan &h = p->host;
    constexpr bool f64 = sizeof(T) == 8;
    const ChainSlot base = chain_slot(f64);
    if (f_ext || p->opt.no_chain || !h.rchain[base].ok) return {ROUTE_INTERPRETER, base, 0};
    const size_t n_tiles = (B + kWave - 1) / kWave;
    for (const int waves : {4, 2}) {
        const RneaChainProgram &lp = h.rchain[chain_slot(f64, waves)];
        if (lp.n_waves == waves && lm_serves<T>(p, lp, waves, n_cu, n_tiles)) return {ROUTE_LM, chain_slot(f64, waves), waves};
    }
    if (gen1_usable<T>(h, h.rchain[base])) return {ROUTE_GEN1, base, 0};
    // f32: the inverse-dynamics kernel needs 109 VGPRs, so four wavefronts per SIMD fit; models whose blocks all fit the
    // LDS of the two-per-SIMD shape (no global-slab fallback) run the program laid out for half the LDS per wavefront
    // once the batch fills 16 wavefronts per CU (MIT humanoid 0.105 -> 0.095 ms, Mini Cheetah 0.079 -> 0.070 ms; JVRC-1,
    // whose blocks spill already, loses)
    if (!f64 && h.rchain[SLOT_F32_WIDE].ok && h.rchain[base].n_glb == 0 && h.rchain[base].gens.empty() && n_tiles > static_cast<size_t>(n_cu) * 8)
        return {ROUTE_CHAIN, SLOT_F32_WIDE, 0};
    return {ROUTE_CHAIN, base, 0};
}

template <class T>
int run_chain(const grbda_plan *p, const DeviceTables &t, const Route &r, const T *q, const T *qd, const T *tau, T *ydd, size_t B, int device,
              void *stream, bool gravity = true, const WrenchList<T> *wrenches = nullptr)  // wrenches: ROUTE_CHAIN only (wrench_route)
{
    const HostPlan &h = p->host;
    const ChainProgram &cp = h.chain[r.slot];
    const size_t n_tiles = (B + kWave - 1) / kWave;
    const size_t in_rows = static_cast<size_t>(h.nq + 2 * h.nv);
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    ChainDev<T> d = chain_dev<T>(p, t, r.slot);
    if (!gravity)
        for (int i = 0; i < 6; i++) d.a_root[i] = T(0);
    void *scratch = nullptr;
    if (r.path == ROUTE_GEN1) {  // single-cluster programs: the fused, slab-free kernel (chain_kernels.hip, aba_gen1_kernel)
        gen1_only(d);
        d.sv_global = 0;
        d.out_lds = -1;
        d.lds_bytes = static_cast<int>(static_cast<size_t>(cp.n_lds) * kWave * sizeof(T));
        const size_t lds_total = gen1_lds_bytes<T>(h, cp);
        const size_t grid = gen1_grid(p, t.n_cu, n_tiles, gen1_waves_per_simd<T>(cp.gens[0].n), lds_total);
        hipError_t e = launch_aba_gen1<T>(d, cp.gens[0].n, cp.gens[0].kind != 0, q, qd, tau, ydd, B, static_cast<int>(grid), lds_total, hs);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "aba single-cluster launch");
    }
    if (r.path == ROUTE_LM) {  // (chain_kernels.hip, aba_chain_lm_kernel)
        if (cp.diffs.empty()) d.diffs = nullptr;  // (fp32 programs only: plan.cpp)
        no_gens(d);
        d.n_glb_slots = cp.n_glb + 1;  // (+ the row that carries the other wavefronts' bad-pivot masks to wavefront 0, aba_chain_lm_kernel)
        d.sv_global = 0;
        const size_t lds_lm = lm_lds_bytes<T>(h, cp);
        d.lds_bytes = static_cast<int>(lds_lm);
        const size_t grid = n_tiles;  // (<= 4 workgroups per CU: all resident)
        if (int rc = ensure_scratch(p, device, stream, scratch_bytes(grid, static_cast<size_t>(d.n_glb_slots) + in_rows, sizeof(T)), &scratch)) return rc;
        hipError_t e = launch_aba_chain_lm<T>(d, q, qd, tau, ydd, B, static_cast<T *>(scratch), static_cast<int>(grid), lds_lm, hs, r.lm_waves);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "aba chain launch (latency mode)");
    }
    const int kid = sizeof(T) == 8 ? 1 : 0;
    const size_t waves_per_cu = static_cast<size_t>((sizeof(T) == 8 && !cp.gens.empty()) ? p->opt.waves_per_cu_f64_wide_regs : p->opt.waves_per_cu[kid]);
    const LaunchShape s = launch_shape(t.n_cu, n_tiles, waves_per_cu, static_cast<size_t>(cp.n_lds) * kWave * sizeof(T), h.nq, h.nv, sizeof(T),
                                       static_cast<size_t>(p->opt.lds_bytes_per_wave[kid]), true);
    {   // the floating base's segments that only move data through the slab (devplan.h, ChainDev::fuse)
        int n_free_bwd = 0, at_bwd = -1;
        for (size_t i = 0; i < cp.segs.size(); i++)
            if (cp.segs[i].op == SEG_FREE_BWD) { n_free_bwd++; at_bwd = static_cast<int>(i); }
        if (!cp.segs.empty() && cp.segs[0].op == SEG_FREE_FWD && n_free_bwd == 1 && cp.frees[cp.segs[0].first].lds_v >= 0) {
            // (without room for all three inputs the prologue stages one array at a time: the velocities are gone when it returns)
            if (s.stage_all_fits) d.fuse |= 1;
            d.stage_lds_v = cp.frees[cp.segs[0].first].lds_v;
            d.stage_v_index = cp.frees[cp.segs[0].first].v_index;
        }
        if (n_free_bwd == 1 && at_bwd + 1 < static_cast<int>(cp.segs.size()) && cp.segs[at_bwd + 1].op == SEG_FREE_ACC &&
            cp.segs[at_bwd + 1].first == cp.segs[at_bwd].first)
            d.fuse |= 2;
    }
    d.lds_bytes = static_cast<int>(s.lds_bytes);
    // (the launch that keeps the inputs in registers -- launch_aba_chain reads the same rule)
    const bool inreg = !wrenches && chain_inputs_in_registers(sizeof(T), d.n_gens, d.n_diffs, d.sv_global, d.nq, d.nv);
    // (the slab: the rows the kernel's own rule gives a wavefront -- no input rows when they live in registers)
    const size_t slab_rows = static_cast<size_t>(chain_slab_rows(inreg, d.nq, d.nv, d.n_glb_slots, d.out_lds).total);
    if (int rc = ensure_scratch(p, device, stream, scratch_bytes(s.grid, slab_rows, sizeof(T)), &scratch)) return rc;
    hipError_t e = wrenches ? launch_aba_chain_wrench<T>(d, *wrenches, q, qd, tau, ydd, B, static_cast<T *>(scratch), static_cast<int>(s.grid), s.lds_bytes, hs)
                            : launch_aba_chain<T>(d, q, qd, tau, ydd, B, static_cast<T *>(scratch), static_cast<int>(s.grid), s.lds_bytes, hs);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "aba chain launch");
}

template <class T>
int run_rnea_chain(const grbda_plan *p, const DeviceTables &t, const Route &r, const T *q, const T *qd, const T *ydd, T *tau, size_t B, int device,
                   void *stream, bool gravity = true, const WrenchList<T> *wrenches = nullptr)  // wrenches: ROUTE_CHAIN only (wrench_route)
{
    const HostPlan &h = p->host;
    const RneaChainProgram &rp = h.rchain[r.slot];
    const size_t n_tiles = (B + kWave - 1) / kWave;
    const size_t in_rows = static_cast<size_t>(h.nq + 2 * h.nv);
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    RneaChainDev<T> d = rnea_chain_dev<T>(p, t, r.slot);
    if (!gravity)
        for (int i = 0; i < 6; i++) d.a_root[i] = T(0);
    void *scratch = nullptr;
    if (r.path == ROUTE_LM) {  // (chain_kernels.hip, rnea_chain_lm_kernel)
        if (rp.diffs.empty()) d.diffs = nullptr;  // (fp32 programs only)
        no_gens(d);
        d.n_glb_slots = 0;
        const size_t lds_bytes = lm_lds_bytes<T>(h, rp);
        d.lds_bytes = static_cast<int>(lds_bytes);
        const size_t grid = n_tiles;  // (all resident)
        if (int rc = ensure_scratch(p, device, stream, scratch_bytes(grid, in_rows, sizeof(T)), &scratch)) return rc;
        hipError_t e = launch_rnea_chain_lm<T>(d, q, qd, ydd, tau, B, static_cast<T *>(scratch), static_cast<int>(grid), lds_bytes, hs, r.lm_waves);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "rnea chain launch (latency mode)");
    }
    if (r.path == ROUTE_GEN1) {  // single-cluster programs: the fused, slab-free kernel (chain_kernels.hip, rnea_gen1_kernel)
        gen1_only(d);
        d.lds_bytes = static_cast<int>(static_cast<size_t>(rp.n_lds) * kWave * sizeof(T));
        const size_t lds_total = gen1_lds_bytes<T>(h, rp);
        const size_t grid = gen1_grid(p, t.n_cu, n_tiles, rnea_gen1_waves_per_simd<T>(rp.gens[0].n), lds_total);
        hipError_t e = launch_rnea_gen1<T>(d, rp.gens[0].n, rp.gens[0].kind != 0, q, qd, ydd, tau, B, static_cast<int>(grid), lds_total, hs);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "rnea single-cluster launch");
    }
    // (the four-wavefronts-per-SIMD program: 16 per CU; otherwise the ABA launch shape, 8 wavefronts per CU)
    const bool wide = r.slot == SLOT_F32_WIDE;
    const int kid = sizeof(T) == 8 ? 1 : 0;
    const LaunchShape s = launch_shape(t.n_cu, n_tiles, wide ? static_cast<size_t>(16) : static_cast<size_t>(p->opt.waves_per_cu[kid]),
                                       static_cast<size_t>(rp.n_lds) * kWave * sizeof(T), h.nq, h.nv, sizeof(T),
                                       static_cast<size_t>(wide ? p->opt.chain32w_lds_bytes : p->opt.lds_bytes_per_wave[kid]), true);
    d.lds_bytes = static_cast<int>(s.lds_bytes);
    if (int rc = ensure_scratch(p, device, stream, scratch_bytes(s.grid, in_rows + static_cast<size_t>(rp.n_glb), sizeof(T)), &scratch)) return rc;
    const std::vector<ChainFree> &bases = h.chain[r.slot].frees;
    hipError_t e = wrenches ? launch_rnea_chain_wrench<T>(d, *wrenches, bases.empty() ? -1 : bases[0].body, q, qd, ydd, tau, B, static_cast<T *>(scratch),
                                                          static_cast<int>(s.grid), s.lds_bytes, hs)
                            : launch_rnea_chain<T>(d, q, qd, ydd, tau, B, static_cast<T *>(scratch), static_cast<int>(s.grid), s.lds_bytes, hs);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "rnea chain launch");
}

template <class T>
int projection_run(const grbda_plan *p, bool rnea, const T *q, const T *qd, const T *x, const T *f_ext, T *out, size_t B, int device, void *stream);
int projection_run_f32_through_f64(const grbda_plan *p, bool rnea, const float *q, const float *qd, const float *x, const float *f_ext, float *out,
                                   size_t B, int device, void *stream);

// gravity = false: the same dynamics with a_root = 0, for callers that difference two runs and want no gravity in either (the unit-wrench
// route of the inverse OSIM).  The spanning-tree route keeps the plan's gravity: its sub-plan's launches are not reached from here.
template <class T>
int run(const grbda_plan *p, bool rnea, const T *q, const T *qd, const T *x, const T *f_ext, T *out, size_t B,
        int device, void *stream, bool gravity = true)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !qd || !x || !out) return set_err(GRBDA_EINVAL, "null argument");
    if (B == 0) return GRBDA_OK;
    if (p->host.projection_only) {
        // (external forces: world-frame wrenches on the BODIES, which the spanning model shares with this one -- they enter its inverse dynamics)
        if constexpr (sizeof(T) == 4) {
            // clusters beyond the structured limits: a dense solve over chains tens of links long loses cond(H) x 6e-8 in fp32 (measured
            // 1e-2 on the reference's depth-10 parallel chains); the route is slow anyway, so fp32 callers get the fp64 route's result
            if (p->host.big_clusters && !rnea) return projection_run_f32_through_f64(p, rnea, q, qd, x, f_ext, out, B, device, stream);
        }
        return projection_run<T>(p, rnea, q, qd, x, f_ext, out, B, device, stream);
    }
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    // chain-structured fast path (chain_kernels.hip) of models the chain programs cover
    const Route r = rnea ? choose_rnea<T>(p, t->n_cu, B, f_ext != nullptr) : choose_aba<T>(p, t->n_cu, B, f_ext != nullptr);
    if (r.path != ROUTE_INTERPRETER)
        return rnea ? run_rnea_chain<T>(p, *t, r, q, qd, x, out, B, device, stream, gravity)
                    : run_chain<T>(p, *t, r, q, qd, x, out, B, device, stream, gravity);
    DevPlan<T> d = make_dev_plan<T>(p, *t, rnea, f_ext != nullptr);
    d.fext = f_ext;
    if (!gravity)
        for (int i = 0; i < 6; i++) d.a_root[i] = T(0);
    const int kid = (rnea ? 2 : 0) + (sizeof(T) == 8 ? 1 : 0);
    const LaunchShape s = launch_shape(t->n_cu, (B + kWave - 1) / kWave, static_cast<size_t>(kid == 1 ? p->opt.waves_per_cu_f64_wide_regs : p->opt.waves_per_cu[kid]),
                                       static_cast<size_t>(d.n_lds_slots) * kWave * sizeof(T), d.nq, d.nv, sizeof(T),
                                       static_cast<size_t>(p->opt.lds_bytes_per_wave[kid]), true);
    d.lds_bytes = static_cast<int>(s.lds_bytes);
    // (sized by the grid before the LDS-fit clamp: inherited, not chosen)
    const size_t n_glb = static_cast<size_t>(d.n_glb_slots) + static_cast<size_t>(d.nq + 2 * d.nv);  // + staged inputs
    void *scratch = nullptr;
    if (int rc = ensure_scratch(p, device, stream, scratch_bytes(s.grid_unclamped, n_glb, sizeof(T)), &scratch)) return rc;
    hipError_t e;
    if (rnea)
        e = launch_rnea<T>(d, q, qd, x, out, B, static_cast<T *>(scratch), static_cast<int>(s.grid), s.lds_bytes,
                           static_cast<hipStream_t>(stream));
    else
        // (f64 only) the two-wavefronts-per-SIMD build pays for its spills only when the grid fills them
        e = launch_aba<T>(d, q, qd, x, out, B, static_cast<T *>(scratch), static_cast<int>(s.grid), s.lds_bytes,
                          static_cast<hipStream_t>(stream), s.grid > static_cast<size_t>(t->n_cu) * 4);
    if (e != hipSuccess) return hip_err(e, rnea ? "rnea launch" : "aba launch");
    return GRBDA_OK;
}

// ---- host arrays: the staging of the *_host_f64 entry points (single-state facade calls) -----------------------------------------
// in() / out() / inout() allocate a device array each, as they are called; run() then copies the inputs in, makes the call (which
// enqueues on the null stream), waits for the device and copies the outputs back, all in the order of declaration.  The arrays are
// freed when the stage goes out of scope, whatever failed.
class HostStage {
    struct Array {
        void *dev;
        const void *src;  // host array copied in before the call (null: none)
        void *dst;        // host array the result is copied to (null: none)
        size_t bytes;
    };
    std::vector<Array> arrays_;
    int rc_ = GRBDA_OK;
    template <class T>
    T *add(const T *src, T *dst, size_t count)
    {
        Array a{nullptr, src, dst, count * sizeof(T)};
        hipError_t e;
        if (rc_ == GRBDA_OK && (e = hipMalloc(&a.dev, a.bytes ? a.bytes : 16)) != hipSuccess) rc_ = hip_err(e, "hipMalloc");
        arrays_.push_back(a);
        return static_cast<T *>(a.dev);
    }

public:
    HostStage() = default;
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    ~HostStage()
    {
        for (const Array &a : arrays_)
            if (a.dev) (void)hipFree(a.dev);
    }
    template <class T>
    const T *in(const T *src, size_t count) { return add<T>(src, nullptr, count); }
    template <class T>
    T *out(T *dst, size_t count) { return add<T>(nullptr, dst, count); }  // (dst null: a device array nobody reads back)
    template <class T>
    T *inout(T *io, size_t count) { return add<T>(io, io, count); }
    template <class Call>
    int run(Call call)
    {
        if (rc_) return rc_;
        hipError_t e;
        for (const Array &a : arrays_)
            if (a.src && (e = hipMemcpy(a.dev, a.src, a.bytes, hipMemcpyHostToDevice)) != hipSuccess) return hip_err(e, "hipMemcpy H2D");
        if (int rc = call()) return rc;
        if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_err(e, "kernel execution");
        for (const Array &a : arrays_)
            if (a.dst && (e = hipMemcpy(a.dst, a.dev, a.bytes, hipMemcpyDeviceToHost)) != hipSuccess) return hip_err(e, "hipMemcpy D2H");
        return GRBDA_OK;
    }
};

int run_host_f64(const grbda_plan *p, bool rnea, const double *q, const double *qd, const double *x,
                 const double *f_ext, double *out, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !qd || !x || !out) return set_err(GRBDA_EINVAL, "null argument");
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, nfe = static_cast<size_t>(p->host.n_bodies) * 6;
    HostStage st;
    const double *dfe = f_ext ? st.in(f_ext, B * nfe) : nullptr;
    const double *dq = st.in(q, B * nq), *dqd = st.in(qd, B * nv), *dx = st.in(x, B * nv);
    double *dout = st.out(out, B * nv);
    return st.run([&] { return run<double>(p, rnea, dq, dqd, dx, dfe, dout, B, device, nullptr); });
}

// ---- steps either side of the path: Newton projection, spanning recovery (kernels.hip) -----------------------
int span_count(const grbda_plan *p)
{
    int n = 0;
    for (const ClusterRec &c : p->host.lay64.clusters) n += c.kind == CK_FREE ? 6 : c.k;
    return n;
}

// Launch shape and scratch slab of an auxiliary kernel -- one that works on a slot layout of the forward dynamics of the same precision:
// waves_per_cu one-wavefront workgroups per CU over the tiles of B states, `store_bytes` of slot store each, and a slab of `slab_rows` rows
// besides the nq + 2 nv staged input rows.  The slab is sized by the grid before the LDS-fit clamp, where that is asked for (inherited).
template <class T>
int aux_launch(const grbda_plan *p, const DeviceTables &t, size_t B, size_t waves_per_cu, size_t store_bytes, bool clamp_to_lds_fit, size_t slab_rows,
               int device, void *stream, LaunchShape &s, T *&scratch)
{
    const HostPlan &h = p->host;
    s = launch_shape(t.n_cu, (B + kWave - 1) / kWave, waves_per_cu, store_bytes, h.nq, h.nv, sizeof(T),
                     static_cast<size_t>(p->opt.lds_bytes_per_wave[sizeof(T) == 8 ? 1 : 0]), clamp_to_lds_fit);
    void *sp = nullptr;
    if (int rc = ensure_scratch(p, device, stream, scratch_bytes(s.grid_unclamped, slab_rows + static_cast<size_t>(h.nq + 2 * h.nv), sizeof(T)), &sp)) return rc;
    scratch = static_cast<T *>(sp);
    return GRBDA_OK;
}
// the auxiliary kernels of kernels.hip: the ABA's own slot layout, one wavefront per SIMD (they are not register-tuned), no LDS-fit clamp
// (inherited, not chosen)
template <class T>
int aux_setup(const grbda_plan *p, size_t B, int device, void *stream, DevPlan<T> &d, T **scratch, int *grid,
              size_t *lds_bytes)
{
    // (the auxiliary kernels walk the cluster tables with per-lane arrays sized by kMaxClusterBodies / kMaxClusterDof)
    if (p->host.big_clusters)
        return set_err(GRBDA_EUNSUPPORTED, "only forward / inverse dynamics and the mass matrix are covered for clusters beyond the structured kernels' limits");
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    d = make_dev_plan<T>(p, *t, false, false);
    LaunchShape s;
    if (int rc = aux_launch<T>(p, *t, B, 4, static_cast<size_t>(d.n_lds_slots) * kWave * sizeof(T), false, d.n_glb_slots, device, stream, s, *scratch)) return rc;
    d.lds_bytes = static_cast<int>(s.lds_bytes);
    *grid = static_cast<int>(s.grid);
    *lds_bytes = s.lds_bytes;
    return GRBDA_OK;
}

template <class T>
int project(const grbda_plan *p, T *q, int32_t *ok, size_t B, int max_iter, double tol, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || max_iter < 0) return set_err(GRBDA_EINVAL, "bad argument");
    if (B == 0) return GRBDA_OK;
    if (p->host.big_clusters) {  // (clusters beyond the structured limits: the wide Newton kernel of manifold_kernels.hip)
        DeviceTables *t = nullptr;
        if (int rc = ensure_device(p, device, &t)) return rc;
        DevPlan<T> dp = make_dev_plan<T>(p, *t, false, false);
        const size_t g = tile_grid(t->n_cu, 4, B);
        hipError_t e = launch_manifold_newton<T>(dp, p->host.n_clusters, q, ok, B, max_iter, static_cast<T>(tol), static_cast<int>(g),
                                                 static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "projection launch");
    }
    DevPlan<T> d;
    T *scratch = nullptr;
    int grid = 0;
    size_t lds = 0;
    if (int rc = aux_setup<T>(p, B, device, stream, d, &scratch, &grid, &lds)) return rc;
    hipError_t e = launch_project<T>(d, p->host.n_clusters, q, ok, B, max_iter, static_cast<T>(tol), scratch, grid, lds,
                                     static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "projection launch");
}

template <class T>
int spanning(const grbda_plan *p, const T *q, const T *qd, const T *ydd, T *qd_span, T *qdd_span, size_t B, int device,
             void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !qd || !ydd || !qdd_span) return set_err(GRBDA_EINVAL, "null argument");
    if (B == 0) return GRBDA_OK;
    if (p->host.big_clusters) {
        // clusters beyond the structured limits: qd_s = G yd, qdd_s = G ydd + g from the wide constraint kernel of the spanning-tree route
        // (manifold_kernels.hip), whose spanning coordinates are the bodies in order -- the layout of this entry point
        if (!p->span) return set_err(GRBDA_EUNSUPPORTED, "the model needs the spanning-tree route, which covers at most 128 velocities");
        DeviceTables *t = nullptr;
        if (int rc = ensure_device(p, device, &t)) return rc;
        const size_t nq = p->host.nq, nv = p->host.nv, nq_s = p->span->host.nq, nv_s = p->span->host.nv;
        if (static_cast<size_t>(span_count(p)) != nv_s) return set_err(GRBDA_EUNSUPPORTED, "spanning layout mismatch");
        const size_t per_state = nq_s + nv_s + static_cast<size_t>(p->n_cpl_rows);
        const Chunk c = budgeted_chunk(p, p->work_proj, device, stream, 1024ull << 20, per_state * sizeof(T), B);
        void *wptr = nullptr;
        if (int rc = ensure_work(p, p->work_proj, device, stream, c.bytes, &wptr)) return rc;
        Carver<T> w(wptr, c.chunk * per_state);
        T *q_s = w.take(c.chunk * nq_s), *v_tmp = w.take(c.chunk * nv_s), *cpl = w.take(c.chunk * p->n_cpl_rows);
        assert(w.taken == w.cap);
        DevPlan<T> dp = make_dev_plan<T>(p, *t, false, false);
        for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
            const size_t g = tile_grid(t->n_cu, 4, nb);
            hipError_t e = launch_manifold_constraint<T>(dp, p->host.n_clusters, t->span_q, t->span_v, t->crow, static_cast<int>(nq_s),
                                                         static_cast<int>(nv_s), p->n_cpl_rows, 0, q + b0 * nq, qd + b0 * nv, ydd + b0 * nv, q_s,
                                                         qd_span ? qd_span + b0 * nv_s : v_tmp, qdd_span + b0 * nv_s, cpl, nb, static_cast<int>(g),
                                                         static_cast<hipStream_t>(stream), 1, p->has_trig);
            if (e != hipSuccess) return hip_err(e, "manifold constraint launch");
        }
        return GRBDA_OK;
    }
    DevPlan<T> d;
    T *scratch = nullptr;
    int grid = 0;
    size_t lds = 0;
    if (int rc = aux_setup<T>(p, B, device, stream, d, &scratch, &grid, &lds)) return rc;
    hipError_t e = launch_spanning<T>(d, p->host.n_clusters, span_count(p), q, qd, ydd, qd_span, qdd_span, B, scratch,
                                      grid, lds, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "spanning launch");
}

// ---- time stepping (kernels.hip, integrate_kernel; include/grbda_hip.h "Time stepping") ----------------------------------------------
bool ranges_overlap(const void *a, size_t n, const void *b, size_t m);

bool has_loop_clusters(const grbda_plan *p)
{
    for (const ClusterRec &c : p->host.lay64.clusters)
        if (c.kind == CK_LOOP) return true;
    return false;
}
// Everything grbda_integrate_* refuses, on the host and before any device call: the argument rules (device and host arrays alike), then
// the two kinds of plan the integrator does not cover.  Outputs may BE their inputs (q_next == q, qd_next == qd); any other overlap of an
// output with an input or with the other output is refused.
template <class T>
int integrate_args(const grbda_plan *p, const T *q, const T *qd, const T *ydd, double dt, const T *q_next, const T *qd_next, int max_iter,
                   double tol, size_t B)
{
    if (!q || !qd || !ydd || !q_next || !qd_next) return set_err(GRBDA_EINVAL, "null argument");
    if (!std::isfinite(dt)) return set_err(GRBDA_EINVAL, "dt is not finite");
    if (max_iter < 0 || std::isnan(tol)) return set_err(GRBDA_EINVAL, "bad projection arguments");
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const void *in[3] = {q, qd, ydd}, *out[2] = {q_next, qd_next};
    const size_t in_bytes[3] = {bq, bv, bv}, out_bytes[2] = {bq, bv};
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++)
            if (!(i == j && out[i] == in[j]) && ranges_overlap(out[i], out_bytes[i], in[j], in_bytes[j]))
                return set_err(GRBDA_EINVAL, "an output array overlaps an input array (only q_next == q and qd_next == qd are allowed)");
    if (ranges_overlap(q_next, bq, qd_next, bv)) return set_err(GRBDA_EINVAL, "q_next and qd_next overlap");
    for (const ClusterRec &c : p->host.lay64.clusters)
        if (c.kind == CK_FREE && p->host.ori_repr != 0)
            return set_err(GRBDA_EUNSUPPORTED, "time stepping covers the quaternion floating base only: the rate map of a roll-pitch-yaw base is not built");
    if (p->host.projection_only && has_loop_clusters(p))
        return set_err(GRBDA_EUNSUPPORTED, "time stepping does not cover implicit clusters of plans on the spanning-tree route (their G is evaluated by the "
                                           "spanning-tree kernels only)");
    return GRBDA_OK;
}

// the launch itself (arguments checked, B > 0)
template <class T>
int integrate_launch(const grbda_plan *p, const T *q, const T *qd, const T *ydd, double dt, T *q_next, T *qd_next, int32_t *ok, int max_iter,
                     double tol, size_t B, int device, void *stream, bool ok_and = false)
{
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    DevPlan<T> d = make_dev_plan<T>(p, *t, false, false);
    // The slot layout of the ABA of the same precision, like the other auxiliary kernels -- but only implicit clusters use slots, so an
    // explicit plan asks for the staging area alone, and in fp32 (two wavefronts per SIMD by registers) runs eight wavefronts per CU.
    const bool loops = has_loop_clusters(p);
    const size_t store = loops ? static_cast<size_t>(d.n_lds_slots) * kWave * sizeof(T) : 0;
    LaunchShape s;
    T *scratch = nullptr;
    if (int rc = aux_launch<T>(p, *t, B, loops || sizeof(T) == 8 ? 4 : 8, store, true, static_cast<size_t>(d.n_glb_slots) + kIntegrateLocalRows, device, stream, s,
                               scratch))
        return rc;
    d.lds_bytes = static_cast<int>(s.lds_bytes);
    hipError_t e = launch_integrate<T>(d, p->host.n_clusters, q, qd, ydd, static_cast<T>(dt), q_next, qd_next, ok, ok_and ? 1 : 0, B, max_iter, static_cast<T>(tol),
                                       scratch, static_cast<int>(s.grid), s.lds_bytes, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "integrate launch");
}

template <class T>
int integrate(const grbda_plan *p, const T *q, const T *qd, const T *ydd, double dt, T *q_next, T *qd_next, int32_t *ok, int max_iter, double tol,
              size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = integrate_args<T>(p, q, qd, ydd, dt, q_next, qd_next, max_iter, tol, B)) return rc;
    if (B == 0) return GRBDA_OK;
    return integrate_launch<T>(p, q, qd, ydd, dt, q_next, qd_next, ok, max_iter, tol, B, device, stream);
}

// what grbda_step_* passes to the projection: the reference's nearZero, and the iteration count the Python layer passes to
// grbda_project_positions_*
constexpr int kStepMaxIter = 50;
constexpr double kStepTol = 1e-8;

// the argument rules of grbda_step_* beyond the integrator's: ydd is written by the forward dynamics and read by the integrator
template <class T>
int step_args(const grbda_plan *p, const T *q, const T *qd, const T *tau, const T *f_ext, double dt, const T *ydd, const T *q_next, const T *qd_next,
              size_t B)
{
    if (!tau || !ydd) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = integrate_args<T>(p, q, qd, ydd, dt, q_next, qd_next, kStepMaxIter, kStepTol, B)) return rc;
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const size_t bf = B * static_cast<size_t>(p->host.n_bodies) * 6 * sizeof(T);
    if (ranges_overlap(ydd, bv, q, bq) || ranges_overlap(ydd, bv, qd, bv) || ranges_overlap(ydd, bv, tau, bv) || ranges_overlap(ydd, bv, f_ext, bf))
        return set_err(GRBDA_EINVAL, "ydd overlaps an input array");
    if (ranges_overlap(q_next, bq, tau, bv) || ranges_overlap(qd_next, bv, tau, bv) || ranges_overlap(q_next, bq, f_ext, bf) ||
        ranges_overlap(qd_next, bv, f_ext, bf))
        return set_err(GRBDA_EINVAL, "an output array overlaps tau or f_ext");
    return GRBDA_OK;
}

// grbda_aba_* followed by grbda_integrate_* on the same stream
template <class T>
int step(const grbda_plan *p, const T *q, const T *qd, const T *tau, const T *f_ext, double dt, T *ydd, T *q_next, T *qd_next, int32_t *ok, size_t B,
         int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = step_args<T>(p, q, qd, tau, f_ext, dt, ydd, q_next, qd_next, B)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;  // (GRBDA_ENODEVICE whatever route the forward dynamics take)
    if (int rc = run<T>(p, false, q, qd, tau, f_ext, ydd, B, device, stream)) return rc;
    return integrate_launch<T>(p, q, qd, ydd, dt, q_next, qd_next, ok, kStepMaxIter, kStepTol, B, device, stream);
}

// T steps in place; every state copied to the trajectory arrays device-to-device on the same stream
template <class T>
int rollout(const grbda_plan *p, T *q, T *qd, const T *tau, int tau_steps, double dt, int n_steps, T *ydd_work, T *q_traj, T *qd_traj, int32_t *ok,
            size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (n_steps < 0) return set_err(GRBDA_EINVAL, "T is negative");
    if (tau_steps != 1 && tau_steps != n_steps) return set_err(GRBDA_EINVAL, "tau_steps must be 1 or T");
    if (int rc = step_args<T>(p, q, qd, tau, static_cast<const T *>(nullptr), dt, ydd_work, q, qd, B)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, bq = B * nq * sizeof(T), bv = B * nv * sizeof(T);
    const size_t steps = static_cast<size_t>(n_steps);
    // (tau[T][B][nv]: every step's block, not only the first, stays clear of what the steps write)
    if (tau_steps > 1 && (ranges_overlap(tau, steps * bv, q, bq) || ranges_overlap(tau, steps * bv, qd, bv) || ranges_overlap(tau, steps * bv, ydd_work, bv)))
        return set_err(GRBDA_EINVAL, "tau overlaps an array the steps write");
    const void *state[4] = {q, qd, tau, ydd_work};
    const size_t state_bytes[4] = {bq, bv, (tau_steps > 1 ? steps : 1) * bv, bv};
    for (int j = 0; j < 4; j++)
        if (ranges_overlap(q_traj, steps * bq, state[j], state_bytes[j]) || ranges_overlap(qd_traj, steps * bv, state[j], state_bytes[j]))
            return set_err(GRBDA_EINVAL, "a trajectory array overlaps a state array");
    if (ranges_overlap(q_traj, steps * bq, qd_traj, steps * bv)) return set_err(GRBDA_EINVAL, "the trajectory arrays overlap");
    if (B == 0 || n_steps == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    for (int k = 0; k < n_steps; k++) {
        const T *tk = tau + (tau_steps > 1 ? static_cast<size_t>(k) * B * nv : 0);
        if (int rc = run<T>(p, false, q, qd, tk, static_cast<const T *>(nullptr), ydd_work, B, device, stream)) return rc;
        // (ok: the first step writes the flags, the later ones AND theirs into them)
        if (int rc = integrate_launch<T>(p, q, qd, ydd_work, dt, q, qd, ok, kStepMaxIter, kStepTol, B, device, stream, k > 0)) return rc;
        hipError_t e;
        if (q_traj && (e = hipMemcpyAsync(q_traj + static_cast<size_t>(k) * B * nq, q, bq, hipMemcpyDeviceToDevice, hs)) != hipSuccess)
            return hip_err(e, "hipMemcpyAsync");
        if (qd_traj && (e = hipMemcpyAsync(qd_traj + static_cast<size_t>(k) * B * nv, qd, bv, hipMemcpyDeviceToDevice, hs)) != hipSuccess)
            return hip_err(e, "hipMemcpyAsync");
    }
    return GRBDA_OK;
}

// ---- state input in the reference's conventions (kernels.hip, state_kernel) ----------------------------------
// widths of the caller's rows for the given per-cluster flags; GRBDA_ESTATE for independent positions of an implicit cluster
int state_widths(const grbda_plan *p, const uint8_t *pos_sp, const uint8_t *vel_sp, StateFlags *F, int *in_nq, int *in_nv)
{
    const auto &cl = p->host.lay64.clusters;
    if (cl.size() > static_cast<size_t>(64 * kStateFlagWords)) return set_err(GRBDA_EUNSUPPORTED, "more than 256 clusters");
    StateFlags f{};
    int wq = 0, wv = 0;
    const int npos_free = p->host.ori_repr == GRBDA_ORI_QUATERNION ? 7 : 6;
    for (size_t c = 0; c < cl.size(); c++) {
        const ClusterRec &r = cl[c];
        const bool ps = pos_sp ? pos_sp[c] != 0 : r.kind == CK_LOOP, vs = vel_sp ? vel_sp[c] != 0 : false;
        if (r.kind == CK_LOOP && !ps)
            return set_err(GRBDA_ESTATE, "cluster " + std::to_string(c) +
                                             ": Independent positions cannot be converted to spanning positions when the constraint is implicit.");
        if (ps) f.pos[c >> 6] |= 1ull << (c & 63);
        if (vs) f.vel[c >> 6] |= 1ull << (c & 63);
        wq += r.kind == CK_FREE ? npos_free : (ps ? r.k : r.n);
        wv += r.kind == CK_FREE ? 6 : (vs ? r.k : r.n);
    }
    if (F) *F = f;
    if (in_nq) *in_nq = wq;
    if (in_nv) *in_nv = wv;
    return GRBDA_OK;
}

template <class T>
int state_convert(const grbda_plan *p, const uint8_t *pos_sp, const uint8_t *vel_sp, const T *q_in, const T *qd_in, T *q, T *qd,
                  int32_t *status, T *cond, size_t B, double tol, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q_in || (qd && !qd_in)) return set_err(GRBDA_EINVAL, "null argument");
    StateFlags F;
    int in_nq = 0, in_nv = 0;
    if (int rc = state_widths(p, pos_sp, vel_sp, &F, &in_nq, &in_nv)) return rc;
    if (B == 0) return GRBDA_OK;
    if (p->host.big_clusters) {  // (clusters beyond the structured limits: the same rules in manifold_kernels.hip's wide state kernel)
        DeviceTables *t = nullptr;
        if (int rc = ensure_device(p, device, &t)) return rc;
        DevPlan<T> dp = make_dev_plan<T>(p, *t, false, false);
        const size_t g = tile_grid(t->n_cu, 4, B);
        hipError_t e = launch_manifold_state<T>(dp, p->host.n_clusters, F, q_in, qd_in, in_nq, in_nv, q, qd, status, cond, B, static_cast<T>(tol),
                                                static_cast<int>(g), static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "state conversion launch");
    }
    DevPlan<T> d;
    T *scratch = nullptr;
    int grid = 0;
    size_t lds = 0;
    if (int rc = aux_setup<T>(p, B, device, stream, d, &scratch, &grid, &lds)) return rc;
    hipError_t e = launch_state<T>(d, p->host.n_clusters, F, q_in, qd_in, in_nq, in_nv, q, qd, status, cond, B, static_cast<T>(tol),
                                   scratch, grid, lds, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "state conversion launch");
}

// ---- contact side: body poses, test force (include/grbda_hip.h) ---------------------------------------------
// ("1..8": kMaxContacts, devplan.h; `noun`: what the entry point calls its contacts)
int contact_count(int n_contacts, const char *noun)
{
    if (n_contacts < 1 || n_contacts > kMaxContacts) return set_err(GRBDA_EINVAL, std::string("1..8 contact ") + noun + " per call");
    return GRBDA_OK;
}
// the contact description of an entry point, checked on the host: the arrays, the count, then every body index
template <class T>
int contact_set(const grbda_plan *p, int n_contacts, const int *bodies, const double *offsets, const char *noun, ContactSet<T> &cs)
{
    if (!bodies || !offsets) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = contact_count(n_contacts, noun)) return rc;
    cs.n = n_contacts;
    for (int c = 0; c < n_contacts; c++) {
        if (bodies[c] < 0 || bodies[c] >= p->host.n_bodies) return set_err(GRBDA_EINVAL, "body index out of range");
        cs.body[c] = bodies[c];
        for (int i = 0; i < 3; i++) cs.off[c][i] = static_cast<T>(offsets[3 * c + i]);
    }
    return GRBDA_OK;
}
// no output array may share a byte with an input array or with another output (null entries are skipped)
template <class In, class Out, size_t NI, size_t NO>
int no_overlap(In (&in)[NI], const size_t (&in_bytes)[NI], Out (&out)[NO], const size_t (&out_bytes)[NO])
{
    for (size_t i = 0; i < NO; i++) {
        for (size_t j = 0; j < NI; j++)
            if (ranges_overlap(out[i], out_bytes[i], in[j], in_bytes[j])) return set_err(GRBDA_EINVAL, "an output array overlaps an input array");
        for (size_t j = i + 1; j < NO; j++)
            if (ranges_overlap(out[i], out_bytes[i], out[j], out_bytes[j])) return set_err(GRBDA_EINVAL, "two output arrays overlap");
    }
    return GRBDA_OK;
}
template <class T>
std::array<T, 3> gravity3(const grbda_plan *p)  // the plan's gravity, linear part (world axes)
{
    return {static_cast<T>(p->host.gravity[3]), static_cast<T>(p->host.gravity[4]), static_cast<T>(p->host.gravity[5])};
}

// The stages of the kinematics (arguments checked, nb > 0, device found): poses_kernel; the spanning rates into the caller's work arrays
// vs, as [nb][span_count], then twists_kernel.
template <class T>
int poses_stage(const grbda_plan *p, const DeviceTables &t, const T *q, T *Xa, size_t nb, void *stream)
{
    const DevPlan<T> d = make_dev_plan<T>(p, t, false, false);
    hipError_t e = launch_poses<T>(d, p->host.n_clusters, q, Xa, nb, static_cast<int>(tile_grid(t.n_cu, 8, nb)), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "poses launch");
}
template <class T>
int twists_stage(const grbda_plan *p, const DeviceTables &t, const T *q, const T *qd, const T *ydd, T *V, T *vs, T *as, size_t nb, int device,
                 void *stream, bool gravity = true)
{
    if (int rc = spanning<T>(p, q, qd, ydd, vs, as, nb, device, stream)) return rc;
    DevPlan<T> d = make_dev_plan<T>(p, t, false, false);
    if (!gravity)  // (the frame drift: the root's acceleration is zero)
        for (T &x : d.a_root) x = 0;
    hipError_t e = launch_twists<T>(d, p->host.n_clusters, span_count(p), q, vs, as, V, nb, static_cast<int>(tile_grid(t.n_cu, 8, nb)),
                                    static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "twists launch");
}

template <class T>
int poses(const grbda_plan *p, const T *q, T *Xa, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !Xa) return set_err(GRBDA_EINVAL, "null argument");
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    return poses_stage<T>(p, *t, q, Xa, B, stream);
}

// spatial velocity / acceleration of every body: the spanning rates (spanning_kernel) into the plan's per-(device, stream)
// workspace, then the tree walk (twists_kernel)
template <class T>
int twists(const grbda_plan *p, const T *q, const T *qd, const T *ydd, T *V, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !qd || !ydd || !V) return set_err(GRBDA_EINVAL, "null argument");
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t ns = static_cast<size_t>(span_count(p));
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, 2 * B * ns * sizeof(T) + 256, &wptr)) return rc;
    Carver<T> w(wptr, 2 * B * ns);
    T *vs = w.take(B * ns), *as = w.take(B * ns);
    return twists_stage<T>(p, *t, q, qd, ydd, V, vs, as, B, device, stream);
}

// ---- poses and twists of a listed few bodies (include/grbda_hip_bodies.h; body_list_kernels.hip) ----------------------------------------
// (the walk of a body list, BodyWalkHost and build_body_walk: walk.h)
template <class T>
BodyWalk<T> device_body_walk(const grbda_plan *p, const DeviceTables &t, const BodyWalkHost &H)
{
    BodyWalk<T> W{};
    W.n_steps = H.walk_len;
    W.n_list = H.n;
    W.n_saved = H.max_saved;
    W.nq = p->host.nq;
    W.n_span = span_count(p);
    W.ori_repr = p->host.ori_repr;
    W.consts = consts_of<T>(t);
    for (int i = 0; i < 6; i++) W.a_root[i] = static_cast<T>(-p->host.gravity[i]);
    std::memcpy(W.slot, H.slot, sizeof(W.slot));
    std::memcpy(W.step, H.step, sizeof(W.step));
    return W;
}
// What every entry point that takes a body list refuses of the list (wrench_args and contact_set: their own caps and messages).
// with_list: the one other array that a list of n > 0 needs (the listed output), or `bodies` again
int body_list_check(const grbda_plan *p, int n, const int *bodies, const void *with_list)
{
    if (n < 0 || n > kMaxBodyList) return set_err(GRBDA_EINVAL, "0..16 bodies per call");
    if (n > 0 && (!bodies || !with_list)) return set_err(GRBDA_EINVAL, "null argument");
    for (int i = 0; i < n; i++)
        if (bodies[i] < 0 || bodies[i] >= p->host.n_bodies) return set_err(GRBDA_EINVAL, "body index out of range");
    return GRBDA_OK;
}
// Everything the list entry points refuse, on the host and before any device call.  qd == nullptr && ydd == nullptr: the poses.
template <class T>
int body_list_args(const grbda_plan *p, bool twists, const T *q, const T *qd, const T *ydd, int n, const int *bodies, const T *out, size_t B)
{
    if (!q || (twists && (!qd || !ydd))) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = body_list_check(p, n, bodies, out)) return rc;
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const void *const in[3] = {q, twists ? qd : nullptr, twists ? ydd : nullptr}, *const outs[1] = {n > 0 ? out : nullptr};
    const size_t in_bytes[3] = {bq, bv, bv}, out_bytes[1] = {B * static_cast<size_t>(n) * 12 * sizeof(T)};
    return no_overlap(in, in_bytes, outs, out_bytes);
}
// One pass over nb states (arguments checked, nb > 0, n > 0, device found): the walk kernel, or -- route 1 -- the full kernel into `full`
// [nb][n_bodies][12] and the gather.  Twists: the spanning rates into vs, as [nb][span_count] first, as twists_stage.
template <class T>
int body_list_stage(const grbda_plan *p, const DeviceTables &t, const BodyWalkHost &H, bool twists, const T *q, const T *qd, const T *ydd, T *out,
                    T *full, T *vs, T *as, size_t nb, int device, void *stream, bool gravity = true)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (H.route == 1) {
        if (int rc = twists ? twists_stage<T>(p, t, q, qd, ydd, full, vs, as, nb, device, stream, gravity) : poses_stage<T>(p, t, q, full, nb, stream))
            return rc;
        hipError_t e = launch_body_gather<T>(H.list, full, p->host.n_bodies, nb, out, hs);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "body gather launch");
    }
    BodyWalk<T> W = device_body_walk<T>(p, t, H);
    if (!gravity)
        for (T &x : W.a_root) x = 0;
    // eight one-wavefront workgroups per CU as the full kernels, fewer where the saved values' LDS holds fewer
    const size_t per_cu = std::min<size_t>(8, lds_workgroups_per_cu(static_cast<size_t>(H.max_saved) * 12 * kWave * sizeof(T)));
    const int grid = static_cast<int>(tile_grid(t.n_cu, per_cu, nb));
    hipError_t e;
    if (twists) {
        if (int rc = spanning<T>(p, q, qd, ydd, vs, as, nb, device, stream)) return rc;
        e = launch_body_twists_list<T>(W, q, vs, as, out, nb, grid, hs);
    } else {
        e = launch_body_poses_list<T>(W, q, out, nb, grid, hs);
    }
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "body list launch");
}
// The work memory of one body_list_stage call, in elements per state: the listed output (n x 12; n = 0: the stage writes the caller's
// array), the full rows of route 1, each of the two spanning rates of the twists.  ONE definition of what a call site counts into its
// chunk and of what it takes from the slab, in that order.
struct ListWork {
    size_t out = 0, full = 0, span = 0;
    size_t per_state() const { return out + full + 2 * span; }
    template <class T>
    struct Arrays {
        T *out, *full, *vs, *as;
    };
    template <class T>
    Arrays<T> take(Carver<T> &w, size_t nb) const
    {
        Arrays<T> a{};
        a.out = out ? w.take(nb * out) : nullptr;
        a.full = full ? w.take(nb * full) : nullptr;
        a.vs = span ? w.take(nb * span) : nullptr;
        a.as = span ? w.take(nb * span) : nullptr;
        return a;
    }
};
ListWork list_work(const grbda_plan *p, const BodyWalkHost &H, bool twists, int n)
{
    return {static_cast<size_t>(n) * 12, H.route == 1 ? static_cast<size_t>(p->host.n_bodies) * 12 : 0,
            twists ? static_cast<size_t>(span_count(p)) : 0};
}
template <class T>
int body_list_run(const grbda_plan *p, bool twists, const T *q, const T *qd, const T *ydd, int n, const int *bodies, T *out, size_t B, int device,
                  void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = body_list_args<T>(p, twists, q, qd, ydd, n, bodies, out, B)) return rc;
    if (n == 0 || B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const BodyWalkHost H = build_body_walk(p->host, layout_of(p->host, sizeof(T) == 4 ? 0 : 1), n, bodies);
    const ListWork lw = list_work(p, H, twists, 0);  // (the output is the caller's)
    const size_t per_state = lw.per_state();
    if (per_state == 0) return body_list_stage<T>(p, *t, H, false, q, nullptr, nullptr, out, nullptr, nullptr, nullptr, B, device, stream);
    const size_t nq = p->host.nq, nv = p->host.nv, n12 = static_cast<size_t>(n) * 12;
    const Chunk c = budgeted_chunk(p, p->work, device, stream, 1024ull << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        const auto m = lw.take(w, nb);
        if (int rc = body_list_stage<T>(p, *t, H, twists, q + b0 * nq, twists ? qd + b0 * nv : nullptr, twists ? ydd + b0 * nv : nullptr, out + b0 * n12,
                                        m.full, m.vs, m.as, nb, device, stream))
            return rc;
    }
    return GRBDA_OK;
}
int body_list_host_f64(const grbda_plan *p, bool twists, const double *q, const double *qd, const double *ydd, int n, const int *bodies, double *out,
                       size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = body_list_args<double>(p, twists, q, qd, ydd, n, bodies, out, B)) return rc;
    if (n == 0 || B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = twists ? st.in(qd, B * nv) : nullptr, *dy = twists ? st.in(ydd, B * nv) : nullptr;
    double *dout = st.out(out, B * static_cast<size_t>(n) * 12);
    return st.run([&] { return body_list_run<double>(p, twists, dq, dqd, dy, n, bodies, dout, B, device, nullptr); });
}

// ---- energy, centre of mass, centroidal momentum (centroidal_kernels.hip; include/grbda_hip.h) -----------------------------------
// sum of the body masses: entry (3, 3) of the 21 packed inertia constants behind BodyRec::cofs + 12 (devmath.h, sidx(3, 3) = 15)
double plan_total_mass(const grbda_plan *p)
{
    double m = 0;
    for (const BodyRec &b : p->host.lay64.bodies) m += p->host.consts[static_cast<size_t>(b.cofs) + 12 + 15];
    return m;
}
// what the outputs of a call need: the velocities (kinetic, com_vel, h) and the accelerations (hdot)
template <class T>
bool centroidal_velocities(const CentroidalOut<T> &o) { return o.kinetic || o.com_vel || o.h || o.hdot; }
// Everything the entry points refuse, on the host and before any device call.  `sizes`: elements per state of the six outputs.
template <class T>
int centroidal_args(const grbda_plan *p, const T *q, const T *qd, const T *ydd, const CentroidalOut<T> &o, size_t B)
{
    if (!q) return set_err(GRBDA_EINVAL, "null argument");
    if (!o.kinetic && !o.potential && !o.com && !o.com_vel && !o.h && !o.hdot) return set_err(GRBDA_EINVAL, "no output asked for");
    if (centroidal_velocities(o) && !qd) return set_err(GRBDA_EINVAL, "kinetic, com_vel, h and hdot need qd");
    if (o.hdot && !ydd) return set_err(GRBDA_EINVAL, "hdot needs ydd");
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T), b1 = B * sizeof(T);
    const void *const in[3] = {q, qd, ydd}, *const out[6] = {o.kinetic, o.potential, o.com, o.com_vel, o.h, o.hdot};
    const size_t in_bytes[3] = {bq, bv, bv}, out_bytes[6] = {b1, b1, 3 * b1, 3 * b1, 6 * b1, 6 * b1};
    if (int rc = no_overlap(in, in_bytes, out, out_bytes)) return rc;
    if ((o.com || o.com_vel || o.h || o.hdot) && !(plan_total_mass(p) > 0))
        return set_err(GRBDA_EUNSUPPORTED, "the total mass of the model is not positive: the centre of mass and the centroidal momentum are not defined");
    return GRBDA_OK;
}
// One launch of centroidal_kernel over nb rows (arguments checked, nb > 0, device found): the spanning rates into the caller's work arrays
// vs, as [nb][span_count] when an output needs them (spanning<T>, as twists_stage; velocities alone: the acceleration half is computed at
// ydd = qd and not read), the scratch slab sized by the launch record, then the one launch site.
template <class T>
int centroidal_stage(const grbda_plan *p, const DeviceTables &t, const T *q, const T *qd, const T *ydd, const CentroidalOut<T> &o, T *vs, T *as,
                     size_t nb, int device, void *stream)
{
    const bool velocities = centroidal_velocities(o), rates = o.hdot != nullptr;
    if (velocities)
        if (int rc = spanning<T>(p, q, qd, rates ? ydd : qd, vs, as, nb, device, stream)) return rc;
    const CentroidalLaunch L = centroidal_launch(velocities, rates, centroidal_rows(p->host).n_parent_bodies, t.n_cu, nb);
    void *scratch = nullptr;
    if (int rc = ensure_scratch(p, device, stream, scratch_bytes(L.grid, L.slab_rows, sizeof(T)), &scratch)) return rc;
    const DevPlan<T> d = make_dev_plan<T>(p, t, false, false);
    const std::array<T, 3> g = gravity3<T>(p);
    hipError_t e = launch_centroidal<T>(d, p->host.n_clusters, span_count(p), t.centroidal_rows, L, q, velocities ? vs : nullptr, rates ? as : nullptr,
                                        g.data(), static_cast<T>(plan_total_mass(p)), o, nb, static_cast<T *>(scratch), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "centroidal launch");
}
// grbda_energy_* and grbda_centroidal_*: the batch in chunks of the work slab (the spanning rates are all it holds; none without velocities)
template <class T>
int centroidal(const grbda_plan *p, const T *q, const T *qd, const T *ydd, const CentroidalOut<T> &o, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = centroidal_args<T>(p, q, qd, ydd, o, B)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, ns = static_cast<size_t>(span_count(p));
    Chunk c{B, 0};
    T *vs = nullptr, *as = nullptr;
    if (centroidal_velocities(o)) {
        c = budgeted_chunk(p, p->work, device, stream, 1024ull << 20, 2 * ns * sizeof(T), B);
        void *wptr = nullptr;
        if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
        Carver<T> w(wptr, c.chunk * 2 * ns);
        vs = w.take(c.chunk * ns);
        as = w.take(c.chunk * ns);
        assert(w.taken == w.cap);
    }
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        CentroidalOut<T> oc{};
        oc.kinetic = o.kinetic ? o.kinetic + b0 : nullptr;
        oc.potential = o.potential ? o.potential + b0 : nullptr;
        oc.com = o.com ? o.com + b0 * 3 : nullptr;
        oc.com_vel = o.com_vel ? o.com_vel + b0 * 3 : nullptr;
        oc.h = o.h ? o.h + b0 * 6 : nullptr;
        oc.hdot = o.hdot ? o.hdot + b0 * 6 : nullptr;
        if (int rc = centroidal_stage<T>(p, *t, q + b0 * nq, qd ? qd + b0 * nv : nullptr, ydd ? ydd + b0 * nv : nullptr, oc, vs, as, nb, device, stream))
            return rc;
    }
    return GRBDA_OK;
}
// row (b, j) of the expanded batch of the momentum matrix: state b at the unit velocity e_j
template <class T>
__global__ void unit_velocity_rows_kernel(const T *__restrict__ q, int nq, int nv, size_t nb, T *__restrict__ q_x, T *__restrict__ qd_x)
{
    const size_t width = (size_t)(nq + nv), total = nb * (size_t)nv * width;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t row = t / width;
        const int col = (int)(t % width);
        if (col < nq) q_x[row * nq + col] = q[(row / nv) * nq + col];
        else qd_x[row * nv + (col - nq)] = (size_t)(col - nq) == row % nv ? T(1) : T(0);
    }
}
template <class T>
int centroidal_matrix_args(const grbda_plan *p, const T *q, const T *A, size_t B)
{
    if (!q || !A) return set_err(GRBDA_EINVAL, "null argument");
    const void *const in[1] = {q}, *const out[1] = {A};
    const size_t in_bytes[1] = {B * static_cast<size_t>(p->host.nq) * sizeof(T)}, out_bytes[1] = {B * 6 * static_cast<size_t>(p->host.nv) * sizeof(T)};
    if (int rc = no_overlap(in, in_bytes, out, out_bytes)) return rc;
    if (!(plan_total_mass(p) > 0))
        return set_err(GRBDA_EUNSUPPORTED, "the total mass of the model is not positive: the centre of mass and the centroidal momentum are not defined");
    return GRBDA_OK;
}
// A[B][6][nv], h = A(q) yd: momentum is linear in yd, so column j is the h of (q, e_j) -- the expanded batch of nv rows per state through the
// same two stages, as many states per pass as the work slab holds (per state nv rows of q, qd, and the two spanning rates)
template <class T>
int centroidal_matrix(const grbda_plan *p, const T *q, T *A, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = centroidal_matrix_args<T>(p, q, A, B)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, ns = static_cast<size_t>(span_count(p));
    const size_t per_state = nv * (nq + nv + 2 * ns);
    const Chunk c = fixed_chunk(work_budget(p, p->work, device, stream, 1024ull << 20), per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    Carver<T> w(wptr, c.chunk * per_state);
    T *q_x = w.take(c.chunk * nv * nq), *qd_x = w.take(c.chunk * nv * nv), *vs = w.take(c.chunk * nv * ns), *as = w.take(c.chunk * nv * ns);
    assert(w.taken == w.cap);
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        hipLaunchKernelGGL((unit_velocity_rows_kernel<T>), dim3(blocks_for(nb * nv * (nq + nv))), dim3(256), 0, static_cast<hipStream_t>(stream), q + b0 * nq,
                           static_cast<int>(nq), static_cast<int>(nv), nb, q_x, qd_x);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_err(e, "unit velocity rows launch");
        CentroidalOut<T> o{};
        o.h = A + b0 * 6 * nv;
        o.h_cols = static_cast<int>(nv);
        if (int rc = centroidal_stage<T>(p, *t, q_x, qd_x, static_cast<const T *>(nullptr), o, vs, as, nb * nv, device, stream)) return rc;
    }
    return GRBDA_OK;
}

// ---- frame Jacobians and their drift at a listed few body frames (include/grbda_hip_jacobians.h; frame_jacobian_kernels.hip) ------------
// (the walk of route 0, JacWalkHost and build_jac_walk: walk.h)
template <class T>
JacWalk<T> device_jac_walk(const grbda_plan *p, const DeviceTables &t, const JacWalkHost &H, const double *offsets, int frame)
{
    JacWalk<T> W{};
    W.n_steps = H.walk_len;
    W.n_list = H.n;
    W.n_saved = H.max_saved;
    W.nq = p->host.nq;
    W.nv = p->host.nv;
    W.ori_repr = p->host.ori_repr;
    W.world = frame == GRBDA_WRENCH_WORLD;
    W.consts = consts_of<T>(t);
    for (int i = 0; i < H.n; i++)  // component k of a plan-frame vector is component (k + canon + 1) % 3 of the reference-frame one
        for (int k = 0; k < 3; k++) W.off[i][k] = offsets ? static_cast<T>(offsets[3 * i + (k + H.canon[i] + 1) % 3]) : T(0);
    std::memcpy(W.cols, H.cols, sizeof(W.cols));
    std::memcpy(W.canon, H.canon, sizeof(W.canon));
    std::memcpy(W.step, H.step, sizeof(W.step));
    return W;
}
// Everything the entry points refuse, on the host and before any device call
template <class T>
int frame_jacobians_args(const grbda_plan *p, const T *q, const T *qd, int n, const int *bodies, int frame, const T *J, const T *drift, size_t B)
{
    if (!q) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = body_list_check(p, n, bodies, bodies)) return rc;
    if (frame != GRBDA_WRENCH_BODY && frame != GRBDA_WRENCH_WORLD) return set_err(GRBDA_EINVAL, "frame must be GRBDA_WRENCH_BODY or GRBDA_WRENCH_WORLD");
    if (n > 0 && !J && !drift) return set_err(GRBDA_EINVAL, "no output asked for: J and drift are both null");
    if (n > 0 && drift && !qd) return set_err(GRBDA_EINVAL, "the drift needs qd");
    const size_t nv = p->host.nv;
    const void *const in[2] = {q, drift ? qd : nullptr}, *const outs[2] = {n > 0 ? J : nullptr, n > 0 ? drift : nullptr};
    const size_t in_bytes[2] = {B * static_cast<size_t>(p->host.nq) * sizeof(T), B * nv * sizeof(T)};
    const size_t out_bytes[2] = {B * static_cast<size_t>(n) * 6 * nv * sizeof(T), B * static_cast<size_t>(n) * 6 * sizeof(T)};
    return no_overlap(in, in_bytes, outs, out_bytes);
}
// Route 1 of J over nb states, the stage grbda_frame_jacobians_* and the route-1 J^T f share: the expanded batch (nv rows per state: q, the
// unit velocities, zero accelerations) through body_list_stage and the finishing kernel.  lt: list_work of the listed twists; the stage
// takes jacobian_columns_work() elements per state from w.  Xa: the listed poses, read for world frames only.
size_t jacobian_columns_work(size_t nq, size_t nv, const ListWork &lt) { return nv * (nq + 2 * nv + lt.per_state()); }
template <class T>
int jacobian_columns_stage(const grbda_plan *p, const DeviceTables &t, const BodyWalkHost &H, const FrameSet<T> &F, const ListWork &lt, Carver<T> &w,
                           const T *qc, const T *Xa, size_t nb, T *J, int device, void *stream)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const size_t nq = p->host.nq, nv = p->host.nv, rows = nb * nv;
    T *q_x = w.take(rows * nq), *qd_x = w.take(rows * nv), *z_x = w.take(rows * nv);
    const auto m = lt.take(w, rows);
    hipLaunchKernelGGL((unit_velocity_rows_kernel<T>), dim3(blocks_for(rows * (nq + nv))), dim3(256), 0, hs, qc, static_cast<int>(nq),
                       static_cast<int>(nv), nb, q_x, qd_x);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_err(e, "unit velocity rows launch");
    if (hipError_t e = hipMemsetAsync(z_x, 0, rows * nv * sizeof(T), hs); e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    if (int rc = body_list_stage<T>(p, t, H, true, q_x, qd_x, z_x, m.out, m.full, m.vs, m.as, rows, device, stream)) return rc;
    if (hipError_t e = launch_frame_jacobian_columns<T>(F, m.out, Xa, static_cast<int>(nv), nb, J, hs); e != hipSuccess)
        return hip_err(e, "frame Jacobian columns launch");
    return GRBDA_OK;
}
// the frames as the finishing kernels of route 1 take them: the offsets in the reference's body axes, the column masks of the walk builder
template <class T>
FrameSet<T> frame_set(const JacWalkHost &JH, int n, const double *offsets, int frame)
{
    FrameSet<T> F{};
    F.n = n;
    F.world = frame == GRBDA_WRENCH_WORLD;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) F.off[i][k] = offsets ? static_cast<T>(offsets[3 * i + k]) : T(0);
    std::memcpy(F.cols, JH.cols, sizeof(F.cols));
    return F;
}
// the launch shape of the walk kernels of this family: one-wavefront workgroups, as many per CU as `lds` bytes each allow, at most eight
int jac_walk_grid(const DeviceTables &t, size_t lds, size_t nb)
{
    return static_cast<int>(tile_grid(t.n_cu, std::min<size_t>(8, lds_workgroups_per_cu(lds)), nb));
}
// Route 0: the walk kernel writes J.  Route 1: per chunk the expanded batch (nv rows per state: q, the unit velocities, zero accelerations)
// through body_list_stage and the finishing kernel.  The drift, on both routes: the listed twists at (q, qd, 0) with a zero root
// acceleration, and the finishing kernel.  World frames read the listed poses (body_list_stage) in both finishing kernels.
template <class T>
int frame_jacobians_run(const grbda_plan *p, const T *q, const T *qd, int n, const int *bodies, const double *offsets, int frame, T *J, T *drift,
                        size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = frame_jacobians_args<T>(p, q, qd, n, bodies, frame, J, drift, B)) return rc;
    if (n == 0 || B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const Layout &L = layout_of(p->host, sizeof(T) == 4 ? 0 : 1);
    const JacWalkHost JH = build_jac_walk(p->host, L, n, bodies);
    const BodyWalkHost H = build_body_walk(p->host, L, n, bodies);
    const FrameSet<T> F = frame_set<T>(JH, n, offsets, frame);
    const bool walk = J && JH.route == 0, columns = J && JH.route == 1, poses = F.world && (columns || drift);
    const size_t nq = p->host.nq, nv = p->host.nv, jn = static_cast<size_t>(n) * 6 * nv;
    const ListWork lp = list_work(p, H, false, n), lt = list_work(p, H, true, n);  // the listed poses; the listed twists
    const auto launch_walk = [&](size_t b0, size_t nb) {
        const JacWalk<T> W = device_jac_walk<T>(p, *t, JH, offsets, frame);
        const size_t lds = static_cast<size_t>(JH.max_saved + n) * 12 * kWave * sizeof(T);
        const int grid = jac_walk_grid(*t, lds, nb);
        hipError_t e = launch_frame_jacobian_walk<T>(W, q + b0 * nq, J + b0 * jn, nb, grid, hs);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "frame Jacobian walk launch");
    };
    const size_t per_state = (poses ? lp.per_state() : 0) + (columns ? jacobian_columns_work(nq, nv, lt) : 0) + (drift ? nv + lt.per_state() : 0);
    if (per_state == 0) return launch_walk(0, B);
    const Chunk c = budgeted_chunk(p, p->work, device, stream, 1024ull << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        const T *qc = q + b0 * nq;
        T *Xa = nullptr;
        if (poses) {
            const auto m = lp.take(w, nb);
            Xa = m.out;
            if (int rc = body_list_stage<T>(p, *t, H, false, qc, nullptr, nullptr, Xa, m.full, m.vs, m.as, nb, device, stream)) return rc;
        }
        if (walk)
            if (int rc = launch_walk(b0, nb)) return rc;
        if (columns)
            if (int rc = jacobian_columns_stage<T>(p, *t, H, F, lt, w, qc, Xa, nb, J + b0 * jn, device, stream)) return rc;
        if (drift) {
            T *z = w.take(nb * nv);
            const auto m = lt.take(w, nb);
            if (hipError_t e = hipMemsetAsync(z, 0, nb * nv * sizeof(T), hs); e != hipSuccess) return hip_err(e, "hipMemsetAsync");
            if (int rc = body_list_stage<T>(p, *t, H, true, qc, qd + b0 * nv, z, m.out, m.full, m.vs, m.as, nb, device, stream, false)) return rc;
            if (hipError_t e = launch_frame_drift<T>(F, m.out, Xa, nb, drift + b0 * static_cast<size_t>(n) * 6, hs); e != hipSuccess)
                return hip_err(e, "frame drift launch");
        }
    }
    return GRBDA_OK;
}
int frame_jacobians_host_f64(const grbda_plan *p, const double *q, const double *qd, int n, const int *bodies, const double *offsets, int frame,
                             double *J, double *drift, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = frame_jacobians_args<double>(p, q, qd, n, bodies, frame, J, drift, B)) return rc;
    if (n == 0 || B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = drift ? st.in(qd, B * nv) : nullptr;
    double *dJ = J ? st.out(J, B * static_cast<size_t>(n) * 6 * nv) : nullptr, *dd = drift ? st.out(drift, B * static_cast<size_t>(n) * 6) : nullptr;
    return st.run([&] { return frame_jacobians_run<double>(p, dq, dqd, n, bodies, offsets, frame, dJ, dd, B, device, nullptr); });
}

// ---- J v and J^T f at a listed few body frames (include/grbda_hip_jacobian_products.h; frame_product_kernels.hip) -------------------
// Everything the entry points refuse, on the host and before any device call
template <class T>
int frame_products_args(const grbda_plan *p, const T *q, const T *v, const T *f, int n, const int *bodies, int frame, const T *Jv, const T *JTf,
                        size_t B)
{
    if (!q) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = body_list_check(p, n, bodies, bodies)) return rc;
    if (frame != GRBDA_WRENCH_BODY && frame != GRBDA_WRENCH_WORLD) return set_err(GRBDA_EINVAL, "frame must be GRBDA_WRENCH_BODY or GRBDA_WRENCH_WORLD");
    if (n > 0 && !Jv && !JTf) return set_err(GRBDA_EINVAL, "no output asked for: Jv and JTf are both null");
    if (n > 0 && !Jv != !v) return set_err(GRBDA_EINVAL, Jv ? "Jv needs v" : "v is given without Jv");
    if (n > 0 && !JTf != !f) return set_err(GRBDA_EINVAL, JTf ? "JTf needs f" : "f is given without JTf");
    const size_t nv = p->host.nv, n6 = static_cast<size_t>(n) * 6;
    const void *const in[3] = {q, n > 0 ? v : nullptr, n > 0 ? f : nullptr}, *const outs[2] = {n > 0 ? Jv : nullptr, n > 0 ? JTf : nullptr};
    const size_t in_bytes[3] = {B * static_cast<size_t>(p->host.nq) * sizeof(T), B * nv * sizeof(T), B * n6 * sizeof(T)};
    const size_t out_bytes[2] = {B * n6 * sizeof(T), B * nv * sizeof(T)};
    return no_overlap(in, in_bytes, outs, out_bytes);
}
// The route is the one of frame_jacobians_run for the list (build_jac_walk).  Route 0: one walk kernel, no work memory.  Route 1, per
// chunk of the work slab: the listed poses for world frames; J v from the listed twists at (q, v, 0) with a zero root acceleration -- one
// row per state -- and the finishing kernel; J^T f from the chunk's J by jacobian_columns_stage and the contraction kernel.
template <class T>
int frame_products_run(const grbda_plan *p, const T *q, const T *v, const T *f, int n, const int *bodies, const double *offsets, int frame, T *Jv,
                       T *JTf, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = frame_products_args<T>(p, q, v, f, n, bodies, frame, Jv, JTf, B)) return rc;
    if (n == 0 || B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const Layout &L = layout_of(p->host, sizeof(T) == 4 ? 0 : 1);
    const JacWalkHost JH = build_jac_walk(p->host, L, n, bodies);
    const size_t nq = p->host.nq, nv = p->host.nv, n6 = static_cast<size_t>(n) * 6, jn = n6 * nv;
    if (JH.route == 0) {
        const JacWalk<T> W = device_jac_walk<T>(p, *t, JH, offsets, frame);
        const size_t lds = static_cast<size_t>(18 * JH.max_saved + 6 * n) * kWave * sizeof(T);
        hipError_t e = launch_frame_product_walk<T>(W, q, v, f, Jv, JTf, B, jac_walk_grid(*t, lds, B), hs);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "frame product walk launch");
    }
    const BodyWalkHost H = build_body_walk(p->host, L, n, bodies);
    const FrameSet<T> F = frame_set<T>(JH, n, offsets, frame);
    const ListWork lp = list_work(p, H, false, n), lt = list_work(p, H, true, n);  // the listed poses; the listed twists
    const size_t per_state = (F.world ? lp.per_state() : 0) + (Jv ? nv + lt.per_state() : 0) + (JTf ? jn + jacobian_columns_work(nq, nv, lt) : 0);
    const Chunk c = budgeted_chunk(p, p->work, device, stream, 1024ull << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        const T *qc = q + b0 * nq;
        T *Xa = nullptr;
        if (F.world) {
            const auto m = lp.take(w, nb);
            Xa = m.out;
            if (int rc = body_list_stage<T>(p, *t, H, false, qc, nullptr, nullptr, Xa, m.full, m.vs, m.as, nb, device, stream)) return rc;
        }
        if (Jv) {
            T *z = w.take(nb * nv);
            const auto m = lt.take(w, nb);
            if (hipError_t e = hipMemsetAsync(z, 0, nb * nv * sizeof(T), hs); e != hipSuccess) return hip_err(e, "hipMemsetAsync");
            if (int rc = body_list_stage<T>(p, *t, H, true, qc, v + b0 * nv, z, m.out, m.full, m.vs, m.as, nb, device, stream, false)) return rc;
            if (hipError_t e = launch_frame_jv<T>(F, m.out, Xa, nb, Jv + b0 * n6, hs); e != hipSuccess) return hip_err(e, "frame Jv launch");
        }
        if (JTf) {
            T *J = w.take(nb * jn);
            if (int rc = jacobian_columns_stage<T>(p, *t, H, F, lt, w, qc, Xa, nb, J, device, stream)) return rc;
            if (hipError_t e = launch_frame_jtf<T>(J, f + b0 * n6, n, static_cast<int>(nv), nb, JTf + b0 * nv, hs); e != hipSuccess)
                return hip_err(e, "frame JTf launch");
        }
    }
    return GRBDA_OK;
}
int frame_products_host_f64(const grbda_plan *p, const double *q, const double *v, const double *f, int n, const int *bodies, const double *offsets,
                            int frame, double *Jv, double *JTf, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = frame_products_args<double>(p, q, v, f, n, bodies, frame, Jv, JTf, B)) return rc;
    if (n == 0 || B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, n6 = static_cast<size_t>(n) * 6;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dv = Jv ? st.in(v, B * nv) : nullptr, *df = JTf ? st.in(f, B * n6) : nullptr;
    double *dJv = Jv ? st.out(Jv, B * n6) : nullptr, *dJTf = JTf ? st.out(JTf, B * nv) : nullptr;
    return st.run([&] { return frame_products_run<double>(p, dq, dv, df, n, bodies, offsets, frame, dJv, dJTf, B, device, nullptr); });
}

// ---- inverse operational-space inertia of a set of contact frames (include/grbda_hip.h) -----------------------
// (ContactSet<T>, kMaxContacts: devplan.h)
// world wrench (about the world origin) of a Cartesian force at a point fixed in body `body`
template <class T>
__global__ void wrench_kernel(const T *__restrict__ Xa, const T *__restrict__ force, int n_bodies, int body, T ox, T oy,
                              T oz, size_t nb, T *__restrict__ fext)
{
    for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < nb; b += (size_t)gridDim.x * blockDim.x) {
        const T *X = Xa + (b * n_bodies + body) * 12;
        // p = r + E^T offset (E: world -> body)
        const T px = X[9] + X[0] * ox + X[3] * oy + X[6] * oz;
        const T py = X[10] + X[1] * ox + X[4] * oy + X[7] * oz;
        const T pz = X[11] + X[2] * ox + X[5] * oy + X[8] * oz;
        const T fx = force[3 * b], fy = force[3 * b + 1], fz = force[3 * b + 2];
        T *w = fext + b * (size_t)n_bodies * 6;
        for (int i = 0; i < n_bodies * 6; i++) w[i] = 0;
        w += (size_t)body * 6;
        w[0] = py * fz - pz * fy;
        w[1] = pz * fx - px * fz;
        w[2] = px * fy - py * fx;
        w[3] = fx;
        w[4] = fy;
        w[5] = fz;
    }
}
// dstate = a1 - a0 ;  lambda_inv = (t0 - t1) . dstate
template <class T>
__global__ void test_force_finish(const T *__restrict__ a1, const T *__restrict__ a0, const T *__restrict__ t1,
                                  const T *__restrict__ t0, int nv, size_t nb, T *__restrict__ dstate,
                                  T *__restrict__ lambda_inv)
{
    for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < nb; b += (size_t)gridDim.x * blockDim.x) {
        T s = 0;
        for (int i = 0; i < nv; i++) {
            const T d = a1[b * nv + i] - a0[b * nv + i];
            dstate[b * nv + i] = d;
            s += (t0[b * nv + i] - t1[b * nv + i]) * d;
        }
        lambda_inv[b] = s;
    }
}

// rows (b, j), j < 6 n: unit spatial force e_{j % 6} in contact frame j / 6 (body axes, origin at the contact
// point) as a world wrench on that body; row 6 n: no force
template <class T>
__global__ void osim_expand_kernel(ContactSet<T> cs, const T *__restrict__ q, const T *__restrict__ Xa, int nq,
                                   int n_bodies, size_t nb, T *__restrict__ qx, T *__restrict__ fext)
{
    const int R = 6 * cs.n + 1;
    const size_t rows = nb * (size_t)R;
    for (size_t row = blockIdx.x * (size_t)blockDim.x + threadIdx.x; row < rows; row += (size_t)gridDim.x * blockDim.x) {
        const size_t b = row / R;
        const int j = (int)(row % R);
        for (int i = 0; i < nq; i++) qx[row * nq + i] = q[b * nq + i];
        T *w = fext + row * (size_t)n_bodies * 6;
        for (int i = 0; i < n_bodies * 6; i++) w[i] = 0;
        if (j == R - 1) continue;
        const int c = j / 6, k = j % 6;
        const T *X = Xa + (b * n_bodies + cs.body[c]) * 12;
        const T ox = cs.off[c][0], oy = cs.off[c][1], oz = cs.off[c][2];
        const T p[3] = {X[9] + X[0] * ox + X[3] * oy + X[6] * oz, X[10] + X[1] * ox + X[4] * oy + X[7] * oz,
                        X[11] + X[2] * ox + X[5] * oy + X[8] * oz};
        const int a = k % 3;
        const T e[3] = {X[3 * a], X[3 * a + 1], X[3 * a + 2]};  // E^T e_a: body axis a in world coordinates
        w += (size_t)cs.body[c] * 6;
        if (k < 3) {  // unit moment
            w[0] = e[0]; w[1] = e[1]; w[2] = e[2];
        } else {      // unit force at p
            w[0] = p[1] * e[2] - p[2] * e[1];
            w[1] = p[2] * e[0] - p[0] * e[2];
            w[2] = p[0] * e[1] - p[1] * e[0];
            w[3] = e[0]; w[4] = e[1]; w[5] = e[2];
        }
    }
}
// g_i = tau(no force) - tau(w_i) = J^T e_i,  a_j = ydd(w_j) - ydd(no force) = H^-1 J^T e_j,  Linv[i][j] = g_i . a_j
template <class T>
__global__ void osim_combine_kernel(const T *__restrict__ acc, const T *__restrict__ tau, int nv, int m, size_t nb,
                                    T *__restrict__ Linv, T *__restrict__ J)
{
    const size_t total = nb * (size_t)m * m;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t b = t / ((size_t)m * m);
        const int i = (int)((t / m) % m), j = (int)(t % m);
        const T *ab = acc + b * (size_t)(m + 1) * nv, *tb = tau + b * (size_t)(m + 1) * nv;
        T s = 0;
        for (int v = 0; v < nv; v++) {
            const T g = tb[(size_t)m * nv + v] - tb[(size_t)i * nv + v];
            s += g * (ab[(size_t)j * nv + v] - ab[(size_t)m * nv + v]);
            if (J && j == 0) J[(b * m + i) * nv + v] = g;
        }
        Linv[t] = s;
    }
}

// The unit-wrench route: 6 n + 1 rows per state through the forward and the inverse dynamics.  Scalars of work space per state: the poses;
// per row q, wrenches, zeros and the two results.
size_t osim_unit_per_state(const grbda_plan *p, int n_contacts)
{
    const size_t nq = p->host.nq, nv = p->host.nv, nbod = p->host.n_bodies, R = 6 * static_cast<size_t>(n_contacts) + 1;
    return nbod * 12 + R * (nq + nbod * 6 + 3 * nv);
}
// Which way one call takes the inverse OSIM (grbda_inv_osim_*, grbda_apply_test_force_*, grbda_contact_dynamics_*; table in DESIGN.md):
// force propagation along the contacts' ancestor paths (chain_kernels.hip, osim_chain_kernel) for models the chain program covers and
// contact frames on link / base bodies, else unit wrenches.  Asked once per call, after the argument checks.
template <class T>
struct OsimRoute {
    bool chain;           // force propagation; else the unit-wrench route
    OsimArgs<T> args;     // chain: the argument block of the force-propagation kernel for these contacts
    size_t ws_per_state;  // scalars of work space per state: nv zeros (chain), osim_unit_per_state (unit wrenches)
};
// (tf_*: applyTestForce mode, one contact)
template <class T>
OsimRoute<T> choose_osim(const grbda_plan *p, int n_contacts, const int *bodies, const double *offsets, bool want_J, const T *tf_force, T *tf_lambda,
                         T *tf_dstate)
{
    const HostPlan &h = p->host;
    const ChainSlot slot = chain_slot(sizeof(T) == 8);
    const ChainProgram &cp = h.chain[slot];
    OsimRoute<T> r{};  // (every early return below: the unit-wrench route)
    r.ws_per_state = osim_unit_per_state(p, n_contacts);
    // (programs with generic clusters -- plan.h, ChainGen -- have no walk steps in the force-propagation kernel)
    if (p->opt.no_chain || p->opt.no_efpa || !cp.ok || !cp.gens.empty() || n_contacts > kOsimMaxContacts) return r;
    const Layout &L = h.lay64;
    OsimArgs<T> &A = r.args;
    A.n_contacts = n_contacts;
    A.want_J = want_J ? 1 : 0;
    A.test_force = tf_force ? 1 : 0;
    A.force = tf_force;
    A.lambda_inv = tf_lambda;
    A.dstate = tf_dstate;
    if (tf_force && n_contacts != 1) return r;
    std::vector<std::vector<int>> path_clusters(n_contacts);
    int max_rows = 0;
    for (int e = 0; e < n_contacts; e++) {
        const int b = bodies[e];
        int c = h.crba.bodies[b].cluster;
        int rows = 0, len = 0;
        bool first = true;
        while (c >= 0) {
            if (len >= kOsimMaxPath) return r;
            const ClusterRec &cr = L.clusters[c];
            OsimStep st;
            st.v_index = static_cast<int16_t>(cr.v_index);
            st.w_row = static_cast<int16_t>(rows);
            int found = -1;
            if (cr.kind == CK_FREE) {
                for (size_t i = 0; i < cp.frees.size(); i++)
                    if (cp.frees[i].v_index == cr.v_index) found = static_cast<int>(i);
                st.kind = OSIM_FREE;
                rows += 6;
            } else if (cr.shape != SHAPE_GENERIC) {
                if (first && b != cr.link_body) return r;  // a contact on a rotor
                for (size_t i = 0; i < cp.links.size(); i++)
                    if (cp.links[i].v_index == cr.v_index) found = static_cast<int>(i);
                st.kind = OSIM_LINK;
                rows += 1;
            } else if (cr.kind == CK_LOOP || [&] {
                           for (const ChainDiff &df : cp.diffs)
                               if (df.v_index == cr.v_index) return true;
                           return false;
                       }()) {
                // two-rotor differential, or an explicit pair that runs through its segments: the path enters at link1 (a
                // contact on it) or at link2 (a contact on it or below)
                for (size_t i = 0; i < cp.diffs.size(); i++)
                    if (cp.diffs[i].v_index == cr.v_index) found = static_cast<int>(i);
                if (found < 0) return r;
                if (!first || L.bodies[b].cofs == cp.diffs[found].cofs[1]) st.kind = OSIM_DIFF_LINK2;
                else if (L.bodies[b].cofs == cp.diffs[found].cofs[0]) st.kind = OSIM_DIFF_LINK1;
                else return r;  // a contact on a rotor
                rows += 2;
            } else {
                if (!first) return r;  // pair clusters are leaves of the chain program
                for (size_t i = 0; i < cp.pairs.size(); i++)
                    if (cp.pairs[i].v_index == cr.v_index) found = static_cast<int>(i);
                if (found < 0) return r;
                if (L.bodies[b].cofs == cp.pairs[found].cofs[0]) st.kind = OSIM_PAIR_LINK1;
                else if (L.bodies[b].cofs == cp.pairs[found].cofs[1]) st.kind = OSIM_PAIR_LINK2;
                else return r;
                rows += 2;
            }
            if (found < 0) return r;
            st.rec = static_cast<int16_t>(found);
            A.path[e][len++] = st;
            path_clusters[e].push_back(c);
            first = false;
            c = cr.parent_body >= 0 ? h.crba.bodies[cr.parent_body].cluster : -1;
        }
        A.path_len[e] = len;
        A.n_rows[e] = rows;
        if (rows > max_rows) max_rows = rows;
        // K0: wrench on the contact body, in the PLAN's body frame (canonical joint axes, plan.cpp), per unit contact wrench
        // given in the reference's body axes at the contact point: [n; f] -> [n + o x f; f], then the cyclic permutation
        const double *o = offsets + 3 * e;
        double W[36] = {0};
        for (int j = 0; j < 3; j++) {
            W[6 * j + j] = 1.0;            // unit moment e_j
            W[6 * (3 + j) + 3 + j] = 1.0;  // unit force e_j ...
        }
        // ... and its moment about the body origin o x e_j (column 3 + j, rows 0..2)
        W[6 * 1 + 3] = o[2];  W[6 * 2 + 3] = -o[1];   // o x e_x = (0, o_z, -o_y)
        W[6 * 0 + 4] = -o[2]; W[6 * 2 + 4] = o[0];    // o x e_y = (-o_z, 0, o_x)
        W[6 * 0 + 5] = o[1];  W[6 * 1 + 5] = -o[0];   // o x e_z = (o_y, -o_x, 0)
        const int ca = L.bodies[b].canon_axis;  // v_plan = Rc v_ref: x -> z: rows (y, z, x); y -> z: rows (z, x, y)
        const int perm[3][3] = {{1, 2, 0}, {2, 0, 1}, {0, 1, 2}};
        if (e == 0)
            for (int i = 0; i < 3; i++) A.perm[i] = perm[ca][i];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 6; j++) {
                A.K0[e][6 * i + j] = static_cast<T>(W[6 * perm[ca][i] + j]);
                A.K0[e][6 * (3 + i) + j] = static_cast<T>(W[6 * (3 + perm[ca][i]) + j]);
            }
    }
    for (int e1 = 0; e1 < n_contacts; e1++)
        for (int e2 = 0; e2 < n_contacts; e2++) {
            const std::vector<int> &a = path_clusters[e1], &b2 = path_clusters[e2];
            int rows = 0;
            size_t i = a.size(), j = b2.size();
            while (i > 0 && j > 0 && a[i - 1] == b2[j - 1]) {
                const ClusterRec &cr = L.clusters[a[i - 1]];
                rows += cr.kind == CK_FREE ? 6 : cr.n;
                i--;
                j--;
            }
            A.common[e1][e2] = rows;
        }
    A.w_base = cp.n_glb;
    A.w_stride = 6 * max_rows;
    r.chain = true;
    r.ws_per_state = static_cast<size_t>(h.nv);
    return r;
}
// The force-propagation route: one launch of osim_chain_kernel.  zeros: B * nv scalars of the caller's work space (cleared here), which
// stand in for the velocities and torques of every tile.
template <class T>
int osim_chain_launch(const grbda_plan *p, const DeviceTables &t, const OsimArgs<T> &A, const T *q, T *Linv, T *J, size_t B, int device, void *stream,
                      T *zeros)
{
    const HostPlan &h = p->host;
    const ChainSlot slot = chain_slot(sizeof(T) == 8);
    const ChainProgram &cp = h.chain[slot];
    ChainDev<T> d = chain_dev<T>(p, t, slot);
    no_gens(d);
    d.n_glb_slots = cp.n_glb + A.n_contacts * A.w_stride;
    d.out_lds = -1;  // (the force-propagation kernel keeps its result rows in the slab)
    // (gravity enters the acceleration sweep only, which runs in applyTestForce mode alone -- there without it)
    if (A.test_force)
        for (int i = 0; i < 6; i++) d.a_root[i] = T(0);
    // one wavefront per SIMD: the walk kernel is not register-tuned (no LDS-fit clamp: inherited, not chosen)
    LaunchShape s;
    T *scratch = nullptr;
    if (int rc = aux_launch<T>(p, t, B, 4, static_cast<size_t>(cp.n_lds) * kWave * sizeof(T), false, d.n_glb_slots, device, stream, s, scratch)) return rc;
    d.lds_bytes = static_cast<int>(s.lds_bytes);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    hipError_t e;
    if ((e = hipMemsetAsync(zeros, 0, B * static_cast<size_t>(h.nv) * sizeof(T), hs)) != hipSuccess) return hip_err(e, "hipMemsetAsync");
    e = launch_osim_chain<T>(d, A, q, static_cast<const T *>(zeros), Linv, J, B, scratch, static_cast<int>(s.grid), s.lds_bytes, hs);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "osim chain launch");
}
// nb states of the unit-wrench route on the caller's work space: takes nb * osim_unit_per_state scalars from w
template <class T>
int inv_osim_unit(const grbda_plan *p, const DeviceTables &t, const ContactSet<T> &cs, const T *q, T *Linv, T *J, size_t nb, int device, void *stream,
                  Carver<T> &w)
{
    const size_t nq = p->host.nq, nv = p->host.nv, nbod = p->host.n_bodies;
    const size_t m = 6 * static_cast<size_t>(cs.n), R = m + 1, nrows = nb * R;
    const size_t before = w.taken;
    T *Xa = w.take(nb * nbod * 12), *qx = w.take(nrows * nq), *fext = w.take(nrows * nbod * 6), *zero = w.take(nrows * nv);
    T *acc = w.take(nrows * nv), *tau = w.take(nrows * nv);
    assert(w.taken - before == nb * osim_unit_per_state(p, cs.n));
    (void)before;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(zero, 0, nrows * nv * sizeof(T), hs);
    if (e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    if (int rc = poses_stage<T>(p, t, q, Xa, nb, stream)) return rc;
    hipLaunchKernelGGL((osim_expand_kernel<T>), dim3(blocks_for(nrows)), dim3(256), 0, hs, cs, q, Xa, static_cast<int>(nq), static_cast<int>(nbod), nb,
                       qx, fext);
    if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "expand launch");
    // (without gravity: the rows are differenced against the row that has no wrench, and gravity in both would cancel only up to rounding
    // -- the inverse OSIM, and the contact impulse built on it, then differ between two gravities, 8.5e-5 of 10 in fp32)
    int rc;
    if ((rc = run<T>(p, false, qx, zero, zero, fext, acc, nrows, device, stream, false)) ||
        (rc = run<T>(p, true, qx, zero, zero, fext, tau, nrows, device, stream, false)))
        return rc;
    hipLaunchKernelGGL((osim_combine_kernel<T>), dim3(blocks_for(nb * m * m)), dim3(256), 0, hs, acc, tau, static_cast<int>(nv), static_cast<int>(m), nb,
                       Linv, J);
    return (e = hipGetLastError()) == hipSuccess ? GRBDA_OK : hip_err(e, "combine launch");
}
// nb states of the inverse OSIM on the route chosen: takes nb * r.ws_per_state scalars from w
template <class T>
int osim_stage(const grbda_plan *p, const DeviceTables &t, const OsimRoute<T> &r, const ContactSet<T> &cs, const T *q, T *Linv, T *J, size_t nb, int device,
               void *stream, Carver<T> &w)
{
    if (r.chain) return osim_chain_launch<T>(p, t, r.args, q, Linv, J, nb, device, stream, w.take(nb * r.ws_per_state));
    return inv_osim_unit<T>(p, t, cs, q, Linv, J, nb, device, stream, w);
}

// grbda_apply_test_force_*: the force-propagation kernel in applyTestForce mode, one unchunked launch; else four runs of the dynamics per
// chunk, with and without the point's wrench
template <class T>
int test_force(const grbda_plan *p, const T *q, int body, const double *offset, const T *force, T *lambda_inv, T *dstate,
               size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !offset || !force || !lambda_inv || !dstate) return set_err(GRBDA_EINVAL, "null argument");
    if (body < 0 || body >= p->host.n_bodies) return set_err(GRBDA_EINVAL, "body index out of range");
    if (B == 0) return GRBDA_OK;
    const OsimRoute<T> r = choose_osim<T>(p, 1, &body, offset, false, force, lambda_inv, dstate);
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    void *wptr = nullptr;
    if (r.chain) {  // (the block of zeros: grown under ensure_work's capture rule)
        if (int rc = ensure_work(p, p->work, device, stream, B * r.ws_per_state * sizeof(T) + 256, &wptr)) return rc;
        return osim_chain_launch<T>(p, *t, r.args, q, nullptr, nullptr, B, device, stream, static_cast<T *>(wptr));
    }
    const size_t nq = p->host.nq, nv = p->host.nv, nbod = p->host.n_bodies;
    const size_t per_state = nbod * 18 + 5 * nv;  // poses, wrenches, zeros, four results
    const Chunk c = fixed_chunk(256u << 20, per_state * sizeof(T), B);
    const size_t chunk = c.chunk;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    Carver<T> w(wptr, chunk * per_state);
    T *Xa = w.take(chunk * nbod * 12), *fext = w.take(chunk * nbod * 6), *zero = w.take(chunk * nv);
    T *a1 = w.take(chunk * nv), *a0 = w.take(chunk * nv), *t1 = w.take(chunk * nv), *t0 = w.take(chunk * nv);
    assert(w.taken == w.cap);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(zero, 0, chunk * nv * sizeof(T), hs);
    if (e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    for (const auto [b0, nb] : ChunkWalk{B, chunk}) {
        const T *qc = q + b0 * nq;
        if (int rc = poses_stage<T>(p, *t, qc, Xa, nb, stream)) return rc;
        const int blocks = blocks_for(nb);
        hipLaunchKernelGGL((wrench_kernel<T>), dim3(blocks), dim3(256), 0, hs, Xa, force + 3 * b0, static_cast<int>(nbod),
                           body, static_cast<T>(offset[0]), static_cast<T>(offset[1]), static_cast<T>(offset[2]), nb, fext);
        if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "wrench launch");
        int rc;
        if ((rc = run<T>(p, false, qc, zero, zero, fext, a1, nb, device, stream)) ||
            (rc = run<T>(p, false, qc, zero, zero, nullptr, a0, nb, device, stream)) ||
            (rc = run<T>(p, true, qc, zero, zero, fext, t1, nb, device, stream)) ||
            (rc = run<T>(p, true, qc, zero, zero, nullptr, t0, nb, device, stream)))
            return rc;
        hipLaunchKernelGGL((test_force_finish<T>), dim3(blocks), dim3(256), 0, hs, a1, a0, t1, t0, static_cast<int>(nv), nb,
                           dstate + b0 * nv, lambda_inv + b0);
        if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "finish launch");
    }
    return GRBDA_OK;
}

// grbda_inv_osim_*: force propagation in one unchunked launch over the batch, unit wrenches in chunks of 256 MiB
template <class T>
int inv_osim(const grbda_plan *p, const T *q, int n_contacts, const int *bodies, const double *offsets, T *Linv, T *J,
             size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !Linv) return set_err(GRBDA_EINVAL, "null argument");
    ContactSet<T> cs;
    if (int rc = contact_set<T>(p, n_contacts, bodies, offsets, "frames", cs)) return rc;
    if (B == 0) return GRBDA_OK;
    const OsimRoute<T> r = choose_osim<T>(p, n_contacts, bodies, offsets, J != nullptr, nullptr, nullptr, nullptr);
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, m = 6 * static_cast<size_t>(n_contacts), per_state = r.ws_per_state;
    const Chunk c = r.chain ? Chunk{B, B * per_state * sizeof(T) + 256} : fixed_chunk(256u << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        if (int rc = osim_stage<T>(p, *t, r, cs, q + b0 * nq, Linv + b0 * m * m, J ? J + b0 * m * nv : nullptr, nb, device, stream, w)) return rc;
    }
    return GRBDA_OK;
}

// ---- contact points and contact-constrained forward dynamics (contact_kernels.hip; include/grbda_hip.h) -----------------------------
template <class T>
int contact_points_args(const grbda_plan *p, const T *q, const T *qd, const T *ydd, int n_contacts, const int *bodies, const double *offsets,
                        const T *pos, const T *vel, const T *acc, size_t B, ContactSet<T> &cs)
{
    if (!q) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = contact_set<T>(p, n_contacts, bodies, offsets, "points", cs)) return rc;
    if (!pos && !vel && !acc) return set_err(GRBDA_EINVAL, "no output asked for");
    if ((vel || acc) && !qd) return set_err(GRBDA_EINVAL, "vel and acc need qd");
    if (acc && !ydd) return set_err(GRBDA_EINVAL, "acc needs ydd");
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const size_t bo = B * static_cast<size_t>(n_contacts) * 3 * sizeof(T);
    const void *const in[3] = {q, qd, ydd}, *const out[3] = {pos, vel, acc};
    const size_t in_bytes[3] = {bq, bv, bv}, out_bytes[3] = {bo, bo, bo};
    return no_overlap(in, in_bytes, out, out_bytes);
}
// Per chunk: poses, and for vel / acc the twists (at ydd, or at zeros when only vel is asked for), then contact_points_kernel.  One slab of
// p->work for the whole pipeline (twists_stage takes its spanning rates from it).
template <class T>
int contact_points(const grbda_plan *p, const T *q, const T *qd, const T *ydd, int n_contacts, const int *bodies, const double *offsets, T *pos,
                   T *vel, T *acc, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<T> cs;
    if (int rc = contact_points_args<T>(p, q, qd, ydd, n_contacts, bodies, offsets, pos, vel, acc, B, cs)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, nbod = p->host.n_bodies, ns = static_cast<size_t>(span_count(p)), n = static_cast<size_t>(n_contacts);
    const bool rates = vel || acc, zero_ydd = rates && !acc;  // (vel alone: the twists' velocity half does not depend on ydd)
    const size_t per_state = nbod * 12 + (rates ? nbod * 12 + 2 * ns + (zero_ydd ? nv : 0) : 0);
    const Chunk c = budgeted_chunk(p, p->work, device, stream, 1024ull << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    Carver<T> w(wptr, c.chunk * per_state);
    T *Xa = w.take(c.chunk * nbod * 12), *V = rates ? w.take(c.chunk * nbod * 12) : nullptr;
    T *vs = rates ? w.take(c.chunk * ns) : nullptr, *as = rates ? w.take(c.chunk * ns) : nullptr, *zeros = zero_ydd ? w.take(c.chunk * nv) : nullptr;
    assert(w.taken == w.cap);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (zeros && (e = hipMemsetAsync(zeros, 0, c.chunk * nv * sizeof(T), hs)) != hipSuccess) return hip_err(e, "hipMemsetAsync");
    const std::array<T, 3> g = gravity3<T>(p);
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        if (int rc = poses_stage<T>(p, *t, q + b0 * nq, Xa, nb, stream)) return rc;
        if (rates)
            if (int rc = twists_stage<T>(p, *t, q + b0 * nq, qd + b0 * nv, zeros ? zeros : ydd + b0 * nv, V, vs, as, nb, device, stream)) return rc;
        e = launch_contact_points<T>(cs, Xa, V, static_cast<int>(nbod), g.data(), nb, pos ? pos + b0 * n * 3 : nullptr, vel ? vel + b0 * n * 3 : nullptr,
                                     acc ? acc + b0 * n * 3 : nullptr, hs);
        if (e != hipSuccess) return hip_err(e, "contact points launch");
    }
    return GRBDA_OK;
}

template <class T>
int contact_dynamics_args(const grbda_plan *p, const T *q, const T *qd, const T *tau, const T *f_ext, int n_contacts, const int *bodies,
                          const double *offsets, const T *a_des, double damping, const T *ydd, const T *lambda, const T *ydd_free, size_t B,
                          ContactSet<T> &cs)
{
    if (!q || !qd || !tau || !ydd || !lambda) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = contact_set<T>(p, n_contacts, bodies, offsets, "points", cs)) return rc;
    if (!std::isfinite(damping) || damping < 0) return set_err(GRBDA_EINVAL, "damping must be finite and not negative");
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const size_t bf = B * static_cast<size_t>(p->host.n_bodies) * 6 * sizeof(T), bc = B * static_cast<size_t>(n_contacts) * 3 * sizeof(T);
    const void *const in[5] = {q, qd, tau, f_ext, a_des}, *const out[3] = {ydd, lambda, ydd_free};
    const size_t in_bytes[5] = {bq, bv, bv, bf, bc}, out_bytes[3] = {bv, bc, bv};
    return no_overlap(in, in_bytes, out, out_bytes);
}
// Forward dynamics subject to "these points have this acceleration".  Per chunk, on one slab of p->work carved here for the whole pipeline
// (the inverse OSIM and the twists take their work arrays from it; the forward dynamics use the scratch slab and work_proj only):
//   1 ydd_free = FD(q, qd, tau, f_ext)          2 poses          3 twists at ydd_free          4 Linv = J H^-1 J^T of the contact frames
//   5 contact_solve_kernel: lambda and the wrench rows          6 ydd = FD(q, qd, tau, wrench rows)
template <class T>
int contact_dynamics(const grbda_plan *p, const T *q, const T *qd, const T *tau, const T *f_ext, int n_contacts, const int *bodies,
                     const double *offsets, const T *a_des, double damping, T *ydd, T *lambda, T *ydd_free, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<T> cs;
    if (int rc = contact_dynamics_args<T>(p, q, qd, tau, f_ext, n_contacts, bodies, offsets, a_des, damping, ydd, lambda, ydd_free, B, cs)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const OsimRoute<T> r = choose_osim<T>(p, n_contacts, bodies, offsets, false, nullptr, nullptr, nullptr);
    const size_t nq = p->host.nq, nv = p->host.nv, nbod = p->host.n_bodies, ns = static_cast<size_t>(span_count(p)), n = static_cast<size_t>(n_contacts);
    const size_t m6 = 6 * n;
    // ydd_free (when the caller does not keep it), poses, twists and their spanning rates, Linv, wrench rows, and the inverse OSIM's own
    const size_t per_state = (ydd_free ? 0 : nv) + nbod * 24 + 2 * ns + m6 * m6 + nbod * 6 + r.ws_per_state;
    const Chunk c = budgeted_chunk(p, p->work, device, stream, 1024ull << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    const std::array<T, 3> g = gravity3<T>(p);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        T *yf = ydd_free ? ydd_free + b0 * nv : w.take(nb * nv);
        T *Xa = w.take(nb * nbod * 12), *V = w.take(nb * nbod * 12), *vs = w.take(nb * ns), *as = w.take(nb * ns);
        T *Linv = w.take(nb * m6 * m6), *wrench = w.take(nb * nbod * 6);
        const T *qc = q + b0 * nq, *qdc = qd + b0 * nv, *tc = tau + b0 * nv, *fc = f_ext ? f_ext + b0 * nbod * 6 : nullptr;
        int rc;
        if ((rc = run<T>(p, false, qc, qdc, tc, fc, yf, nb, device, stream)) || (rc = poses_stage<T>(p, *t, qc, Xa, nb, stream)) ||
            (rc = twists_stage<T>(p, *t, qc, qdc, yf, V, vs, as, nb, device, stream)) ||
            (rc = osim_stage<T>(p, *t, r, cs, qc, Linv, nullptr, nb, device, stream, w)))
            return rc;
        hipError_t e = launch_contact_solve<T>(cs, Linv, Xa, V, a_des ? a_des + b0 * n * 3 : nullptr, fc, static_cast<int>(nbod), static_cast<T>(damping), g.data(), nb,
                                               lambda + b0 * n * 3, wrench, t->bad_count, t->n_cu, hs);
        if (e != hipSuccess) return hip_err(e, "contact solve launch");
        if ((rc = run<T>(p, false, qc, qdc, tc, wrench, ydd + b0 * nv, nb, device, stream))) return rc;
    }
    return GRBDA_OK;
}

// ---- sparse body wrenches (include/grbda_hip_wrench.h) --------------------------------------------------------------------------------
// The list as the wrench-carrying kernels take it, for n <= kMaxWrenches checked body indices: ONE filler for wrench_args and for the
// scheduled contacts (active_contacts), so that the canon bits cannot differ between them.
template <class T>
WrenchList<T> wrench_list(const grbda_plan *p, int n, const int *bodies, const T *wrench)
{
    WrenchList<T> W;
    W.n = n;
    W.w = wrench;
    W.canon = 0;
    for (int i = 0; i < kMaxWrenches; i++) {
        W.body[i] = i < n ? bodies[i] : -1;
        if (i < n) W.canon |= static_cast<unsigned>(p->host.lay64.bodies[bodies[i]].canon_axis & 3) << (2 * i);
    }
    return W;
}
// Everything grbda_aba_wrench_* / grbda_rnea_wrench_* refuse, on the host and before any device call; fills the kernels' list.
template <class T>
int wrench_args(const grbda_plan *p, const T *q, const T *qd, const T *x, int n, const int *bodies, const T *wrench, int frame, const T *out, size_t B,
                WrenchList<T> &W)
{
    if (!q || !qd || !x || !out) return set_err(GRBDA_EINVAL, "null argument");
    if (n < 0 || n > kMaxWrenches) return set_err(GRBDA_EINVAL, "0..16 body wrenches per call");
    if (frame != GRBDA_WRENCH_BODY && frame != GRBDA_WRENCH_WORLD) return set_err(GRBDA_EINVAL, "frame must be GRBDA_WRENCH_BODY or GRBDA_WRENCH_WORLD");
    if (n > 0 && (!bodies || !wrench)) return set_err(GRBDA_EINVAL, "null argument");
    for (int i = 0; i < n; i++)
        if (bodies[i] < 0 || bodies[i] >= p->host.n_bodies) return set_err(GRBDA_EINVAL, "body index out of range");
    W = wrench_list<T>(p, n, bodies, wrench);
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const void *const in[4] = {q, qd, x, n > 0 ? wrench : nullptr}, *const outs[1] = {out};
    const size_t in_bytes[4] = {bq, bv, bv, B * static_cast<size_t>(n) * 6 * sizeof(T)}, out_bytes[1] = {bv};
    return no_overlap(in, in_bytes, outs, out_bytes);
}
// The route of a call with a non-empty list: ROUTE_CHAIN on the one-wavefront program of the precision (the wrench-carrying kernels of
// chain_kernels.hip, unit 4) or ROUTE_INTERPRETER (a dense world-frame f_ext chunk through run()).  ONE definition, read by wrench_run and
// by grbda_wrench_kernel_name.  The chain route needs the plain program -- no differentials, no generic clusters -- a batch the launch
// rule gives to the one-wavefront kernels (latency mode carries no wrench hook), and every listed body among the link bodies, pair links
// and bases of the program: a rotor evaluated in closed form has no bias force of its own to take a wrench off.
template <class T>
Route wrench_route(const grbda_plan *p, bool rnea, int n_cu, size_t B, const WrenchList<T> &W)
{
    const HostPlan &h = p->host;
    const ChainSlot base = chain_slot(sizeof(T) == 8);
    const Route fallback{ROUTE_INTERPRETER, base, 0};
    if (h.projection_only) return fallback;
    const Route r = rnea ? choose_rnea<T>(p, n_cu, B, false) : choose_aba<T>(p, n_cu, B, false);
    if (r.path != ROUTE_CHAIN) return fallback;
    const ChainProgram &cp = h.chain[base];
    const RneaChainProgram &rp = h.rchain[base];
    if (!cp.ok || !cp.diffs.empty() || !cp.gens.empty() || cp.frees.size() > 1) return fallback;
    if (rnea && (!rp.ok || !rp.diffs.empty() || !rp.gens.empty())) return fallback;
    for (int i = 0; i < W.n; i++) {
        bool found = false;
        for (const ChainFree &f : cp.frees) found = found || f.body == W.body[i];
        for (const ChainLink &l : cp.links) found = found || l.body == W.body[i];
        for (const ChainPair &pr : cp.pairs) found = found || pr.body[0] == W.body[i] || pr.body[1] == W.body[i];
        if (!found) return fallback;
    }
    return {ROUTE_CHAIN, base, 0};
}
// Forward / inverse dynamics with the listed wrenches.  Chain route, body frame: one launch on the caller's arrays, no work memory.  Chain
// route, world frame: per chunk the poses of the listed bodies (body_list_stage), wrench_to_body_kernel, the launch.  Fallback: per chunk a
// zeroed dense chunk, (body frame: the listed poses,) wrench_scatter_kernel, run().  The chunks come off p->work (run() itself uses the scratch slab and work_proj only).
// wrench_stage: the call with its arguments checked, a list of n > 0, B > 0 and the device found -- what grbda_aba_wrench_* / grbda_rnea_wrench_*
// run, and the wrench-carrying forward dynamics of the scheduled contacts (gravity = false there: run()'s rule).
template <class T>
int wrench_stage(const grbda_plan *p, const DeviceTables *t, const WrenchList<T> &W, bool rnea, const T *q, const T *qd, const T *x, int n,
                 const int *bodies, const T *wrench, int frame, T *out, size_t B, int device, void *stream, bool gravity = true);
template <class T>
int wrench_run(const grbda_plan *p, bool rnea, const T *q, const T *qd, const T *x, int n, const int *bodies, const T *wrench, int frame, T *out,
               size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    WrenchList<T> W;
    if (int rc = wrench_args<T>(p, q, qd, x, n, bodies, wrench, frame, out, B, W)) return rc;
    if (n == 0) return run<T>(p, rnea, q, qd, x, nullptr, out, B, device, stream);
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    return wrench_stage<T>(p, t, W, rnea, q, qd, x, n, bodies, wrench, frame, out, B, device, stream);
}
template <class T>
int wrench_stage(const grbda_plan *p, const DeviceTables *t, const WrenchList<T> &W, bool rnea, const T *q, const T *qd, const T *x, int n,
                 const int *bodies, const T *wrench, int frame, T *out, size_t B, int device, void *stream, bool gravity)
{
    const Route r = wrench_route<T>(p, rnea, t->n_cu, B, W);
    const bool chain = r.path == ROUTE_CHAIN;
    const auto launch = [&](const WrenchList<T> &Wc, size_t b0, size_t nb) {
        const size_t nq = p->host.nq, nv = p->host.nv;
        return rnea ? run_rnea_chain<T>(p, *t, r, q + b0 * nq, qd + b0 * nv, x + b0 * nv, out + b0 * nv, nb, device, stream, gravity, &Wc)
                    : run_chain<T>(p, *t, r, q + b0 * nq, qd + b0 * nv, x + b0 * nv, out + b0 * nv, nb, device, stream, gravity, &Wc);
    };
    if (chain && frame == GRBDA_WRENCH_BODY) return launch(W, 0, B);
    const size_t nq = p->host.nq, nv = p->host.nv, nbod = p->host.n_bodies, n6 = static_cast<size_t>(n) * 6;
    const bool rotate = chain || frame == GRBDA_WRENCH_BODY;  // (the poses are computed only then)
    // the poses of the listed bodies alone, in list order (body_list_stage); a list past the walk's caps takes the full rows as well
    const BodyWalkHost H = rotate ? build_body_walk(p->host, layout_of(p->host, sizeof(T) == 4 ? 0 : 1), n, bodies) : BodyWalkHost{};
    const ListWork lw = rotate ? list_work(p, H, false, n) : ListWork{};
    const size_t per_state = lw.per_state() + (chain ? n6 : nbod * 6);
    const Chunk c = budgeted_chunk(p, p->work, device, stream, 1024ull << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        const auto m = lw.take(w, nb);
        T *Xa = m.out;
        WrenchList<T> Wc = W;
        Wc.w = wrench + b0 * n6;
        if (rotate)
            if (int rc = body_list_stage<T>(p, *t, H, false, q + b0 * nq, nullptr, nullptr, Xa, m.full, m.vs, m.as, nb, device, stream)) return rc;
        if (chain) {
            T *wb = w.take(nb * n6);
            hipError_t e = launch_wrench_to_body<T>(Wc, Xa, nb, wb, hs);
            if (e != hipSuccess) return hip_err(e, "wrench rotation launch");
            Wc.w = wb;
            if (int rc = launch(Wc, b0, nb)) return rc;
        } else {
            T *fext = w.take(nb * nbod * 6);
            hipError_t e = hipMemsetAsync(fext, 0, nb * nbod * 6 * sizeof(T), hs);
            if (e == hipSuccess) e = launch_wrench_scatter<T>(Wc, Xa, frame == GRBDA_WRENCH_BODY, static_cast<int>(nbod), nb, fext, hs);
            if (e != hipSuccess) return hip_err(e, "wrench scatter launch");
            if (int rc = run<T>(p, rnea, q + b0 * nq, qd + b0 * nv, x + b0 * nv, fext, out + b0 * nv, nb, device, stream, gravity)) return rc;
        }
    }
    return GRBDA_OK;
}
int wrench_host_f64(const grbda_plan *p, bool rnea, const double *q, const double *qd, const double *x, int n, const int *bodies, const double *wrench,
                    int frame, double *out, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    WrenchList<double> W;
    if (int rc = wrench_args<double>(p, q, qd, x, n, bodies, wrench, frame, out, B, W)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = st.in(qd, B * nv), *dx = st.in(x, B * nv);
    const double *dw = n > 0 ? st.in(wrench, B * static_cast<size_t>(n) * 6) : nullptr;
    double *dout = st.out(out, B * nv);
    return st.run([&] { return wrench_run<double>(p, rnea, dq, dqd, dx, n, bodies, dw, frame, dout, B, device, nullptr); });
}

// Everything grbda_contact_impulse_* refuses, on the host and before any device call.  qd_next may BE qd (equal pointers, as for
// grbda_integrate_*); any other overlap of an output with an input or with the other output is refused.
template <class T>
int contact_impulse_args(const grbda_plan *p, const T *q, const T *qd, int n_contacts, const int *bodies, const double *offsets, const T *v_des,
                         double restitution, double damping, const T *qd_next, const T *impulse, size_t B, ContactSet<T> &cs)
{
    if (!q || !qd || !qd_next || !impulse) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = contact_set<T>(p, n_contacts, bodies, offsets, "points", cs)) return rc;
    if (!std::isfinite(damping) || damping < 0) return set_err(GRBDA_EINVAL, "damping must be finite and not negative");
    if (!std::isfinite(restitution) || restitution < 0 || restitution > 1) return set_err(GRBDA_EINVAL, "restitution must lie in [0, 1]");
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const size_t bc = B * static_cast<size_t>(n_contacts) * 3 * sizeof(T);
    const void *const in[3] = {q, qd_next == qd ? nullptr : qd, v_des}, *const out[2] = {qd_next, impulse};  // (null entries are skipped)
    const size_t in_bytes[3] = {bq, bv, bc}, out_bytes[2] = {bv, bc};
    return no_overlap(in, in_bytes, out, out_bytes);
}
// The instant a contact closes: (J_w H^-1 J_w^T + mu I) Lambda = v_des - (1 + e) J_w qd, qd_next = qd + H^-1 J_w^T Lambda.  Per chunk, on one
// slab of p->work carved here for the whole pipeline (as contact_dynamics):
//   1 poses          2 twists at qd (the acceleration halves, computed at zeros, are not read)          3 Linv of the contact frames
//   4 impulse_solve_kernel: the impulses and the wrench rows          5 y1 = FD(q, 0, 0, wrench rows), y0 = FD(q, 0, 0, none): the forward
//   dynamics are affine in the wrenches, so y1 - y0 = H^-1 J_w^T Lambda with gravity cancelled          6 qd_next = qd + (y1 - y0)
// A chunk reads its rows of qd (stage 2) before stage 6 writes them, so qd_next == qd is safe.
template <class T>
int contact_impulse(const grbda_plan *p, const T *q, const T *qd, int n_contacts, const int *bodies, const double *offsets, const T *v_des,
                    double restitution, double damping, T *qd_next, T *impulse, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<T> cs;
    if (int rc = contact_impulse_args<T>(p, q, qd, n_contacts, bodies, offsets, v_des, restitution, damping, qd_next, impulse, B, cs)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const OsimRoute<T> r = choose_osim<T>(p, n_contacts, bodies, offsets, false, nullptr, nullptr, nullptr);
    const size_t nq = p->host.nq, nv = p->host.nv, nbod = p->host.n_bodies, ns = static_cast<size_t>(span_count(p)), n = static_cast<size_t>(n_contacts);
    const size_t m6 = 6 * n;
    // zeros, y1, y0, poses, twists and their spanning rates, Linv, wrench rows, and the inverse OSIM's own
    const size_t per_state = 3 * nv + nbod * 24 + 2 * ns + m6 * m6 + nbod * 6 + r.ws_per_state;
    const Chunk c = budgeted_chunk(p, p->work, device, stream, 1024ull << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    // (the zeros lead the slab at the chunk's full size: every pass finds them where this call cleared them)
    if (hipError_t e = hipMemsetAsync(wptr, 0, c.chunk * nv * sizeof(T), hs); e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        const T *zero = w.take(c.chunk * nv);
        T *y1 = w.take(nb * nv), *y0 = w.take(nb * nv);
        T *Xa = w.take(nb * nbod * 12), *V = w.take(nb * nbod * 12), *vs = w.take(nb * ns), *as = w.take(nb * ns);
        T *Linv = w.take(nb * m6 * m6), *wrench = w.take(nb * nbod * 6);
        const T *qc = q + b0 * nq, *qdc = qd + b0 * nv;
        int rc;
        if ((rc = poses_stage<T>(p, *t, qc, Xa, nb, stream)) || (rc = twists_stage<T>(p, *t, qc, qdc, zero, V, vs, as, nb, device, stream)) ||
            (rc = osim_stage<T>(p, *t, r, cs, qc, Linv, nullptr, nb, device, stream, w)))
            return rc;
        hipError_t e = launch_impulse_solve<T>(cs, Linv, Xa, V, v_des ? v_des + b0 * n * 3 : nullptr, static_cast<int>(nbod), static_cast<T>(damping),
                                               static_cast<T>(restitution), nb, impulse + b0 * n * 3, wrench, t->bad_count, t->n_cu, hs);
        if (e != hipSuccess) return hip_err(e, "impulse solve launch");
        if ((rc = run<T>(p, false, qc, zero, zero, wrench, y1, nb, device, stream)) || (rc = run<T>(p, false, qc, zero, zero, nullptr, y0, nb, device, stream)))
            return rc;
        if ((e = launch_impulse_finish<T>(qdc, y1, y0, nb * nv, qd_next + b0 * nv, hs)) != hipSuccess) return hip_err(e, "impulse finish launch");
    }
    return GRBDA_OK;
}

// ---- scheduled contacts: per-state active sets, the contact-aware step, the rollout (include/grbda_hip_contact_step.h) -----------------
// What every entry point of the header derives from its contact description once the arguments are checked: the set and the body-frame
// wrench list of the same bodies (both travel by value), the inverse-OSIM route contact_dynamics would take, and the walk of the listed
// poses and twists -- the list is `bodies` itself, slot c belongs to contact c.
template <class T>
struct ActiveContacts {
    ContactSet<T> cs;
    WrenchList<T> W;  // (w: set per chunk)
    const int *bodies;
    OsimRoute<T> r;
    BodyWalkHost H;
    ListWork lwp, lwt;  // the listed poses, the listed twists
    size_t n, m6;
    // scalars of work space per state of the stages every pipeline shares: poses, twists, Linv and the inverse OSIM's own, the wrench list
    size_t shared_per_state() const { return lwp.per_state() + lwt.per_state() + m6 * m6 + r.ws_per_state + n * 6; }
};
template <class T>
ActiveContacts<T> active_contacts(const grbda_plan *p, const ContactSet<T> &cs, const int *bodies, const double *offsets)
{
    ActiveContacts<T> A{};
    A.cs = cs;
    A.bodies = bodies;
    A.n = static_cast<size_t>(cs.n);
    A.m6 = 6 * A.n;
    A.W = wrench_list<T>(p, cs.n, bodies, static_cast<const T *>(nullptr));
    A.r = choose_osim<T>(p, cs.n, bodies, offsets, false, nullptr, nullptr, nullptr);
    A.H = build_body_walk(p->host, layout_of(p->host, sizeof(T) == 4 ? 0 : 1), cs.n, bodies);
    A.lwp = list_work(p, A.H, false, cs.n);
    A.lwt = list_work(p, A.H, true, cs.n);
    return A;
}
// the shared arrays of one chunk, carved in the order shared_per_state() counts them (the inverse OSIM takes its own from the carver)
template <class T>
struct ActiveWork {
    ListWork::Arrays<T> mp, mt;
    T *Linv, *wrench;
    ActiveWork(const ActiveContacts<T> &A, Carver<T> &w, size_t nb)
        : mp(A.lwp.take(w, nb)), mt(A.lwt.take(w, nb)), Linv(w.take(nb * A.m6 * A.m6)), wrench(w.take(nb * A.n * 6))
    {
    }
};
// The stages below run nb states of one chunk: arguments checked, device found, every pointer at the chunk's first state.
// What depends on q alone: the listed poses and the inverse OSIM of all n contact frames (contact_step uses one pair for both solves).
template <class T>
int active_frames_stage(const grbda_plan *p, const DeviceTables &t, const ActiveContacts<T> &A, const ActiveWork<T> &k, const T *q, size_t nb,
                        int device, void *stream, Carver<T> &w)
{
    if (int rc = body_list_stage<T>(p, t, A.H, false, q, nullptr, nullptr, k.mp.out, k.mp.full, k.mp.vs, k.mp.as, nb, device, stream)) return rc;
    return osim_stage<T>(p, t, A.r, A.cs, q, k.Linv, nullptr, nb, device, stream, w);
}
//   1 ydd_free = FD(q, qd, tau)          2 listed twists at ydd_free          3 contact_active_solve_kernel: lambda and the body-frame wrench list
//   4 ydd = FD(q, qd, tau, wrench list), the sparse-wrench call on its own routes          5 the states with an empty set keep ydd_free
template <class T>
int active_dynamics_stage(const grbda_plan *p, const DeviceTables &t, const ActiveContacts<T> &A, const ActiveWork<T> &k, const T *q, const T *qd,
                          const T *tau, const int32_t *active, const T *a_des, double kd, double damping, T *ydd, T *lambda, T *yf, size_t nb,
                          int device, void *stream)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const std::array<T, 3> g = gravity3<T>(p);
    int rc;
    if ((rc = run<T>(p, false, q, qd, tau, nullptr, yf, nb, device, stream)) ||
        (rc = body_list_stage<T>(p, t, A.H, true, q, qd, yf, k.mt.out, k.mt.full, k.mt.vs, k.mt.as, nb, device, stream)))
        return rc;
    hipError_t e = launch_contact_active_solve<T>(false, A.cs, k.Linv, k.mp.out, k.mt.out, a_des, active, static_cast<T>(damping), static_cast<T>(kd),
                                                  g.data(), nb, lambda, k.wrench, t.bad_count, t.n_cu, hs);
    if (e != hipSuccess) return hip_err(e, "contact solve launch");
    WrenchList<T> W = A.W;
    W.w = k.wrench;
    if ((rc = wrench_stage<T>(p, &t, W, false, q, qd, tau, W.n, A.bodies, k.wrench, GRBDA_WRENCH_BODY, ydd, nb, device, stream))) return rc;
    e = launch_free_states_copy<T>(active, W.n, yf, p->host.nv, nb, ydd, hs);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "free states launch");
}
//   1 listed twists at (q, qd, 0)          2 contact_active_solve_kernel, velocity level: the impulses and the body-frame wrench list
//   3 y1 = FD(q, 0, 0, wrench list), y0 = FD(q, 0, 0), both without gravity: at rest each term of y0, and of y1 in a state with an empty
//     set, is exactly zero          4 qd_next = qd + (y1 - y0) (impulse_finish_kernel; qd_next may be qd)
template <class T>
int active_impulse_stage(const grbda_plan *p, const DeviceTables &t, const ActiveContacts<T> &A, const ActiveWork<T> &k, const T *q, const T *qd,
                         const int32_t *active, const T *v_des, double restitution, double damping, T *qd_next, T *impulse, const T *zero, T *y1,
                         T *y0, size_t nb, int device, void *stream)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const T g0[3] = {0, 0, 0};
    if (int rc = body_list_stage<T>(p, t, A.H, true, q, qd, zero, k.mt.out, k.mt.full, k.mt.vs, k.mt.as, nb, device, stream)) return rc;
    hipError_t e = launch_contact_active_solve<T>(true, A.cs, k.Linv, k.mp.out, k.mt.out, v_des, active, static_cast<T>(damping),
                                                  T(1) + static_cast<T>(restitution), g0, nb, impulse, k.wrench, t.bad_count, t.n_cu, hs);
    if (e != hipSuccess) return hip_err(e, "impulse solve launch");
    WrenchList<T> W = A.W;
    W.w = k.wrench;
    int rc;
    if ((rc = wrench_stage<T>(p, &t, W, false, q, zero, zero, W.n, A.bodies, k.wrench, GRBDA_WRENCH_BODY, y1, nb, device, stream, false)) ||
        (rc = run<T>(p, false, q, zero, zero, nullptr, y0, nb, device, stream, false)))
        return rc;
    e = launch_impulse_finish<T>(qd, y1, y0, nb * static_cast<size_t>(p->host.nv), qd_next, hs);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "impulse finish launch");
}
// the rules the entry points share: the contact description, then the gains
template <class T>
int active_set_args(const grbda_plan *p, int n_contacts, const int *bodies, const double *offsets, const double *kd, const double *restitution,
                    double damping, ContactSet<T> &cs)
{
    if (int rc = contact_set<T>(p, n_contacts, bodies, offsets, "points", cs)) return rc;
    if (kd && (!std::isfinite(*kd) || *kd < 0)) return set_err(GRBDA_EINVAL, "kd must be finite and not negative");
    if (!std::isfinite(damping) || damping < 0) return set_err(GRBDA_EINVAL, "damping must be finite and not negative");
    if (restitution && (!std::isfinite(*restitution) || *restitution < 0 || *restitution > 1))
        return set_err(GRBDA_EINVAL, "restitution must lie in [0, 1]");
    return GRBDA_OK;
}
// the work pool of the scheduled contacts: chunk and slab for `per_state` scalars per state
template <class T>
int active_pool(const grbda_plan *p, size_t per_state, size_t B, int device, void *stream, Chunk &c, void **wptr)
{
    c = budgeted_chunk(p, p->work_contact, device, stream, 1024ull << 20, per_state * sizeof(T), B);
    return ensure_work(p, p->work_contact, device, stream, c.bytes, wptr);
}

template <class T>
int contact_dynamics_active_args(const grbda_plan *p, const T *q, const T *qd, const T *tau, int n_contacts, const int *bodies, const double *offsets,
                                 const int32_t *active, const T *a_des, double kd, double damping, const T *ydd, const T *lambda, const T *ydd_free,
                                 size_t B, ContactSet<T> &cs)
{
    if (!q || !qd || !tau || !active || !ydd || !lambda) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = active_set_args<T>(p, n_contacts, bodies, offsets, &kd, nullptr, damping, cs)) return rc;
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const size_t bc = B * static_cast<size_t>(n_contacts) * 3 * sizeof(T);
    const void *const in[5] = {q, qd, tau, active, a_des}, *const out[3] = {ydd, lambda, ydd_free};
    const size_t in_bytes[5] = {bq, bv, bv, B * sizeof(int32_t), bc}, out_bytes[3] = {bv, bc, bv};
    return no_overlap(in, in_bytes, out, out_bytes);
}
template <class T>
int contact_dynamics_active(const grbda_plan *p, const T *q, const T *qd, const T *tau, int n_contacts, const int *bodies, const double *offsets,
                            const int32_t *active, const T *a_des, double kd, double damping, T *ydd, T *lambda, T *ydd_free, size_t B, int device,
                            void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<T> cs;
    if (int rc = contact_dynamics_active_args<T>(p, q, qd, tau, n_contacts, bodies, offsets, active, a_des, kd, damping, ydd, lambda, ydd_free, B, cs))
        return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const ActiveContacts<T> A = active_contacts<T>(p, cs, bodies, offsets);
    const size_t nq = p->host.nq, nv = p->host.nv, n = A.n;
    const size_t per_state = (ydd_free ? 0 : nv) + A.shared_per_state();
    Chunk c;
    void *wptr = nullptr;
    if (int rc = active_pool<T>(p, per_state, B, device, stream, c, &wptr)) return rc;
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        T *yf = ydd_free ? ydd_free + b0 * nv : w.take(nb * nv);
        const ActiveWork<T> k(A, w, nb);
        int rc;
        if ((rc = active_frames_stage<T>(p, *t, A, k, q + b0 * nq, nb, device, stream, w)) ||
            (rc = active_dynamics_stage<T>(p, *t, A, k, q + b0 * nq, qd + b0 * nv, tau + b0 * nv, active + b0, a_des ? a_des + b0 * n * 3 : nullptr, kd,
                                           damping, ydd + b0 * nv, lambda + b0 * n * 3, yf, nb, device, stream)))
            return rc;
    }
    return GRBDA_OK;
}

template <class T>
int contact_impulse_active_args(const grbda_plan *p, const T *q, const T *qd, int n_contacts, const int *bodies, const double *offsets,
                                const int32_t *active, const T *v_des, double restitution, double damping, const T *qd_next, const T *impulse,
                                size_t B, ContactSet<T> &cs)
{
    if (!q || !qd || !active || !qd_next || !impulse) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = active_set_args<T>(p, n_contacts, bodies, offsets, nullptr, &restitution, damping, cs)) return rc;
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const size_t bc = B * static_cast<size_t>(n_contacts) * 3 * sizeof(T);
    const void *const in[4] = {q, qd_next == qd ? nullptr : qd, active, v_des}, *const out[2] = {qd_next, impulse};  // (null entries are skipped)
    const size_t in_bytes[4] = {bq, bv, B * sizeof(int32_t), bc}, out_bytes[2] = {bv, bc};
    return no_overlap(in, in_bytes, out, out_bytes);
}
// (a chunk reads its rows of qd -- the twists -- before its last stage writes them, so qd_next == qd is safe, as for contact_impulse)
template <class T>
int contact_impulse_active(const grbda_plan *p, const T *q, const T *qd, int n_contacts, const int *bodies, const double *offsets,
                           const int32_t *active, const T *v_des, double restitution, double damping, T *qd_next, T *impulse, size_t B, int device,
                           void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<T> cs;
    if (int rc = contact_impulse_active_args<T>(p, q, qd, n_contacts, bodies, offsets, active, v_des, restitution, damping, qd_next, impulse, B, cs))
        return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const ActiveContacts<T> A = active_contacts<T>(p, cs, bodies, offsets);
    const size_t nq = p->host.nq, nv = p->host.nv, n = A.n;
    const size_t per_state = 3 * nv + A.shared_per_state();  // zeros, y1, y0
    Chunk c;
    void *wptr = nullptr;
    if (int rc = active_pool<T>(p, per_state, B, device, stream, c, &wptr)) return rc;
    // (the zeros lead the slab at the chunk's full size: every pass finds them where this call cleared them)
    if (hipError_t e = hipMemsetAsync(wptr, 0, c.chunk * nv * sizeof(T), static_cast<hipStream_t>(stream)); e != hipSuccess)
        return hip_err(e, "hipMemsetAsync");
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        const T *zero = w.take(c.chunk * nv);
        T *y1 = w.take(nb * nv), *y0 = w.take(nb * nv);
        const ActiveWork<T> k(A, w, nb);
        int rc;
        if ((rc = active_frames_stage<T>(p, *t, A, k, q + b0 * nq, nb, device, stream, w)) ||
            (rc = active_impulse_stage<T>(p, *t, A, k, q + b0 * nq, qd + b0 * nv, active + b0, v_des ? v_des + b0 * n * 3 : nullptr, restitution, damping,
                                          qd_next + b0 * nv, impulse + b0 * n * 3, zero, y1, y0, nb, device, stream)))
            return rc;
    }
    return GRBDA_OK;
}

// Everything grbda_contact_step_* refuses: its own rules, then the integrator's (the aliasing of q_next / qd_next and what grbda_step_*
// does not cover), then the overlaps of the arrays the integrator does not know.
template <class T>
int contact_step_args(const grbda_plan *p, const T *q, const T *qd, const T *tau, int n_contacts, const int *bodies, const double *offsets,
                      const int32_t *active, const int32_t *prev_active, double kd, double restitution, double damping, double dt, const T *ydd,
                      const T *lambda, const T *impulse, const T *q_next, const T *qd_next, const int32_t *ok, size_t B, ContactSet<T> &cs)
{
    if (!q || !qd || !tau || !active || !ydd || !lambda || !q_next || !qd_next) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = active_set_args<T>(p, n_contacts, bodies, offsets, &kd, &restitution, damping, cs)) return rc;
    if (impulse && !prev_active) return set_err(GRBDA_EINVAL, "impulse needs prev_active: without it no impulse stage runs");
    if (int rc = integrate_args<T>(p, q, qd, ydd, dt, q_next, qd_next, kStepMaxIter, kStepTol, B)) return rc;
    const size_t bq = B * static_cast<size_t>(p->host.nq) * sizeof(T), bv = B * static_cast<size_t>(p->host.nv) * sizeof(T);
    const size_t bc = B * static_cast<size_t>(n_contacts) * 3 * sizeof(T), bi = B * sizeof(int32_t);
    // (q_next == q and qd_next == qd passed the integrator's rule: the pair then counts once, as an output)
    const void *const in[5] = {q_next == q ? nullptr : q, qd_next == qd ? nullptr : qd, tau, active, prev_active};
    const void *const out[6] = {ydd, lambda, impulse, q_next, qd_next, ok};
    const size_t in_bytes[5] = {bq, bv, bv, bi, bi}, out_bytes[6] = {bv, bc, bc, bq, bv, bi};
    return no_overlap(in, in_bytes, out, out_bytes);
}
// scalars of the work pool per state of a step: the shared stages, and for the impulse stage the zeros, y1, y0, the impact masks (one cell
// each) and the impulses nobody keeps.  grbda_contact_rollout_* counts the same, so that its steps chunk as single steps do.
template <class T>
size_t contact_step_per_state(const grbda_plan *p, const ActiveContacts<T> &A)
{
    return A.shared_per_state() + 3 * static_cast<size_t>(p->host.nv) + 1 + 2 * A.n * 3;
}
// One step on a checked call (B > 0, device found, the pool's slab and chunk in hand): per chunk the poses and Linv once, the impulse stage
// when prev_active is given (it leaves qd+ in qd_next), the dynamics at qd+; then the integrator over the batch.  lambda == nullptr: the
// pool keeps the forces (the rollout without lambda_traj).
template <class T>
int contact_step_run(const grbda_plan *p, const DeviceTables &t, const ActiveContacts<T> &A, const Chunk &c, void *wptr, const T *q, const T *qd,
                     const T *tau, const int32_t *active, const int32_t *prev_active, double kd, double restitution, double damping, double dt, T *ydd,
                     T *lambda, T *impulse, T *q_next, T *qd_next, int32_t *ok, bool ok_and, size_t B, int device, void *stream)
{
    const size_t nq = p->host.nq, nv = p->host.nv, n = A.n, per_state = contact_step_per_state<T>(p, A);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    static_assert(sizeof(T) >= sizeof(int32_t), "an impact mask takes one cell of the pool");
    if (prev_active)
        if (hipError_t e = hipMemsetAsync(wptr, 0, c.chunk * nv * sizeof(T), hs); e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    const T *qd_plus = prev_active ? qd_next : qd;
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        Carver<T> w(wptr, c.chunk * per_state);
        const T *zero = w.take(c.chunk * nv);
        T *y1 = w.take(nb * nv), *y0 = w.take(nb * nv);
        int32_t *impact = reinterpret_cast<int32_t *>(w.take(nb));
        T *imp = w.take(nb * n * 3), *lam = w.take(nb * n * 3);
        const ActiveWork<T> k(A, w, nb);
        const T *qc = q + b0 * nq;
        int rc;
        if ((rc = active_frames_stage<T>(p, t, A, k, qc, nb, device, stream, w))) return rc;
        if (prev_active) {
            if (hipError_t e = launch_impact_mask(active + b0, prev_active + b0, static_cast<int>(n), nb, impact, hs); e != hipSuccess)
                return hip_err(e, "impact mask launch");
            if ((rc = active_impulse_stage<T>(p, t, A, k, qc, qd + b0 * nv, impact, static_cast<const T *>(nullptr), restitution, damping,
                                              qd_next + b0 * nv, impulse ? impulse + b0 * n * 3 : imp, zero, y1, y0, nb, device, stream)))
                return rc;
        }
        // (ydd_free goes where y1 was: the impulse stage is done with it)
        if ((rc = active_dynamics_stage<T>(p, t, A, k, qc, qd_plus + b0 * nv, tau + b0 * nv, active + b0, static_cast<const T *>(nullptr), kd, damping,
                                           ydd + b0 * nv, lambda ? lambda + b0 * n * 3 : lam, y1, nb, device, stream)))
            return rc;
    }
    return integrate_launch<T>(p, q, qd_plus, ydd, dt, q_next, qd_next, ok, kStepMaxIter, kStepTol, B, device, stream, ok_and);
}
template <class T>
int contact_step(const grbda_plan *p, const T *q, const T *qd, const T *tau, int n_contacts, const int *bodies, const double *offsets,
                 const int32_t *active, const int32_t *prev_active, double kd, double restitution, double damping, double dt, T *ydd, T *lambda,
                 T *impulse, T *q_next, T *qd_next, int32_t *ok, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<T> cs;
    if (int rc = contact_step_args<T>(p, q, qd, tau, n_contacts, bodies, offsets, active, prev_active, kd, restitution, damping, dt, ydd, lambda, impulse,
                                      q_next, qd_next, ok, B, cs))
        return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const ActiveContacts<T> A = active_contacts<T>(p, cs, bodies, offsets);
    Chunk c;
    void *wptr = nullptr;
    if (int rc = active_pool<T>(p, contact_step_per_state<T>(p, A), B, device, stream, c, &wptr)) return rc;
    return contact_step_run<T>(p, *t, A, c, wptr, q, qd, tau, active, prev_active, kd, restitution, damping, dt, ydd, lambda, impulse, q_next, qd_next, ok,
                               false, B, device, stream);
}
// T steps in place; every state (and every step's forces) copied to the trajectory arrays on the same stream
template <class T>
int contact_rollout(const grbda_plan *p, T *q, T *qd, const T *tau, int tau_steps, int n_contacts, const int *bodies, const double *offsets,
                    const int32_t *active, int active_steps, const int32_t *active_prev, int with_impulses, double kd, double restitution,
                    double damping, double dt, int n_steps, T *ydd_work, T *q_traj, T *qd_traj, T *lambda_traj, int32_t *ok, size_t B, int device,
                    void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !qd || !tau || !active || !ydd_work) return set_err(GRBDA_EINVAL, "null argument");
    ContactSet<T> cs;
    if (int rc = active_set_args<T>(p, n_contacts, bodies, offsets, &kd, &restitution, damping, cs)) return rc;
    if (n_steps < 0) return set_err(GRBDA_EINVAL, "T is negative");
    if (tau_steps != 1 && tau_steps != n_steps) return set_err(GRBDA_EINVAL, "tau_steps must be 1 or T");
    if (active_steps != 1 && active_steps != n_steps) return set_err(GRBDA_EINVAL, "active_steps must be 1 or T");
    if (int rc = integrate_args<T>(p, q, qd, ydd_work, dt, q, qd, kStepMaxIter, kStepTol, B)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, n = static_cast<size_t>(n_contacts), steps = static_cast<size_t>(n_steps);
    const size_t bq = B * nq * sizeof(T), bv = B * nv * sizeof(T), bc = B * n * 3 * sizeof(T), bi = B * sizeof(int32_t);
    // (tau[T][B][nv], active[T][B]: every step's block stays clear of what the steps write)
    const void *const in[3] = {tau, active, with_impulses ? active_prev : nullptr};
    const void *const out[7] = {q, qd, ydd_work, q_traj, qd_traj, lambda_traj, ok};
    const size_t in_bytes[3] = {static_cast<size_t>(tau_steps) * bv, static_cast<size_t>(active_steps) * bi, bi};
    const size_t out_bytes[7] = {bq, bv, bv, steps * bq, steps * bv, steps * bc, bi};
    if (int rc = no_overlap(in, in_bytes, out, out_bytes)) return rc;
    if (B == 0 || n_steps == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const ActiveContacts<T> A = active_contacts<T>(p, cs, bodies, offsets);
    Chunk c;
    void *wptr = nullptr;
    if (int rc = active_pool<T>(p, contact_step_per_state<T>(p, A), B, device, stream, c, &wptr)) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    for (int s = 0; s < n_steps; s++) {
        const size_t at = static_cast<size_t>(s);
        const int32_t *as = active + (active_steps > 1 ? at * B : 0);
        // (a NULL active_prev stands for active[0]; a held mask is its own predecessor)
        const int32_t *prev = !with_impulses ? nullptr : s == 0 ? (active_prev ? active_prev : active) : active + (active_steps > 1 ? (at - 1) * B : 0);
        // (ok: the first step writes the flags, the later ones AND theirs into them)
        if (int rc = contact_step_run<T>(p, *t, A, c, wptr, q, qd, tau + (tau_steps > 1 ? at * B * nv : 0), as, prev, kd, restitution, damping, dt, ydd_work,
                                         lambda_traj ? lambda_traj + at * B * n * 3 : nullptr, static_cast<T *>(nullptr), q, qd, ok, s > 0, B, device,
                                         stream))
            return rc;
        hipError_t e;
        if (q_traj && (e = hipMemcpyAsync(q_traj + at * B * nq, q, bq, hipMemcpyDeviceToDevice, hs)) != hipSuccess) return hip_err(e, "hipMemcpyAsync");
        if (qd_traj && (e = hipMemcpyAsync(qd_traj + at * B * nv, qd, bv, hipMemcpyDeviceToDevice, hs)) != hipSuccess) return hip_err(e, "hipMemcpyAsync");
    }
    return GRBDA_OK;
}

// ---- derived quantities: expanded batches over the two kernels (include/grbda_hip.h) ---------------------
// (DM_ID_DQD, DM_ID_DQ: the same difference batches as DM_DQD, DM_DQ over the INVERSE dynamics, `tau` holding ydd -- grbda_rnea_derivatives_*)
enum DerivedMode { DM_BIAS = 0, DM_MASS = 1, DM_DTAU = 2, DM_DQD = 3, DM_DQ = 4, DM_ID_DQD = 5, DM_ID_DQ = 6 };
__host__ __device__ inline bool dm_steps_q(int mode) { return mode == DM_DQ || mode == DM_ID_DQ; }
__host__ __device__ inline bool dm_steps_qd(int mode) { return mode == DM_DQD || mode == DM_ID_DQD; }

// row (b, j) of the expanded batch: state b with the j-th unit vector (or none) applied
// position col of state q0 after the tangent step `d` along velocity coordinate k (testHelpers.hpp:50-112)
template <class T>
__device__ T perturbed_position(const T *q0, int col, const int32_t *map, int k, T d)
{
    const int kind = map[3 * k], qi = map[3 * k + 1], a = map[3 * k + 2];
    const T x = q0[col];
    if (kind == 0) return col == qi ? x + d : x;
    if (kind == 1) {  // quat (scalar first, positions qi+3 .. qi+6) += quat x (0, d e_a) / 2
        if (col < qi + 3 || col > qi + 6) return x;
        const T w = q0[qi + 3], v[3] = {q0[qi + 4], q0[qi + 5], q0[qi + 6]};
        const int i = col - qi - 3;
        if (i == 0) return x - T(0.5) * d * v[a];
        const int j = i - 1;  // vector component: w e_a + v x e_a
        T p = j == a ? w : T(0);
        if (j == (a + 1) % 3) p += v[(a + 2) % 3];   // (v x e_a)_{a+1} = v_{a+2}
        if (j == (a + 2) % 3) p -= v[(a + 1) % 3];   // (v x e_a)_{a+2} = -v_{a+1}
        return x + T(0.5) * d * p;
    }
    if (kind == 2) {  // pos += R(quat)^T d e_a: component i gets R[a][i] (OrientationTools.h:251-269)
        if (col < qi || col > qi + 2) return x;
        const T e0 = q0[qi + 3], e1 = q0[qi + 4], e2 = q0[qi + 5], e3 = q0[qi + 6];
        const T M[9] = {1 - 2 * (e2 * e2 + e3 * e3), 2 * (e1 * e2 - e0 * e3), 2 * (e1 * e3 + e0 * e2),
                        2 * (e1 * e2 + e0 * e3), 1 - 2 * (e1 * e1 + e3 * e3), 2 * (e2 * e3 - e0 * e1),
                        2 * (e1 * e3 - e0 * e2), 2 * (e2 * e3 + e0 * e1), 1 - 2 * (e1 * e1 + e2 * e2)};
        const int i = col - qi;
        return x + d * M[3 * i + a];  // R = M^T: R[a][i] = M[i][a]
    }
    return x;
}

template <class T>
__global__ void expand_kernel(int mode, const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ tau,
                              int nq, int nv, int R, size_t nb, T *__restrict__ qx, T *__restrict__ qdx,
                              T *__restrict__ xx, const int32_t *__restrict__ dq_map, T step)
{
    const size_t rows = nb * (size_t)R;
    const int w = nq + 2 * nv;
    const size_t total = rows * (size_t)w;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / w;
        const int col = (int)(i % w);
        const size_t b = row / R;
        const int j = (int)(row % R);
        if (col < nq) {
            qx[row * nq + col] = dm_steps_q(mode) ? perturbed_position(q + b * nq, col, dq_map, j >> 1, (j & 1) ? -step : step)
                                               : q[b * nq + col];
        } else if (col < nq + nv) {
            const int k = col - nq;
            T v = 0;
            if (mode == DM_BIAS || dm_steps_q(mode)) v = qd[b * nv + k];
            else if (dm_steps_qd(mode)) v = qd[b * nv + k] + ((j >> 1) == k ? ((j & 1) ? T(-1) : T(1)) : T(0));
            qdx[row * nv + k] = v;
        } else {
            const int k = col - nq - nv;
            T v = 0;
            if (mode == DM_MASS || mode == DM_DTAU) v = (j == k) ? T(1) : T(0);
            else if (dm_steps_qd(mode) || dm_steps_q(mode)) v = tau[b * nv + k];
            xx[row * nv + k] = v;
        }
    }
}

template <class A, class Bt>
__global__ void convert_kernel(const A *__restrict__ src, Bt *__restrict__ dst, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = static_cast<Bt>(src[i]);
}

// out[b][i][j] from the kernel results r[(b, j)][i]
template <class T>
__global__ void combine_kernel(int mode, const T *__restrict__ r, int nv, int R, size_t nb, T *__restrict__ out,
                               T step)
{
    const size_t total = nb * (size_t)nv * nv;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t b = t / ((size_t)nv * nv);
        const int i = (int)((t / nv) % nv), j = (int)(t % nv);
        const T *rb = r + b * (size_t)R * nv;
        T v;
        if (dm_steps_qd(mode) || dm_steps_q(mode))
            v = (rb[(size_t)(2 * j) * nv + i] - rb[(size_t)(2 * j + 1) * nv + i]) / (T(2) * (dm_steps_q(mode) ? step : T(1)));
        else v = rb[(size_t)j * nv + i] - rb[(size_t)nv * nv + i];
        out[t] = v;
    }
}

// ---- derivative routes: which stage computes each output of the derivative entry points -- ONE definition (choose_derivs), asked once per
// call, as choose_aba / Route.  The analytic recursion covers explicit clusters up to nv = 64, the manifold route models with implicit
// clusters through the spanning tree (manifold_kernels.hip); everything else is a difference batch of derived().
inline bool analytic_covers(const grbda_plan *p)
{
    return p->host.deriv.ok && p->host.crba.ok && !p->opt.no_analytic && !p->opt.no_crba && p->host.nv <= kWave;
}
inline bool manifold_covers(const grbda_plan *p)
{
    return p->span && !p->opt.no_manifold && !p->opt.no_analytic && p->host.nv <= kWave && p->span->host.nv <= kWave &&
           p->host.deriv.related.size() == static_cast<size_t>(p->host.nv);
}
// BY_MINV: H^-1 = W^T W from the articulated-body quantities (minv_kernels.hip); BY_FACTOR: dense factorisation of H (deriv_kernels.hip);
// BY_MANIFOLD: the projected spanning-tree matrices and the same factorisation; BY_DIFFERENCES: a batch of derived()
enum DerivPath { NOT_WANTED, BY_MINV, BY_FACTOR, BY_MANIFOLD, BY_DIFFERENCES };
enum MassPath { MASS_MANIFOLD, MASS_CRBA, MASS_UNIT_BATCH };
struct DerivRoute {
    DerivPath dq, dqd, dtau;
    bool solve_f64;  // BY_FACTOR: fp32 matrices factorised in fp64 (GRBDA_SOLVE_F64)
    MassPath mass;   // (whatever else is wanted)
};
// `minv_tables`: DeviceTables::minv_bodies and minv_coltab are both on the device
DerivRoute choose_derivs(const grbda_plan *p, bool minv_tables, size_t elem, bool dq, bool dqd, bool dtau)
{
    const bool manifold = manifold_covers(p);
    // (H = G^T H_s G through the spanning tree is asked first, then one CRBA launch, instead of nv + 1 inverse dynamics)
    const MassPath mass = p->opt.no_crba ? MASS_UNIT_BATCH : (manifold ? MASS_MANIFOLD : (p->host.crba.ok ? MASS_CRBA : MASS_UNIT_BATCH));
    DerivPath state = BY_DIFFERENCES, tau = BY_DIFFERENCES;  // d/dq and d/dqd share a path
    bool wide = false;
    if (analytic_covers(p)) {
        const MinvProgram &mv = p->host.deriv.minv;
        wide = elem == 4 && p->opt.solve_f64;
        // (GRBDA_NO_MINV=1 keeps the factorisation route: A/B runs)
        const bool minv = mv.ok && minv_tables && !wide && !p->opt.no_minv && minv_solve_lds_bytes(p->host.nv, (dq ? 1 : 0) + (dqd ? 1 : 0), mv.n_entries, elem) <= 160u * 1024u;
        state = tau = minv ? BY_MINV : BY_FACTOR;
    } else if (manifold) {
        // plans with big clusters (beyond the structured limits): d/dtau by the manifold route, d/dq and d/dqd by difference batches
        tau = BY_MANIFOLD;
        state = p->host.big_clusters ? BY_DIFFERENCES : BY_MANIFOLD;
    }
    return {dq ? state : NOT_WANTED, dqd ? state : NOT_WANTED, dtau ? tau : NOT_WANTED, wide, mass};
}

// ---- launch sites shared by the derivative pipelines -----------------------------------------------------------------------------------
// a persistent grid: no more workgroups than the LDS of a CU holds at once (JVRC-1's unpack: 12 of its 12.4 KB blocks, not 16) or than units of work
inline size_t persistent_grid(int n_cu, size_t cap, size_t lds_bytes, size_t units)
{
    return std::min(static_cast<size_t>(n_cu) * std::min(cap, lds_workgroups_per_cu(lds_bytes + 512)), units);
}
// whole groups of `il` states in one call of fn(b0, nb, il) (interleaved layouts), the tail of the batch in a second, state-major
template <class Fn>
int for_groups_then_tail(size_t B, int il, Fn fn)
{
    const size_t Bg = il > 1 ? B / il * il : 0;
    if (int rc = Bg ? fn(static_cast<size_t>(0), Bg, il) : GRBDA_OK) return rc;
    return B > Bg ? fn(Bg, B - Bg, 1) : GRBDA_OK;
}
// The batched SPD solve on H in packed rows: H^-1 and up to two solved right-hand sides.  One wavefront per state, as many as the LDS of a CU holds;
// `mfma`: the matrix-core kernel, workgroups of four wavefronts on groups of kDerivGroup states.  `wide`: fp32 in fp64.  `il`: the plain fp32 solve only.
template <class T>
hipError_t spd_solve_stage(const DeviceTables &t, const T *H, const T *r1, const T *r2, T *Hinv, T *x1, T *x2, int nv, int n_rhs, size_t nb,
                           bool wide, bool mfma, int il, hipStream_t hs)
{
    const size_t lds = spd_solve_lds_bytes(nv, wide ? 8 : sizeof(T), n_rhs);
    const size_t cap = mfma ? static_cast<size_t>(spd_mfma_workgroups_per_cu(nv)) : 16;
    const size_t per_cu = std::max<size_t>(1, std::min(lds ? lds_workgroups_per_cu(lds) : 16, cap));
    const size_t units = mfma ? (nb + kDerivGroup - 1) / kDerivGroup : nb;
    const int grid = static_cast<int>(std::min(static_cast<size_t>(t.n_cu) * per_cu, units));
    if constexpr (sizeof(T) == 8) return launch_spd_solve<double, double>(H, 1, r1, r2, Hinv, x1, x2, t.deriv_related, nv, nb, grid, hs, 1);
    else if (wide) return launch_spd_solve<float, double>(H, 1, r1, r2, Hinv, x1, x2, t.deriv_related, nv, nb, grid, hs, 1);
    else return launch_spd_solve<float, float>(H, 1, r1, r2, Hinv, x1, x2, t.deriv_related, nv, nb, grid, hs, il);
}
// The spanning-tree stage of a chunk: the spanning state and the coupling rows of the constraint (q_s, qd_s, qdd_s, cpl), the spanning
// tree's inverse dynamics into x_s, and its derivative recursion into (Aq, Av, Hs) where Hs is given.  Without x_s (H only) the
// recursion runs at zero velocity and acceleration -- its H does not depend on them -- and nothing but q_s comes from the constraint.
template <class T>
int spanning_stage(const grbda_plan *p, const DeviceTables &t, const DeviceTables &ts, const DevPlan<T> &d, const DevPlan<T> &ds, int want_d, const T *q, const T *qd,
                   const T *ydd, const T *f_ext, T *q_s, T *qd_s, T *qdd_s, T *cpl, T *x_s, T *Aq, T *Av, T *Hs, size_t nb, size_t chunk, int device, void *stream)
{
    const grbda_plan *sp = p->span;
    const size_t nv_s = sp->host.nv;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (!x_s && (e = hipMemsetAsync(qd_s, 0, 2 * chunk * nv_s * sizeof(T), hs)) != hipSuccess) return hip_err(e, "hipMemsetAsync");
    e = launch_manifold_constraint<T>(d, p->host.n_clusters, t.span_q, t.span_v, t.crow, sp->host.nq, static_cast<int>(nv_s), p->n_cpl_rows, want_d, q, qd, ydd,
                                      q_s, qd_s, x_s ? qdd_s : nullptr, cpl, nb, static_cast<int>(tile_grid(t.n_cu, 4, nb)), hs, p->constraint_shape, p->has_trig);
    if (e != hipSuccess) return hip_err(e, "manifold constraint launch");
    if (!x_s && (e = hipMemsetAsync(qd_s, 0, chunk * nv_s * sizeof(T), hs)) != hipSuccess) return hip_err(e, "hipMemsetAsync");
    if (int rc = x_s ? run<T>(sp, true, q_s, qd_s, qdd_s, f_ext, x_s, nb, device, stream) : GRBDA_OK) return rc;
    if (!Hs) return GRBDA_OK;
    const size_t g2 = tile_grid(ts.n_cu, 4, nb);
    void *scratch = nullptr;
    if (int rc = ensure_scratch(sp, device, stream, scratch_bytes(g2, sp->host.deriv.n_rows, sizeof(T)), &scratch)) return rc;
    e = launch_rnea_deriv<T>(ds, ts.deriv_bodies, sp->host.n_clusters, sp->host.deriv.n_rows, sp->host.deriv.n_max, q_s, qd_s, qdd_s, Aq, Av, Hs, nb,
                             static_cast<T *>(scratch), static_cast<int>(g2), hs, kWave);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "spanning derivative launch");
}

// the mass matrix by the composite-rigid-body kernel (crba_kernels.hip): one launch instead of nv + 1 inverse-dynamics evaluations
template <class T>
int crba_mass(const grbda_plan *p, const T *q, T *out, size_t B, int device, void *stream)
{
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const int nq = p->host.nq, nv = p->host.nv;
    const size_t nn = static_cast<size_t>(nv) * nv;
    DevPlan<T> d = make_dev_plan<T>(p, *t, false, false);
    const size_t crba_waves = static_cast<size_t>(sizeof(T) == 4 ? p->opt.crba_waves : std::min(p->opt.crba_waves, 8));  // (fp64: 256 registers, two per SIMD)
    const size_t grid = tile_grid(t->n_cu, crba_waves, B);
    void *scratch = nullptr;
    if (int rc = ensure_scratch(p, device, stream, scratch_bytes(grid, p->host.crba.n_rows, sizeof(T)), &scratch)) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (!t->deriv_related) {
        hipError_t e = hipMemsetAsync(out, 0, B * nn * sizeof(T), hs);
        if (e != hipSuccess) return hip_err(e, "hipMemsetAsync");
        e = launch_crba<T>(d, t->crba_bodies, p->host.n_clusters, p->host.crba.n_rows, q, out, B, static_cast<T *>(scratch), static_cast<int>(grid), hs, false, 1);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "crba launch");
    }
    // the lower triangle in packed rows (row-local stores), then unpacked in place, one wavefront per state (JVRC-1, 131 072 states, f32: 1.10 against
    // 1.65 ms for the plain layout; f64 about even); whole groups of kDerivGroup states interleaved (a quarter of the open cache lines per store)
    const int il = unpack_symmetric_lds_bytes(nv, sizeof(T), kDerivGroup) <= 60 * 1024 ? kDerivGroup : 1;
    return for_groups_then_tail(B, il, [&](size_t b0, size_t nb, int ilp) {
        hipError_t e = launch_crba<T>(d, t->crba_bodies, p->host.n_clusters, p->host.crba.n_rows, q + b0 * nq, out + b0 * nn, nb, static_cast<T *>(scratch),
                                      static_cast<int>(tile_grid(t->n_cu, crba_waves, nb)), hs, true, ilp);
        if (e != hipSuccess) return hip_err(e, "crba launch");
        const size_t g2 = persistent_grid(t->n_cu, 16, unpack_symmetric_lds_bytes(nv, sizeof(T), ilp), nb / ilp);
        e = launch_unpack_symmetric<T>(out + b0 * nn, t->deriv_related, nv, nb, static_cast<int>(g2), hs, ilp);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "unpack launch");
    });
}

// the expanded batches: expand / run / combine, in chunks of at most 256 MB of rows
template <class T>
int derived(const grbda_plan *p, int mode, const T *q, const T *qd, const T *tau, const T *f_ext, T *out, size_t B,
            int device, void *stream, double step = 1.0)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    const bool differences = dm_steps_qd(mode) || dm_steps_q(mode);
    if (!q || !out || ((mode == DM_BIAS || differences) && !qd) || (differences && !tau)) return set_err(GRBDA_EINVAL, "null argument");
    bool reproject = false;
    if (dm_steps_q(mode)) {
        if (!(step > 0)) return set_err(GRBDA_EINVAL, "step must be positive");
        for (const ClusterRec &c : p->host.lay64.clusters) reproject |= c.kind == CK_LOOP;
    }
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const int nq = p->host.nq, nv = p->host.nv;
    const int R = mode == DM_BIAS ? 1 : (differences ? 2 * nv : nv + 1);
    const size_t row_scalars = static_cast<size_t>(nq) + 3 * static_cast<size_t>(nv);  // q, qd, x, result
    const Chunk c = fixed_chunk(256u << 20, row_scalars * sizeof(T) * static_cast<size_t>(R), B);
    const size_t rows = c.chunk * static_cast<size_t>(R);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    Carver<T> w(wptr, rows * row_scalars);
    T *qx = w.take(rows * nq), *qdx = w.take(rows * nv), *xx = w.take(rows * nv), *res = w.take(rows * nv);
    assert(w.taken == w.cap);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const bool via_rnea = mode == DM_BIAS || mode == DM_MASS || mode == DM_ID_DQD || mode == DM_ID_DQ;
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        const size_t nrows = nb * static_cast<size_t>(R);
        hipLaunchKernelGGL((expand_kernel<T>), dim3(blocks_for(nrows * static_cast<size_t>(nq + 2 * nv))), dim3(256), 0, hs, mode, q + b0 * nq,
                           qd ? qd + b0 * nv : nullptr, tau ? tau + b0 * nv : nullptr, nq, nv, R, nb, qx, qdx, xx, t->dq_map,
                           static_cast<T>(step));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_err(e, "expand launch");
        if (reproject) {
            // the perturbed states leave the constraint manifold of the implicit clusters by O(step): Newton puts the
            // dependent coordinates back (GenericJoint.cpp:289-385), starting one step away from the solution
            if (int rc = project<T>(p, qx, nullptr, nrows, 25, sizeof(T) == 8 ? 1e-13 : 1e-6, device, stream)) return rc;
        }
        const T *fe = (mode == DM_BIAS && f_ext) ? f_ext + b0 * static_cast<size_t>(p->host.n_bodies) * 6 : nullptr;
        T *dst = mode == DM_BIAS ? out + b0 * nv : res;
        if (int rc = run<T>(p, via_rnea, qx, qdx, xx, fe, dst, nrows, device, stream)) return rc;
        if (mode != DM_BIAS) {
            hipLaunchKernelGGL((combine_kernel<T>), dim3(blocks_for(nb * static_cast<size_t>(nv) * nv)), dim3(256), 0, hs, mode, res, nv, R, nb,
                               out + b0 * static_cast<size_t>(nv) * nv, static_cast<T>(step));
            if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "combine launch");
        }
    }
    return GRBDA_OK;
}

// Forward / inverse dynamics through the spanning tree (HostPlan::projection_only; the reference's Projection-method cross-check,
// RigidBodyTreeDynamics.cpp:86-97):  tau = G^T ID_s(q_s, G yd, G ydd + g);  ydd = (G^T H_s G)^-1 (tau - G^T ID_s(q_s, G yd, g)).
template <class T>
int projection_run(const grbda_plan *p, bool rnea, const T *q, const T *qd, const T *x, const T *f_ext, T *out, size_t B, int device, void *stream)
{
    if (!p->span)
        return set_err(GRBDA_EUNSUPPORTED, "the model needs the spanning-tree route, which covers at most 64 spanning velocities (128 for plans with big clusters)");
    DeviceTables *t = nullptr, *ts = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const grbda_plan *sp = p->span;
    if (int rc = ensure_device(sp, device, &ts)) return rc;
    const bool big = p->host.big_clusters;
    const size_t nq = p->host.nq, nv = p->host.nv, nn = nv * nv;
    const size_t nq_s = sp->host.nq, nv_s = sp->host.nv, nn_s = nv_s * nv_s;
    // (forward dynamics: H_s alone of the spanning recursion's three matrices is stored)
    const size_t per_state = nq_s + 3 * nv_s + static_cast<size_t>(p->n_cpl_rows) + (rnea ? 0 : nn_s + 2 * nn);  // (wide: nn + nv would do)
    // (plans with big clusters: 40-50 KB per state; a chunk that leaves most SIMDs without a tile costs more than the memory)
    const Chunk c = budgeted_chunk(p, p->work_proj, device, stream, (big ? 4096ull : 1024ull) << 20, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work_proj, device, stream, c.bytes, &wptr)) return rc;
    Carver<T> w(wptr, c.chunk * per_state);
    auto take = [&](size_t per) { return w.take(c.chunk * per); };
    T *q_s = take(nq_s), *qd_s = take(nv_s), *qdd_s = take(nv_s), *x_s = take(nv_s), *cpl = take(p->n_cpl_rows);
    T *Hs = rnea ? nullptr : take(nn_s);
    // (more than 64 velocities: related-coordinate TABLES instead of one-word masks, and the workgroup-per-state solve on the one right-hand
    // side instead of H^-1 -- manifold_kernels.hip, kernels 2w and 4)
    const bool wide_nv = nv > static_cast<size_t>(kWave) || nv_s > static_cast<size_t>(kWave);
    T *Hw = rnea ? nullptr : take(nn), *Hinv = rnea ? nullptr : take(wide_nv ? nv : nn);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    DevPlan<T> d = make_dev_plan<T>(p, *t, false, false);
    DevPlan<T> ds = make_dev_plan<T>(sp, *ts, false, false);
    hipError_t e;
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        const size_t grid = tile_grid(t->n_cu, 4, nb);
        // inverse dynamics: qdd_s = G ydd + g; forward dynamics: qdd_s = g (the bias of the spanning tree with the constraint's own acceleration),
        // and H_s from the spanning recursion
        const T *fe = f_ext ? f_ext + b0 * static_cast<size_t>(p->host.n_bodies) * 6 : nullptr;
        if (int rc = spanning_stage<T>(p, *t, *ts, d, ds, 0, q + b0 * nq, qd + b0 * nv, rnea ? x + b0 * nv : nullptr, fe, q_s, qd_s, qdd_s, cpl, x_s, nullptr, nullptr, Hs, nb, c.chunk, device, stream)) return rc;
        if (rnea) {
            e = launch_manifold_apply<T>(d, p->host.n_clusters, t->span_v, t->crow, static_cast<int>(nv_s), p->n_cpl_rows, 0, x_s, nullptr, nullptr,
                                         cpl, out + b0 * nv, nb, static_cast<int>(grid), hs, big);
            if (e != hipSuccess) return hip_err(e, "manifold apply launch");
            continue;
        }
        if (wide_nv) {
            if (!t->related_table || !ts->related_table) return set_err(GRBDA_EUNSUPPORTED, "more than 64 velocities on a plan without big clusters");
            e = launch_manifold_project_wide<T>(d, p->host.n_clusters, t->span_v, t->crow, nullptr, nullptr, t->related_table, ts->related_table,
                                                static_cast<int>(nv_s), p->n_cpl_rows, Hs, cpl, Hw, nb, static_cast<int>(grid), hs);
            if (e != hipSuccess) return hip_err(e, "manifold projection launch");
            e = launch_manifold_apply<T>(d, p->host.n_clusters, t->span_v, t->crow, static_cast<int>(nv_s), p->n_cpl_rows, 2, x_s, x + b0 * nv, nullptr,
                                         cpl, Hinv, nb, static_cast<int>(grid), hs, big);
            if (e != hipSuccess) return hip_err(e, "manifold apply launch");
            e = launch_spd_wide_solve<T>(Hw, t->related_table, Hinv, out + b0 * nv, static_cast<int>(nv), nb, t->n_cu, hs, spd_bad_count_address());
            if (e != hipSuccess) return hip_err(e, "wide solve launch");
            continue;
        }
        e = launch_manifold_project<T>(d, p->host.n_clusters, t->span_v, t->crow, t->deriv_related, ts->deriv_related, static_cast<int>(nv_s),
                                       p->n_cpl_rows, 1, nullptr, nullptr, Hs, nullptr, cpl, nullptr, nullptr, Hw, nb, static_cast<int>(grid), hs, 1, big);
        if (e != hipSuccess) return hip_err(e, "manifold projection launch");
        // (H^-1 alone, never on the matrix cores)
        e = spd_solve_stage<T>(*t, Hw, nullptr, nullptr, Hinv, nullptr, nullptr, static_cast<int>(nv), 0, nb, false, false, 1, hs);
        if (e != hipSuccess) return hip_err(e, "spd solve launch");
        e = launch_manifold_apply<T>(d, p->host.n_clusters, t->span_v, t->crow, static_cast<int>(nv_s), p->n_cpl_rows, 1, x_s, x + b0 * nv, Hinv, cpl,
                                     out + b0 * nv, nb, static_cast<int>(grid), hs, big);
        if (e != hipSuccess) return hip_err(e, "manifold apply launch");
    }
    return GRBDA_OK;
}

// fp32 entry points that compute in fp64.  Chunk by chunk (at most `cap_bytes` of fp64 copies in the plan's work_cvt slab): the arrays with a
// `src` are converted, call(a, nb) runs the fp64 routine on the chunk's arrays a[i] (null where the caller gave none), the arrays with a
// `dst` are converted back.  `width`: scalars per state.
struct CvtArray {
    const float *src;
    float *dst;
    size_t width;
};
template <size_t N, class Call>
int through_f64(const grbda_plan *p, size_t cap_bytes, const CvtArray (&arrays)[N], size_t B, int device, void *stream, Call call)
{
    size_t per_state = 0;
    for (const CvtArray &a : arrays) per_state += (a.src || a.dst) ? a.width : 0;
    const Chunk c = fixed_chunk(cap_bytes, per_state * sizeof(double), B);
    void *cvt = nullptr;
    if (int rc = ensure_work(p, p->work_cvt, device, stream, c.bytes, &cvt)) return rc;
    Carver<double> w(cvt, c.chunk * per_state);
    double *a64[N];
    for (size_t i = 0; i < N; i++) a64[i] = (arrays[i].src || arrays[i].dst) ? w.take(c.chunk * arrays[i].width) : nullptr;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    for (const auto [b0, nb] : ChunkWalk{B, c.chunk}) {
        for (size_t i = 0; i < N; i++) {
            const size_t n = nb * arrays[i].width;
            if (arrays[i].src) hipLaunchKernelGGL((convert_kernel<float, double>), dim3(blocks_for(n)), dim3(256), 0, hs, arrays[i].src + b0 * arrays[i].width, a64[i], n);
        }
        if (int rc = call(a64, nb)) return rc;
        for (size_t i = 0; i < N; i++) {
            const size_t n = nb * arrays[i].width;
            if (arrays[i].dst) hipLaunchKernelGGL((convert_kernel<double, float>), dim3(blocks_for(n)), dim3(256), 0, hs, a64[i], arrays[i].dst + b0 * arrays[i].width, n);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_err(e, "convert launch");
    }
    return GRBDA_OK;
}

int projection_run_f32_through_f64(const grbda_plan *p, bool rnea, const float *q, const float *qd, const float *x, const float *f_ext, float *out,
                                   size_t B, int device, void *stream)
{
    const size_t nq = p->host.nq, nv = p->host.nv, nfe = static_cast<size_t>(p->host.n_bodies) * 6;
    const CvtArray arrays[] = {{q, nullptr, nq}, {qd, nullptr, nv}, {x, nullptr, nv}, {nullptr, out, nv}, {f_ext, nullptr, nfe}};
    return through_f64(p, 256u << 20, arrays, B, device, stream, [&](double *const *a, size_t nb) {
        return projection_run<double>(p, rnea, a[0], a[1], a[2], a[4], a[3], nb, device, stream);
    });
}
// The central difference d/dq (DM_DQ, DM_ID_DQ) for fp32 callers.  A central difference in fp32 has no usable step (eps / h + h^2 bottoms
// out near 1e-2 relative): the differences are taken in fp64 on the converted inputs and the matrices converted back.
int dq_through_f64(const grbda_plan *p, int mode, const float *q, const float *qd, const float *x, double step, float *J, size_t B, int device,
                   void *stream)
{
    const size_t nq = p->host.nq, nv = p->host.nv;
    const CvtArray arrays[] = {{q, nullptr, nq}, {qd, nullptr, nv}, {x, nullptr, nv}, {nullptr, J, nv * nv}};
    return through_f64(p, 64u << 20, arrays, B, device, stream, [&](double *const *a, size_t nb) {
        return derived<double>(p, mode, a[0], a[1], a[2], nullptr, a[3], nb, device, stream, step);
    });
}

// BY_MANIFOLD, MASS_MANIFOLD.  Models with implicit clusters (manifold_kernels.hip): ydd = FD; spanning state and the first-order parts of G, g
// per state; tau_s and (A_q, A_v, H_s) of the spanning tree from its own plan; projection with the per-state G; the same SPD solve.
// H only (dq == dqd == nullptr): qd and tau may be null.  Plans with big clusters have no analytic d/dq, d/dqd (choose_derivs): forward dynamics
// differences for explicit clusters; implicit ones would need the Newton re-projection, which refuses such plans.
template <class T>
int manifold_derivs(const grbda_plan *p, const T *q, const T *qd, const T *tau, T *dq, T *dqd, T *dtau, T *Hout, size_t B, int device,
                    void *stream)
{
    DeviceTables *t = nullptr, *ts = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const grbda_plan *sp = p->span;
    if (int rc = ensure_device(sp, device, &ts)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, nn = nv * nv;
    const size_t nq_s = sp->host.nq, nv_s = sp->host.nv, nn_s = nv_s * nv_s;
    const bool need_d = dq || dqd;
    const bool big = p->host.big_clusters;
    assert(!(big && need_d));
    const int n_rhs = (dq ? 1 : 0) + (dqd ? 1 : 0);
    const bool solve = need_d || dtau;
    // (H^-1 alone stays off the matrix cores here)
    const bool mfma = need_d && spd_solve_on_mfma(sizeof(T), static_cast<int>(nv), n_rhs);
    const int il = mfma ? kDerivGroup : 1;
    // workspace per state: spanning state (q_s, qd_s, qdd_s, tau_s), zeros for a missing qd, coupling rows, the three spanning
    // matrices, the three projected matrices, ydd
    const size_t per_state = nq_s + 3 * nv_s + nv + static_cast<size_t>(p->n_cpl_rows) + 3 * nn_s + 3 * nn + nv;
    // (16 GiB, cut to a quarter of the free memory: TelloWithArms takes 33 KB per state; a 4 GiB chunk -- 131 072 states, 2 048 tiles -- left half
    // of the projection kernel's wavefront slots empty: 13.3 -> 10.8 ms per 262 144 states, 55 -> 44 ms per 1 048 576)
    // (up to 16 GiB -- but no more than the batch itself needs: a small batch does not pin a large slab)
    const size_t want = std::min<size_t>(16384ull << 20, ((B + kWave - 1) / kWave * kWave) * per_state * sizeof(T) + (1u << 20));
    const Chunk c = budgeted_chunk(p, p->work, device, stream, want, per_state * sizeof(T), B);
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, c.bytes, &wptr)) return rc;
    const size_t chunk = c.chunk;
    Carver<T> w(wptr, chunk * per_state);
    auto take = [&](size_t per) { return w.take(chunk * per); };
    T *q_s = take(nq_s), *qd_s = take(nv_s), *qdd_s = take(nv_s), *tau_s = take(nv_s), *zeros = take(nv), *cpl = take(p->n_cpl_rows);
    T *Aq = take(nn_s), *Av = take(nn_s), *Hs = take(nn_s), *Dq = take(nn), *Dqd = take(nn), *Hw = take(nn), *ydd = take(nv);
    assert(w.taken == w.cap);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    DevPlan<T> d = make_dev_plan<T>(p, *t, false, false);
    DevPlan<T> ds = make_dev_plan<T>(sp, *ts, false, false);
    hipError_t e;
    for (const auto [b0, nb] : ChunkWalk{B, chunk}) {
        const T *qc = q + b0 * nq, *qdc = need_d ? qd + b0 * nv : zeros;  // (H only: zero velocities, whatever the caller gave)
        if (!need_d && (e = hipMemsetAsync(zeros, 0, nb * nv * sizeof(T), hs)) != hipSuccess) return hip_err(e, "hipMemsetAsync");
        if (need_d)
            if (int rc = run<T>(p, false, qc, qdc, tau + b0 * nv, nullptr, ydd, nb, device, stream)) return rc;
        if (int rc = spanning_stage<T>(p, *t, *ts, d, ds, need_d ? 1 : 0, qc, qdc, need_d ? ydd : nullptr, nullptr, q_s, qd_s, qdd_s, cpl,
                                       need_d ? tau_s : nullptr, need_d ? Aq : nullptr, need_d ? Av : nullptr, Hs, nb, chunk, device, stream))
            return rc;
        const size_t grid = tile_grid(t->n_cu, 4, nb);
        // the projected H goes to the caller's array when no solve follows, or (state-major layouts, whole groups) to d/dtau
        T *H = !solve ? Hout + b0 * nn : ((dtau && !(il > 1 && (B % kDerivGroup) != 0)) ? dtau + b0 * nn : Hw);
        e = launch_manifold_project<T>(d, p->host.n_clusters, t->span_v, t->crow, t->deriv_related, ts->deriv_related, static_cast<int>(nv_s),
                                       p->n_cpl_rows, need_d ? 0 : 1, Aq, Av, Hs, tau_s, cpl, need_d ? Dq : nullptr, need_d ? Dqd : nullptr, H,
                                       nb, static_cast<int>(grid), hs, solve ? il : 1, big);
        if (e != hipSuccess) return hip_err(e, "manifold projection launch");
        if (!solve) {
            // packed lower rows -> the full symmetric matrix, in place
            const size_t g4 = persistent_grid(t->n_cu, 16, unpack_symmetric_lds_bytes(static_cast<int>(nv), sizeof(T), 1), nb);
            e = launch_unpack_symmetric<T>(H, t->deriv_related, static_cast<int>(nv), nb, static_cast<int>(g4), hs, 1);
            if (e != hipSuccess) return hip_err(e, "unpack launch");
            continue;
        }
        e = spd_solve_stage<T>(*t, H, dq ? Dq : nullptr, dqd ? Dqd : nullptr, dtau ? dtau + b0 * nn : nullptr, dq ? dq + b0 * nn : nullptr,
                               dqd ? dqd + b0 * nn : nullptr, static_cast<int>(nv), n_rhs, nb, false, mfma, il, hs);
        if (e != hipSuccess) return hip_err(e, "spd solve launch");
    }
    return GRBDA_OK;
}

// Chunk size of analytic_derivs.  The slab holds chunk * per_state scalars, plus B nv of them (`ydd_bytes`) when the forward dynamics of the
// WHOLE batch runs in one launch up front (160 MB for a million JVRC-1 states in fp32) instead of one launch per chunk -- a
// quarter-million-state launch runs at 0.35 ms, a quarter of the million-state launch at 0.29.  Every branch keeps the slab within the
// budget, or at one tile of states when the budget is smaller than that.  A stream that captures replays the decision of the eager call it
// captures after (same B, same layout; grbda_plan::deriv_chunk): the held slab may have grown since, and a chunk derived from it again would
// record another launch sequence.
grbda_plan::DerivChunk deriv_chunk_decision(const grbda_plan *p, int n_cu, size_t ps_bytes, bool need_d, size_t ydd_bytes, size_t B, int device,
                                            void *stream)
{
    const bool capturing = is_capturing(stream);
    const auto it = p->deriv_chunk.find({device, stream});
    if (capturing && it != p->deriv_chunk.end() && it->second.B == B && it->second.per_state_bytes == ps_bytes && it->second.need_d == need_d && it->second.chunk)
        return it->second;
    const size_t B_groups = (B + kDerivGroup - 1) / kDerivGroup * kDerivGroup;  // (the last group of the workspace is allocated whole)
    grbda_plan::DerivChunk dc = {B, ps_bytes, B_groups, need_d, false};            // one chunk: no whole-batch ydd
    const size_t budget = work_budget(p, p->work, device, stream, (4096ull << 20) + ydd_bytes);
    if (B_groups * ps_bytes > budget) {
        // (room for the whole batch's ydd and a tile of states besides; otherwise the forward dynamics runs per chunk)
        dc.ydd_all = need_d && budget >= ydd_bytes + static_cast<size_t>(kWave) * ps_bytes;
        dc.chunk = whole_tiles((budget - (dc.ydd_all ? ydd_bytes : 0)) / (ps_bytes ? ps_bytes : 1));  // (and with them whole groups of the interleaved workspace)
        // whole ROUNDS of the one-state-per-lane kernels: a chunk of 2.4 rounds of wavefront slots takes as long as 3 (measured: 159 488-state
        // chunks of JVRC-1, 2 492 tiles on 1 024 slots of the recursion and 2 048 of the factor kernel / the ABA: 19 % and 40 % of the
        // slots idle in the last round).  n_cu * 8 wavefronts = one round at two per SIMD, two rounds of the recursion's four per CU.
        const size_t round = static_cast<size_t>(n_cu) * 8 * kWave;
        if (dc.chunk >= round) dc.chunk = dc.chunk / round * round;
        if (dc.chunk >= B) {  // (only when the budget is below one tile: a single chunk, then without the whole-batch ydd)
            dc.chunk = B_groups;
            dc.ydd_all = false;
        }
    }
    if (!capturing) p->deriv_chunk[{device, stream}] = dc;
    return dc;
}
// d ydd / d tau = H^-1, d ydd / d q = -H^-1 dID/dq, d ydd / d qd = -H^-1 dID/dqd at ydd = FD(q, qd, tau); any of the three outputs may be
// null, one at least is not.  `minv`, `wide`: choose_derivs (BY_MINV; DerivRoute::solve_f64).
template <class T>
int analytic_derivs(const grbda_plan *p, const DeviceTables *t, bool minv, bool wide, const T *q, const T *qd, const T *tau, T *dq, T *dqd, T *dtau,
                    size_t B, int device, void *stream)
{
    const size_t nq = p->host.nq, nv = p->host.nv, nn = nv * nv;
    const bool need_d = dq || dqd;
    // H is built in the caller's d/dtau array when that is wanted (the factor is out of it before H^-1 goes in); dID/dq and
    // dID/dqd in rnea_deriv_kernel's packed layout, the H nobody asked for, and ydd take workspace
    const int n_rhs = (dq ? 1 : 0) + (dqd ? 1 : 0);
    // (d / d tau alone: the CRBA kernel writes the same interleaved H and the matrix-core solve inverts it)
    // (fp64 stays state-major: its interleaved workspace was built and measured in round 4 -- MIT Humanoid 8 % faster, JVRC-1 36 % slower, the
    // row-per-lane fp64 solve reads an interleaved block strided; profiles/r4_derivative_recursion_experiments.txt -- and removed again)
    // H^-1 = W^T W from the articulated-body quantities (minv_kernels.hip): no H, no dense factorisation; f32 and f64 alike on the
    // matrix cores, both workspaces interleaved by groups of kDerivGroup states.
    const MinvProgram &mv = p->host.deriv.minv;
    // f32 with the matrix-core solve: the recursion writes H, dID/dq, dID/dqd interleaved by groups of kDerivGroup states
    // (deriv_kernels.hip); every other combination of the factorisation route keeps the state-major layout
    const bool mfma = !minv && !wide && spd_solve_on_mfma(sizeof(T), static_cast<int>(nv), n_rhs);
    const int il = (minv || mfma) ? kDerivGroup : 1;
    // (only an INTERLEAVED H block can reach past the caller's array: the state-major layouts always build H in place)
    const bool h_in_place = !minv && dtau && (il == 1 || (B % kDerivGroup) == 0);
    const size_t per_state = minv ? static_cast<size_t>(mv.n_entries) + (need_d ? 2 * nn + nv : 0)
                                  : (h_in_place ? 0 : nn) + (need_d ? 2 * nn + nv : 0);
    const grbda_plan::DerivChunk dc = deriv_chunk_decision(p, t->n_cu, per_state * sizeof(T), need_d, need_d ? B * nv * sizeof(T) : 0, B, device, stream);
    const size_t chunk = dc.chunk;
    void *wptr = nullptr;
    if (int rc = ensure_work(p, p->work, device, stream, (chunk * per_state + (dc.ydd_all ? B * nv : 0)) * sizeof(T) + 256, &wptr)) return rc;
    Carver<T> w(wptr, chunk * per_state + (dc.ydd_all ? B * nv : 0));
    T *wH = (!minv && !h_in_place) ? w.take(chunk * nn) : nullptr, *Dq = need_d ? w.take(chunk * nn) : nullptr, *Dqd = need_d ? w.take(chunk * nn) : nullptr;
    T *ydd_chunk = w.take(need_d ? chunk * nv : 0);
    T *recs = minv ? w.take(chunk * mv.n_entries) : nullptr;
    assert(w.taken == chunk * per_state);
    T *ydd_whole = dc.ydd_all ? w.take(B * nv) : nullptr;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    DevPlan<T> d = make_dev_plan<T>(p, *t, false, false);
    if (dc.ydd_all)
        if (int rc = run<T>(p, false, q, qd, tau, nullptr, ydd_whole, B, device, stream)) return rc;
    for (const auto [b0, nb] : ChunkWalk{B, chunk}) {
        T *ydd = dc.ydd_all ? ydd_whole + b0 * nv : ydd_chunk;
        // (an interleaved H block spans the slots of a whole group: when the batch does not end on a group boundary the last
        // group would reach past the caller's d/dtau array, so that H goes to the workspace)
        T *H = h_in_place ? dtau + b0 * nn : wH;
        hipError_t e = hipSuccess;
        // (both kernels write H as packed rows of its lower triangle; the solve reads it through DerivProgram::related, so
        // nothing is cleared)
        if (need_d && !dc.ydd_all)
            if (int rc = run<T>(p, false, q + b0 * nq, qd + b0 * nv, tau + b0 * nv, nullptr, ydd, nb, device, stream)) return rc;
        const size_t grid = tile_grid(t->n_cu, 8, nb);
        const size_t rows = std::max(p->host.crba.n_rows, (need_d || minv) ? p->host.deriv.n_rows : 0);  // (the factor kernel of the minv route uses the recursion's rows)
        // (state-major results: three wavefronts per CU -- a fourth only adds open cache lines; interleaved: one per SIMD)
        const size_t deriv_waves = p->opt.deriv_waves ? static_cast<size_t>(p->opt.deriv_waves) : (il > 1 ? 4 : 3);
        const size_t slabs = std::max(grid, static_cast<size_t>(t->n_cu) * deriv_waves);  // (the factor kernel of the minv route runs n_cu * 8 wavefronts, as `grid`)
        void *scratch = nullptr;
        if (int rc = ensure_scratch(p, device, stream, scratch_bytes(slabs, rows, sizeof(T)), &scratch)) return rc;
        if (need_d) {
            // (the derivative recursion carries the composite inertias in a common frame: H comes out of the same launch)
            const size_t g2 = tile_grid(t->n_cu, deriv_waves, nb);
            e = launch_rnea_deriv<T>(d, t->deriv_bodies, p->host.n_clusters, p->host.deriv.n_rows, p->host.deriv.n_max, q + b0 * nq,
                                     qd + b0 * nv, ydd, Dq, Dqd, minv ? nullptr : H, nb, static_cast<T *>(scratch), static_cast<int>(g2), hs, il);
            if (e != hipSuccess) return hip_err(e, "rnea derivative launch");
        } else if (!minv) {
            e = launch_crba<T>(d, t->crba_bodies, p->host.n_clusters, p->host.crba.n_rows, q + b0 * nq, H, nb, static_cast<T *>(scratch),
                               static_cast<int>(grid), hs, true, il);
            if (e != hipSuccess) return hip_err(e, "crba launch");
        }
        T *o1 = dq ? dq + b0 * nn : nullptr, *o2 = dqd ? dqd + b0 * nn : nullptr, *o3 = dtau ? dtau + b0 * nn : nullptr;
        const T *r1 = dq ? Dq : nullptr, *r2 = dqd ? Dqd : nullptr;
        if (!minv) {
            e = spd_solve_stage<T>(*t, H, r1, r2, o3, o1, o2, static_cast<int>(nv), n_rhs, nb, wide, mfma, il, hs);
            if (e != hipSuccess) return hip_err(e, "spd solve launch");
            continue;
        }
        // articulated-inertia recursion -> record blocks (one state per lane, two wavefronts per SIMD), then the walk and the two
        // products on the matrix cores (one state per wavefront)
        e = launch_abi_factor<T>(d, t->deriv_bodies, t->minv_bodies, p->host.n_clusters, p->host.deriv.n_rows, p->host.deriv.n_max,
                                 mv.n_entries, q + b0 * nq, recs, nb, static_cast<T *>(scratch), static_cast<int>(grid), hs, kDerivGroup,
                                 t->bad_count);
        if (e != hipSuccess) return hip_err(e, "articulated-inertia factor launch");
        size_t per_cu = static_cast<size_t>(minv_workgroups_per_cu<T>(static_cast<int>(nv), p->host.deriv.n_max, n_rhs, mv.n_entries));
        if (p->opt.minv_wpc > 0 && per_cu > static_cast<size_t>(p->opt.minv_wpc)) per_cu = static_cast<size_t>(p->opt.minv_wpc);
        const size_t g3 = std::min(static_cast<size_t>(t->n_cu) * per_cu, (nb + kDerivGroup - 1) / kDerivGroup);
        e = launch_minv_solve<T>(recs, mv.n_entries, kDerivGroup, t->minv_coltab, mv.max_depth, mv.base_off, p->host.deriv.n_max, r1, r2,
                                 kDerivGroup, o3, o1, o2, t->deriv_related, static_cast<int>(nv), nb, static_cast<int>(g3), hs);
        if (e != hipSuccess) return hip_err(e, "minv solve launch");
    }
    return GRBDA_OK;
}

// ---- grbda_fd_dtau_* / _dqd_* / _dq_* / _derivatives_* ----------------------------------------------------------------------------------
// Their one body; `args`: the entry point was given every array it needs.  The route record once, its one analytic or manifold stage for the
// outputs that stage covers, a difference batch for each of the others (d/dtau, d/dqd, d/dq, in that order).
template <class T>
int fd_by_route(const grbda_plan *p, bool args, const T *q, const T *qd, const T *tau, double step, T *dq, T *dqd, T *dtau, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!args) return set_err(GRBDA_EINVAL, "null argument");
    // (fp64 looks at the step first; fp32, whose differences are taken in fp64, after an empty batch and a missing device -- as the entry points always did)
    if (sizeof(T) == 8 && !(step > 0)) return set_err(GRBDA_EINVAL, "step must be positive");
    if (B == 0 || (!dq && !dqd && !dtau)) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    if (!(step > 0)) return set_err(GRBDA_EINVAL, "step must be positive");
    const DerivRoute r = choose_derivs(p, t->minv_bodies && t->minv_coltab, sizeof(T), dq, dqd, dtau);
    const DerivPath stage = dtau && r.dtau != BY_DIFFERENCES ? r.dtau : (dq ? r.dq : r.dqd);
    const auto staged = [](T *out, DerivPath path) { return path == BY_DIFFERENCES ? nullptr : out; };
    int rc = GRBDA_OK;
    if (stage == BY_MANIFOLD) rc = manifold_derivs<T>(p, q, qd, tau, staged(dq, r.dq), staged(dqd, r.dqd), dtau, nullptr, B, device, stream);
    else if (stage == BY_MINV || stage == BY_FACTOR) rc = analytic_derivs<T>(p, t, stage == BY_MINV, r.solve_f64, q, qd, tau, dq, dqd, dtau, B, device, stream);
    if (!rc && r.dtau == BY_DIFFERENCES) rc = derived<T>(p, DM_DTAU, q, nullptr, nullptr, nullptr, dtau, B, device, stream);
    if (!rc && r.dqd == BY_DIFFERENCES) rc = derived<T>(p, DM_DQD, q, qd, tau, nullptr, dqd, B, device, stream);
    if (rc || r.dq != BY_DIFFERENCES) return rc;
    if constexpr (sizeof(T) == 4) return dq_through_f64(p, DM_DQ, q, qd, tau, step, dq, B, device, stream);
    else return derived<T>(p, DM_DQ, q, qd, tau, nullptr, dq, B, device, stream, step);
}
template <class T>
int fd_dtau(const grbda_plan *p, const T *q, T *Hinv, size_t B, int device, void *stream)
{
    return fd_by_route<T>(p, q && Hinv, q, nullptr, nullptr, 1.0, nullptr, nullptr, Hinv, B, device, stream);
}
template <class T>
int fd_dqd(const grbda_plan *p, const T *q, const T *qd, const T *tau, T *J, size_t B, int device, void *stream)
{
    return fd_by_route<T>(p, q && qd && tau && J, q, qd, tau, 1.0, nullptr, J, nullptr, B, device, stream);
}
template <class T>
int fd_dq(const grbda_plan *p, const T *q, const T *qd, const T *tau, double step, T *J, size_t B, int device, void *stream)
{
    if (sizeof(T) == 4 && !p) return set_err(GRBDA_EINVAL, "null argument");  // (the fp32 entry point's word for a null plan)
    return fd_by_route<T>(p, q && qd && tau && J, q, qd, tau, step, J, nullptr, nullptr, B, device, stream);
}
template <class T>
int fd_derivatives(const grbda_plan *p, const T *q, const T *qd, const T *tau, T *dq, T *dqd, T *dtau, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null argument");  // (as for a null array)
    return fd_by_route<T>(p, q && qd && tau, q, qd, tau, 1e-6, dq, dqd, dtau, B, device, stream);
}

// ---- first-order derivatives of the INVERSE dynamics (grbda_rnea_derivatives_*, include/grbda_hip.h) ------------------------------------
// [a, a + n) and [b, b + m) share a byte
bool ranges_overlap(const void *a, size_t n, const void *b, size_t m)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && n && m && x < y + m && y < x + n;
}
// d tau / d q and d tau / d qd at (q, qd, ydd).  Plans the analytic recursion covers: rnea_deriv_kernel on the caller's ydd (no forward
// dynamics, no solve) writes its run layout STRAIGHT INTO dq / dqd -- whole groups of kDerivGroup states interleaved where
// unpack_runs_interleave allows, the tail of the batch state-major, as crba_mass() lays out H -- and unpack_runs_kernel turns
// every block into row-major in place: the scratch slab, no work slab, the same launches for the same B (capturable).  Every other plan:
// the difference batches of derived() over the inverse dynamics.
template <class T>
int id_derivs(const grbda_plan *p, const T *q, const T *qd, const T *ydd, double step, T *dq, T *dqd, size_t B, int device, void *stream)
{
    if (!analytic_covers(p)) {
        if (dqd)
            if (int rc = derived<T>(p, DM_ID_DQD, q, qd, ydd, nullptr, dqd, B, device, stream)) return rc;
        if (!dq) return GRBDA_OK;
        if constexpr (sizeof(T) == 8) return derived<T>(p, DM_ID_DQ, q, qd, ydd, nullptr, dq, B, device, stream, step);
        else if (!(step > 0)) return set_err(GRBDA_EINVAL, "step must be positive");
        else return dq_through_f64(p, DM_ID_DQ, q, qd, ydd, step, dq, B, device, stream);
    }
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    if (!t->deriv_related) return set_err(GRBDA_EUNSUPPORTED, "the plan has no related-coordinate masks on the device");
    const size_t nq = p->host.nq, nv = p->host.nv, nn = nv * nv;
    const int nvi = static_cast<int>(nv);
    // (interleaved results: one wavefront per SIMD; state-major: three per CU -- analytic_derivs)
    const size_t waves_il = p->opt.deriv_waves ? static_cast<size_t>(p->opt.deriv_waves) : 4, waves_sm = p->opt.deriv_waves ? waves_il : 3;
    void *scratch = nullptr;
    if (int rc = ensure_scratch(p, device, stream, scratch_bytes(tile_grid(t->n_cu, std::max(waves_il, waves_sm), B), p->host.deriv.n_rows, sizeof(T)), &scratch))
        return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    DevPlan<T> d = make_dev_plan<T>(p, *t, false, false);
    T *o0 = dq ? dq : dqd, *o1 = dq ? dqd : nullptr;  // (the unpack's first matrix is never null)
    return for_groups_then_tail(B, unpack_runs_interleave(nvi, sizeof(T)), [&](size_t b0, size_t nb, int ilp) {
        const size_t g = tile_grid(t->n_cu, ilp > 1 ? waves_il : waves_sm, nb);
        hipError_t e = launch_rnea_deriv<T>(d, t->deriv_bodies, p->host.n_clusters, p->host.deriv.n_rows, p->host.deriv.n_max, q + b0 * nq, qd + b0 * nv,
                                            ydd + b0 * nv, dq ? dq + b0 * nn : nullptr, dqd ? dqd + b0 * nn : nullptr, nullptr, nb, static_cast<T *>(scratch),
                                            static_cast<int>(g), hs, ilp);
        if (e != hipSuccess) return hip_err(e, "rnea derivative launch");
        // (workgroups of 256 threads, eight per CU at the most)
        const size_t g2 = persistent_grid(t->n_cu, 8, unpack_runs_lds_bytes(nvi, sizeof(T), ilp), nb / ilp);
        e = launch_unpack_runs<T>(o0 + b0 * nn, o1 ? o1 + b0 * nn : nullptr, t->deriv_related, nvi, nb, static_cast<int>(g2), hs, ilp);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "run unpack launch");
    });
}
template <class T>
int mass_matrix(const grbda_plan *p, const T *q, T *H, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !H) return set_err(GRBDA_EINVAL, "null argument");
    if (B == 0) return GRBDA_OK;
    const MassPath m = choose_derivs(p, false, sizeof(T), false, false, false).mass;
    if (m == MASS_MANIFOLD) return manifold_derivs<T>(p, q, nullptr, nullptr, nullptr, nullptr, nullptr, H, B, device, stream);
    if (m == MASS_CRBA) return crba_mass<T>(p, q, H, B, device, stream);
    return derived<T>(p, DM_MASS, q, nullptr, nullptr, nullptr, H, B, device, stream);
}
// the argument rules of grbda_rnea_derivatives_* (device and host arrays alike)
template <class T>
int rnea_derivatives_args(const grbda_plan *p, const T *q, const T *qd, const T *ydd, const T *dq, const T *dqd, const T *dydd, size_t B)
{
    if (!q || !qd || !ydd) return set_err(GRBDA_EINVAL, "null argument");
    if (!dq && !dqd && !dydd) return set_err(GRBDA_EINVAL, "no output asked for");
    const size_t nq = p->host.nq, nv = p->host.nv, bo = B * nv * nv * sizeof(T);
    const void *const in[3] = {q, qd, ydd}, *const out[3] = {dq, dqd, dydd};
    const size_t in_bytes[3] = {B * nq * sizeof(T), B * nv * sizeof(T), B * nv * sizeof(T)}, out_bytes[3] = {bo, bo, bo};
    return no_overlap(in, in_bytes, out, out_bytes);
}
template <class T>
int rnea_derivatives(const grbda_plan *p, const T *q, const T *qd, const T *ydd, double step, T *dq, T *dqd, T *dydd, size_t B, int device,
                     void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = rnea_derivatives_args<T>(p, q, qd, ydd, dq, dqd, dydd, B)) return rc;
    if (B == 0) return GRBDA_OK;
    // d tau / d ydd = H(q): the mass-matrix entry point, whatever else is asked for (the same bits in every subset of the outputs)
    if (dydd)
        if (int rc = mass_matrix<T>(p, q, dydd, B, device, stream)) return rc;
    if (!dq && !dqd) return GRBDA_OK;
    return id_derivs<T>(p, q, qd, ydd, step, dq, dqd, B, device, stream);
}

// ---- vector-Jacobian and Jacobian-vector products (include/grbda_hip_vjp.h, grbda_hip_step_vjp.h, grbda_hip_jvp.h) --------------------
// The plans the stepping entry points of the three headers refuse: what grbda_step_* refuses, and every implicit cluster (the Jacobian of
// the Newton re-projection is not built).  *base: the index of the quaternion base's cluster record, -1 for a plan without one.
int step_vjp_plan(const grbda_plan *p, int *base)
{
    *base = -1;
    const std::vector<ClusterRec> &cl = p->host.lay64.clusters;
    for (size_t c = 0; c < cl.size(); c++) {
        if (cl[c].kind != CK_FREE) continue;
        if (p->host.ori_repr != 0)
            return set_err(GRBDA_EUNSUPPORTED, "time stepping covers the quaternion floating base only: the rate map of a roll-pitch-yaw base is not built");
        if (*base >= 0 || cl[c].n != 6 || cl[c].v_index + 6 > p->host.nv) return set_err(GRBDA_EUNSUPPORTED, "the step's vector-Jacobian product covers one floating base");
        *base = static_cast<int>(c);
    }
    if (has_loop_clusters(p))
        return set_err(GRBDA_EUNSUPPORTED, "the vector-Jacobian products of integrate, step and rollout do not cover implicit clusters: the Jacobian of "
                                           "the Newton re-projection is not built");
    return GRBDA_OK;
}
// an array of a call and the bytes it spans (bytes, not a width: the rollout's arrays hold a block of the batch per step)
struct Extent {
    const void *ptr;
    size_t bytes;
};
using Extents = std::initializer_list<Extent>;
constexpr char kNoCotangent[] = "both cotangents are null", kNoTangent[] = "all tangents are null";
// The argument rules of every entry point of the three headers (device and host arrays alike), in the one order all of them apply:
//   1 every state input is given                      2 one of the optional (co)tangents is (`none`: the message; no list, no rule)
//   3 one of the first `asked` outputs is (an output behind them, ydd of the forward side, is no product of its own)
//   4 dt, where the entry point has one, is finite    5 no output shares a byte with an input or with another output
//   6 stepping: the plan is one step_vjp_plan takes (it fills *base)
//   7 diff_q: the step is positive off the analytic route (its one use: d tau / d q by central differences, id_derivs)
// Everything that can be refused is refused here, before a device is looked at.
int product_rules(const grbda_plan *p, Extents state, Extents tangents, const char *none, Extents out, size_t asked, const double *dt, bool stepping,
                  bool diff_q, double step, int *base)
{
    const void *in[8] = {}, *o[4] = {};  // (a null entry is skipped by no_overlap)
    size_t in_bytes[8] = {}, o_bytes[4] = {}, ni = 0, no = 0;
    assert(state.size() + tangents.size() <= 8 && out.size() <= 4);
    bool any_tangent = tangents.size() == 0, any_out = false;
    for (const Extent &e : state) {
        if (!e.ptr) return set_err(GRBDA_EINVAL, "null argument");
        in[ni] = e.ptr, in_bytes[ni++] = e.bytes;
    }
    for (const Extent &e : tangents) {
        any_tangent = any_tangent || e.ptr;
        in[ni] = e.ptr, in_bytes[ni++] = e.bytes;
    }
    if (!any_tangent) return set_err(GRBDA_EINVAL, none);
    for (const Extent &e : out) {
        any_out = any_out || (no < asked && e.ptr);
        o[no] = e.ptr, o_bytes[no++] = e.bytes;
    }
    if (!any_out) return set_err(GRBDA_EINVAL, "no output asked for");
    if (dt && !std::isfinite(*dt)) return set_err(GRBDA_EINVAL, "dt is not finite");
    if (int rc = no_overlap(in, in_bytes, o, o_bytes)) return rc;
    if (stepping)
        if (int rc = step_vjp_plan(p, base)) return rc;
    if (diff_q && !analytic_covers(p) && !(step > 0)) return set_err(GRBDA_EINVAL, "step must be positive");
    return GRBDA_OK;
}
// The arrays of an entry point as its body declares them, in the order of HostStage: the caller's device arrays as they are, or -- the
// *_host_f64 variants -- a staged copy of every array that is given.  run(): the call, between the copies in and out where there are any.
struct ProductArrays {
    HostStage *stage;
    template <class T>
    const T *in(const T *a, size_t count) { return stage && a ? stage->in(a, count) : a; }
    template <class T>
    T *out(T *a, size_t count) { return stage && a ? stage->out(a, count) : a; }
    template <class Call>
    int run(Call call) { return stage ? stage->run(call) : call(); }
};
// The entry of the family, device and host arrays alike: a null plan, the call scope, the entry point's rules (rules(&base)), an empty
// batch, the device -- current before a host variant allocates anything on it --, then body(arrays, tables, base).
template <class Rules, class Body>
int product_entry(const grbda_plan *p, size_t B, int device, bool host, Rules rules, Body body)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    int base = -1;
    if (int rc = rules(&base)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    HostStage st;  // (holds nothing for device arrays)
    ProductArrays a{host ? &st : nullptr};
    return body(a, *t, base);
}
// `rows` arrays [B][nv] from a pool of the plan (work_step_vjp, work_step_jvp): not chunked -- they are the size of the inputs
template <class T>
int rows_slab(const grbda_plan *p, SlabPool &pool, size_t rows, size_t B, int device, void *stream, T **w)
{
    void *ptr = nullptr;
    if (int rc = ensure_work(p, pool, device, stream, rows * B * p->host.nv * sizeof(T) + 256, &ptr)) return rc;
    *w = static_cast<T *>(ptr);
    return GRBDA_OK;
}
// the quaternion base's cluster record on the device, null for a plan without one: what the two integrate kernels read the base's v_index
// from (the record of the fp64 layout: the cluster's v_index is the same in every layout)
const ClusterRec *base_record(const DeviceTables &t, int base) { return base >= 0 ? t.clusters[1] + base : nullptr; }

// The linearisation both products are built on, chunk by chunk through a slab of the plan (`pool`: work_vjp or work_jvp), and its stages
// on the states [b0, b0 + nb) of a chunk:
//   ydd_stage       forward: ydd = ABA(q, qd, tau), into the caller's ydd_out where it keeps one, into the slab otherwise
//   matrices_stage  d tau / d q and d tau / d qd at (q, qd, ydd) by id_derivs into the slab, row-major (ydd: the forward side's own, or x)
//   pair_stage      the zero-velocity pair r1 = F(q, 0, rhs), r0 = F(q, 0, 0), F the ABA (forward) or the RNEA: r1 - r0 is H^-1 rhs or
//                   H rhs.  The runs of a pair carry no gravity (run(), gravity = false): on plans without the spanning-tree route the
//                   second of them is then exactly zero and the first is not rounded against a bias it does not need.
// A stage enqueues nothing where need_ydd / need_d / need_pair says that no asked-for result needs it, so every result has the same bits in
// every subset.  carve(): wq, wqd: the matrix is wanted (its gradient is asked for, its tangent is given); wx: so is the pair of the inverse
// side (grad_ydd, dydd); with_mid: one more vector between r0 and ydd where matrices and pair meet (jvp_run).  Per state of the chunk: the
// matrices wanted; zeros and the two results of the pair; mid; ydd when the caller keeps none.
template <class T>
struct ProductWork {
    const grbda_plan *p;
    bool forward;
    const T *q, *qd, *x;  // the batch; x: tau (forward) or ydd
    T *ydd_out;           // forward: the caller's ydd, where it keeps one
    double step;
    int device;
    void *stream;
    bool need_d = false, need_pair = false, need_ydd = false;
    size_t chunk = 0;  // states per pass
    T *Mq = nullptr, *Mqd = nullptr, *zeros = nullptr, *r1 = nullptr, *r0 = nullptr, *mid = nullptr, *ydd_slab = nullptr;

    int carve(SlabPool &pool, bool wq, bool wqd, bool wx, bool with_mid, size_t B)
    {
        const size_t nv = p->host.nv, nn = nv * nv;
        need_d = wq || wqd;
        need_pair = forward || wx;
        need_ydd = forward && (need_d || ydd_out);
        const bool need_mid = with_mid && need_d && need_pair, own_ydd = need_ydd && !ydd_out;
        const size_t per_state = (wq ? nn : 0) + (wqd ? nn : 0) + (need_pair ? 3 * nv : 0) + (need_mid ? nv : 0) + (own_ydd ? nv : 0);
        const Chunk c = budgeted_chunk(p, pool, device, stream, 4096ull << 20, per_state * sizeof(T), B);
        void *wptr = nullptr;
        if (int rc = ensure_work(p, pool, device, stream, c.bytes, &wptr)) return rc;
        Carver<T> w(wptr, c.chunk * per_state);
        auto take = [&](bool wanted, size_t per) { return wanted ? w.take(c.chunk * per) : nullptr; };
        Mq = take(wq, nn), Mqd = take(wqd, nn), zeros = take(need_pair, nv), r1 = take(need_pair, nv), r0 = take(need_pair, nv);
        mid = take(need_mid, nv), ydd_slab = take(own_ydd, nv);
        assert(w.taken == w.cap);
        chunk = c.chunk;
        return GRBDA_OK;
    }
    T *ydd(size_t b0) const { return ydd_out ? ydd_out + b0 * p->host.nv : ydd_slab; }
    int ydd_stage(size_t b0, size_t nb) const
    {
        const size_t nv = p->host.nv;
        return need_ydd ? run<T>(p, false, q + b0 * p->host.nq, qd + b0 * nv, x + b0 * nv, nullptr, ydd(b0), nb, device, stream) : GRBDA_OK;
    }
    int matrices_stage(size_t b0, size_t nb) const
    {
        const size_t nv = p->host.nv;
        return need_d ? id_derivs<T>(p, q + b0 * p->host.nq, qd + b0 * nv, forward ? ydd(b0) : x + b0 * nv, step, Mq, Mqd, nb, device, stream) : GRBDA_OK;
    }
    int pair_stage(size_t b0, size_t nb, const T *rhs) const
    {
        if (!need_pair) return GRBDA_OK;
        const T *qc = q + b0 * p->host.nq;
        if (hipError_t e = hipMemsetAsync(zeros, 0, nb * p->host.nv * sizeof(T), static_cast<hipStream_t>(stream)); e != hipSuccess)
            return hip_err(e, "hipMemsetAsync");
        if (int rc = run<T>(p, !forward, qc, zeros, rhs, nullptr, r1, nb, device, stream, false)) return rc;
        return run<T>(p, !forward, qc, zeros, zeros, nullptr, r0, nb, device, stream, false);
    }
};

// ---- grbda_rnea_vjp_* / grbda_aba_vjp_* (include/grbda_hip_vjp.h; vjp_kernels.hip) ---------------------------------------------------------
// x: ydd / tau, g: the cotangent, grad_x: grad_ydd / grad_tau, ydd_out: the forward dynamics' optional result.
// Forward: mu = H^-1 g by the ABA pair, the matrices at ydd = ABA(q, qd, tau); grad_q = -mu^T d tau / d q, grad_qd = -mu^T d tau / d qd,
// grad_tau = mu (vjp_contract_kernel forms the difference of the pair and writes all three).  Inverse: the matrices at the caller's ydd
// contracted with g, and grad_ydd = H g by the RNEA pair.
template <class T>
int vjp_run(const grbda_plan *p, const DeviceTables &t, bool forward, const T *q, const T *qd, const T *x, const T *g, double step, T *grad_q, T *grad_qd,
            T *grad_x, T *ydd_out, size_t B, int device, void *stream)
{
    ProductWork<T> w{p, forward, q, qd, x, ydd_out, step, device, stream};
    if (int rc = w.carve(p->work_vjp, grad_q, grad_qd, grad_x, false, B)) return rc;
    const size_t nv = p->host.nv;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const int nvi = static_cast<int>(nv);
    for (const auto [b0, nb] : ChunkWalk{B, w.chunk}) {
        const T *gc = g + b0 * nv;
        T *oq = grad_q ? grad_q + b0 * nv : nullptr, *oqd = grad_qd ? grad_qd + b0 * nv : nullptr, *ox = grad_x ? grad_x + b0 * nv : nullptr;
        if (int rc = w.ydd_stage(b0, nb)) return rc;
        if (int rc = w.pair_stage(b0, nb, gc)) return rc;
        if (int rc = w.matrices_stage(b0, nb)) return rc;
        const VjpLaunch L = vjp_contract_launch(nvi, sizeof(T), t.n_cu, nb);
        hipError_t e = hipSuccess;
        if (forward) {
            e = launch_vjp_contract<T>(L, w.Mq, w.Mqd, w.r1, w.r0, T(-1), nvi, nb, oq, oqd, ox, hs);
        } else {
            if (ox) e = launch_vjp_contract<T>(L, nullptr, nullptr, w.r1, w.r0, T(1), nvi, nb, nullptr, nullptr, ox, hs);
            if (e == hipSuccess && w.need_d) e = launch_vjp_contract<T>(L, w.Mq, w.Mqd, gc, nullptr, T(1), nvi, nb, oq, oqd, nullptr, hs);
        }
        if (e != hipSuccess) return hip_err(e, "vjp contraction launch");
    }
    return GRBDA_OK;
}
template <class T>
int vjp(const grbda_plan *p, bool forward, const T *q, const T *qd, const T *x, const T *g, double step, T *grad_q, T *grad_qd, T *grad_x, T *ydd_out,
        size_t B, int device, void *stream, bool host = false)
{
    const auto rules = [&](int *) {
        const size_t bq = B * p->host.nq * sizeof(T), bv = B * p->host.nv * sizeof(T);
        return product_rules(p, {{q, bq}, {qd, bv}, {x, bv}, {g, bv}}, {}, nullptr, {{grad_q, bv}, {grad_qd, bv}, {grad_x, bv}, {ydd_out, bv}}, 3, nullptr,
                             false, grad_q, step, nullptr);
    };
    return product_entry(p, B, device, host, rules, [&](ProductArrays &a, const DeviceTables &t, int) {
        const size_t nq = p->host.nq, nv = p->host.nv;
        const T *bq = a.in(q, B * nq), *bqd = a.in(qd, B * nv), *bx = a.in(x, B * nv), *bg = a.in(g, B * nv);
        T *b1 = a.out(grad_q, B * nv), *b2 = a.out(grad_qd, B * nv), *b3 = a.out(grad_x, B * nv), *b4 = a.out(ydd_out, B * nv);
        return a.run([&] { return vjp_run<T>(p, t, forward, bq, bqd, bx, bg, step, b1, b2, b3, b4, B, device, stream); });
    });
}

// ---- vector-Jacobian products of integrate, step and rollout (include/grbda_hip_step_vjp.h; step_vjp_kernels.hip) ---------------------
template <class T>
hipError_t integrate_vjp_launch(const DeviceTables &t, int base, const T *qd_next, double dt, const T *g_q, const T *g_qd, T *grad_q, T *grad_qd,
                                T *grad_ydd, int nv, size_t B, void *stream)
{
    return launch_integrate_vjp<T>(base_record(t, base), qd_next, static_cast<T>(dt), g_q, g_qd, grad_q, grad_qd, grad_ydd, nv, B,
                                   static_cast<hipStream_t>(stream));
}
constexpr size_t kStepVjpRows = 5, kRolloutVjpRows = 10;  // [B][nv] arrays of the slab: one step's; with the loop's adjoints behind them
// The three stages of grbda_step_vjp_* (arguments checked, B > 0, device found); `w`: kStepVjpRows [B][nv] arrays.  Every sum is one
// launch of vjp_add_kernel, here and in the loop of the rollout.
template <class T>
int step_vjp_run(const grbda_plan *p, const DeviceTables &t, int base, const T *q, const T *qd, const T *tau, const T *qd_next, double dt, const T *g_q,
                 const T *g_qd, double step, T *grad_q, T *grad_qd, T *grad_tau, size_t B, int device, void *stream, T *w)
{
    const size_t n = B * p->host.nv;
    const int nvi = static_cast<int>(p->host.nv);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    T *i_q = grad_q ? w : nullptr, *i_qd = grad_qd ? w + n : nullptr, *g_ydd = w + 2 * n, *a_q = grad_q ? w + 3 * n : nullptr,
      *a_qd = grad_qd ? w + 4 * n : nullptr;
    if (hipError_t e = integrate_vjp_launch<T>(t, base, qd_next, dt, g_q, g_qd, i_q, i_qd, g_ydd, nvi, B, stream); e != hipSuccess)
        return hip_err(e, "integrate vjp launch");
    if (int rc = vjp_run<T>(p, t, true, q, qd, tau, g_ydd, step, a_q, a_qd, grad_tau, nullptr, B, device, stream)) return rc;
    hipError_t e = hipSuccess;
    if (grad_q) e = launch_vjp_add<T>(i_q, a_q, grad_q, n, hs);
    if (e == hipSuccess && grad_qd) e = launch_vjp_add<T>(i_qd, a_qd, grad_qd, n, hs);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "vjp add launch");
}
template <class T>
int integrate_vjp(const grbda_plan *p, const T *qd_next, double dt, const T *g_q, const T *g_qd, T *grad_q, T *grad_qd, T *grad_ydd, size_t B, int device,
                  void *stream)
{
    const auto rules = [&](int *base) {
        const size_t bv = B * p->host.nv * sizeof(T);
        return product_rules(p, {{qd_next, bv}}, {{g_q, bv}, {g_qd, bv}}, kNoCotangent, {{grad_q, bv}, {grad_qd, bv}, {grad_ydd, bv}}, 3, &dt, true, false,
                             0.0, base);
    };
    return product_entry(p, B, device, false, rules, [&](ProductArrays &, const DeviceTables &t, int base) {
        hipError_t e = integrate_vjp_launch<T>(t, base, qd_next, dt, g_q, g_qd, grad_q, grad_qd, grad_ydd, static_cast<int>(p->host.nv), B, stream);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "integrate vjp launch");
    });
}
template <class T>
int step_vjp(const grbda_plan *p, const T *q, const T *qd, const T *tau, const T *qd_next, double dt, const T *g_q, const T *g_qd, double step, T *grad_q,
             T *grad_qd, T *grad_tau, size_t B, int device, void *stream, bool host = false)
{
    const auto rules = [&](int *base) {  // (the step: where grbda_aba_vjp_* will take differences in q)
        const size_t bq = B * p->host.nq * sizeof(T), bv = B * p->host.nv * sizeof(T);
        return product_rules(p, {{q, bq}, {qd, bv}, {tau, bv}, {qd_next, bv}}, {{g_q, bv}, {g_qd, bv}}, kNoCotangent,
                             {{grad_q, bv}, {grad_qd, bv}, {grad_tau, bv}}, 3, &dt, true, grad_q, step, base);
    };
    return product_entry(p, B, device, host, rules, [&](ProductArrays &a, const DeviceTables &t, int base) {
        const size_t nq = p->host.nq, nv = p->host.nv;
        const T *bq = a.in(q, B * nq), *bqd = a.in(qd, B * nv), *bt = a.in(tau, B * nv), *bn = a.in(qd_next, B * nv);
        const T *bgq = a.in(g_q, B * nv), *bgqd = a.in(g_qd, B * nv);
        T *o1 = a.out(grad_q, B * nv), *o2 = a.out(grad_qd, B * nv), *o3 = a.out(grad_tau, B * nv);
        return a.run([&] {
            T *w = nullptr;
            if (int rc = rows_slab<T>(p, p->work_step_vjp, kStepVjpRows, B, device, stream, &w)) return rc;
            return step_vjp_run<T>(p, t, base, bq, bqd, bt, bn, dt, bgq, bgqd, step, o1, o2, o3, B, device, stream, w);
        });
    });
}
// The loop of grbda_step_vjp_* from state T back to state 0.  The adjoint lambda_k is the step's output gamma itself, or gamma + g[k] in a
// second pair of arrays where the caller has a cotangent for state k; the last step writes the caller's grad_q0 / grad_qd0.  grad_tau: the
// step writes row k, or -- one tau held for all steps -- the first step (k = T-1) writes grad_tau and every later one is added to it.
template <class T>
int rollout_vjp(const grbda_plan *p, const T *q0, const T *qd0, const T *q_traj, const T *qd_traj, const T *tau, int tau_steps, double dt, int n_steps,
                const T *g_q, const T *g_qd, int g_steps, double step, T *grad_q0, T *grad_qd0, T *grad_tau, size_t B, int device, void *stream)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    // (a missing state input and the three counts in front of the family's rules: the counts size the arrays)
    if (!q0 || !qd0 || !q_traj || !qd_traj || !tau) return set_err(GRBDA_EINVAL, "null argument");
    if (n_steps < 0) return set_err(GRBDA_EINVAL, "T is negative");
    if (tau_steps != 1 && tau_steps != n_steps) return set_err(GRBDA_EINVAL, "tau_steps must be 1 or T");
    if (g_steps != 1 && g_steps != n_steps) return set_err(GRBDA_EINVAL, "g_steps must be 1 or T");
    const size_t nq = p->host.nq, nv = p->host.nv, bq = B * nq * sizeof(T), bv = B * nv * sizeof(T), steps = static_cast<size_t>(n_steps);
    const size_t ts = static_cast<size_t>(tau_steps), gs = static_cast<size_t>(g_steps);
    int base = -1;
    // (the steps k >= 1 hand their position gradient on, whatever the caller asks of state 0)
    if (int rc = product_rules(p, {{q0, bq}, {qd0, bv}, {q_traj, steps * bq}, {qd_traj, steps * bv}, {tau, ts * bv}}, {{g_q, gs * bv}, {g_qd, gs * bv}},
                               kNoCotangent, {{grad_q0, bv}, {grad_qd0, bv}, {grad_tau, ts * bv}}, 3, &dt, true, grad_q0 || n_steps > 1, step, &base))
        return rc;
    if (B == 0 || n_steps == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    T *w = nullptr;
    if (int rc = rows_slab<T>(p, p->work_step_vjp, kRolloutVjpRows, B, device, stream, &w)) return rc;
    const size_t n = B * nv;
    T *gam_q = w + kStepVjpRows * n, *gam_qd = gam_q + n, *sum_q = gam_qd + n, *sum_qd = sum_q + n, *gam_tau = sum_qd + n;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const T *lam_q = g_q ? g_q + (g_steps > 1 ? (steps - 1) * n : 0) : nullptr, *lam_qd = g_qd ? g_qd + (g_steps > 1 ? (steps - 1) * n : 0) : nullptr;
    for (size_t k = steps; k-- > 0;) {
        const T *qk = k ? q_traj + (k - 1) * B * nq : q0, *qdk = k ? qd_traj + (k - 1) * n : qd0, *tk = tau + (tau_steps > 1 ? k * n : 0);
        T *oq = k ? gam_q : grad_q0, *oqd = k ? gam_qd : grad_qd0;
        T *otau = !grad_tau ? nullptr : (tau_steps > 1 ? grad_tau + k * n : (k == steps - 1 ? grad_tau : gam_tau));
        if (int rc = step_vjp_run<T>(p, *t, base, qk, qdk, tk, qd_traj + k * n, dt, lam_q, lam_qd, step, oq, oqd, otau, B, device, stream, w)) return rc;
        hipError_t e = hipSuccess;
        if (otau == gam_tau && grad_tau) e = launch_vjp_add<T>(grad_tau, gam_tau, grad_tau, n, hs);
        lam_q = gam_q;
        lam_qd = gam_qd;
        if (k && g_steps > 1) {  // (state k's own cotangent is row k - 1)
            if (e == hipSuccess && g_q) {
                e = launch_vjp_add<T>(gam_q, g_q + (k - 1) * n, sum_q, n, hs);
                lam_q = sum_q;
            }
            if (e == hipSuccess && g_qd) {
                e = launch_vjp_add<T>(gam_qd, g_qd + (k - 1) * n, sum_qd, n, hs);
                lam_qd = sum_qd;
            }
        }
        if (e != hipSuccess) return hip_err(e, "vjp add launch");
    }
    return GRBDA_OK;
}

// ---- Jacobian-vector products (include/grbda_hip_jvp.h; jvp_kernels.hip, integrate_jvp_kernel of step_vjp_kernels.hip) ----------------
// x: ydd / tau, dx: dydd / dtau, out: dtau_out / dydd_out, ydd_out: the forward dynamics' optional result.
// Inverse: the matrices of the given tangents at the caller's ydd, H dydd by the RNEA pair (vjp_contract_kernel without matrices forms the
// difference, into mid), and jvp_contract_kernel sums the rows against the tangents on top of it.  Forward: the matrices at
// ydd = ABA(q, qd, tau); r = dtau - d tau / d q dq - d tau / d qd dqd (the same kernel, sign -1, dtau added in, into mid); dydd = H^-1 r by
// the ABA pair.
template <class T>
int jvp_run(const grbda_plan *p, const DeviceTables &t, bool forward, const T *q, const T *qd, const T *x, const T *dq, const T *dqd, const T *dx,
            double step, T *out, T *ydd_out, size_t B, int device, void *stream)
{
    ProductWork<T> w{p, forward, q, qd, x, ydd_out, step, device, stream};
    if (int rc = w.carve(p->work_jvp, dq, dqd, dx, true, B)) return rc;
    const size_t nv = p->host.nv;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const int nvi = static_cast<int>(nv);
    for (const auto [b0, nb] : ChunkWalk{B, w.chunk}) {
        const T *dqc = dq ? dq + b0 * nv : nullptr, *dqdc = dqd ? dqd + b0 * nv : nullptr, *dxc = dx ? dx + b0 * nv : nullptr;
        T *oc = out + b0 * nv;
        const JvpLaunch J = jvp_contract_launch(nvi, sizeof(T), t.n_cu, nb);
        const VjpLaunch V = vjp_contract_launch(nvi, sizeof(T), t.n_cu, nb);
        if (int rc = w.ydd_stage(b0, nb)) return rc;
        if (int rc = w.matrices_stage(b0, nb)) return rc;
        const T *rhs = dxc;  // what the pair runs on: dydd; forward: dtau, or r once the rows are taken off it
        if (forward && w.need_d) {
            if (hipError_t e = launch_jvp_contract<T>(J, w.Mq, w.Mqd, dqc, dqdc, dxc, T(-1), nvi, nb, w.mid, hs); e != hipSuccess)
                return hip_err(e, "jvp contraction launch");
            rhs = w.mid;
        }
        if (int rc = w.pair_stage(b0, nb, rhs)) return rc;
        if (w.need_pair) {
            // (out_w = r1 - r0 and nothing else: the difference of the pair as vjp_run forms it)
            T *diff = !forward && w.need_d ? w.mid : oc;
            if (hipError_t e = launch_vjp_contract<T>(V, nullptr, nullptr, w.r1, w.r0, T(1), nvi, nb, nullptr, nullptr, diff, hs); e != hipSuccess)
                return hip_err(e, "pair difference launch");
        }
        if (!forward && w.need_d)  // (mid: null without a pair)
            if (hipError_t e = launch_jvp_contract<T>(J, w.Mq, w.Mqd, dqc, dqdc, w.mid, T(1), nvi, nb, oc, hs); e != hipSuccess)
                return hip_err(e, "jvp contraction launch");
    }
    return GRBDA_OK;
}
template <class T>
int jvp(const grbda_plan *p, bool forward, const T *q, const T *qd, const T *x, const T *dq, const T *dqd, const T *dx, double step, T *out, T *ydd_out,
        size_t B, int device, void *stream, bool host = false)
{
    const auto rules = [&](int *) {
        const size_t bq = B * p->host.nq * sizeof(T), bv = B * p->host.nv * sizeof(T);
        return product_rules(p, {{q, bq}, {qd, bv}, {x, bv}}, {{dq, bv}, {dqd, bv}, {dx, bv}}, kNoTangent, {{out, bv}, {ydd_out, bv}}, 1, nullptr, false, dq,
                             step, nullptr);
    };
    return product_entry(p, B, device, host, rules, [&](ProductArrays &a, const DeviceTables &t, int) {
        const size_t nq = p->host.nq, nv = p->host.nv;
        const T *bq = a.in(q, B * nq), *bqd = a.in(qd, B * nv), *bx = a.in(x, B * nv);
        const T *bdq = a.in(dq, B * nv), *bdqd = a.in(dqd, B * nv), *bdx = a.in(dx, B * nv);
        T *b1 = a.out(out, B * nv), *b2 = a.out(ydd_out, B * nv);
        return a.run([&] { return jvp_run<T>(p, t, forward, bq, bqd, bx, bdq, bdqd, bdx, step, b1, b2, B, device, stream); });
    });
}
template <class T>
hipError_t integrate_jvp_launch(const DeviceTables &t, int base, const T *qd_next, double dt, const T *dq, const T *dqd, const T *dydd, T *dq_next,
                                T *dqd_next, int nv, size_t B, void *stream)
{
    return launch_integrate_jvp<T>(base_record(t, base), qd_next, static_cast<T>(dt), dq, dqd, dydd, dq_next, dqd_next, nv, B,
                                   static_cast<hipStream_t>(stream));
}
template <class T>
int integrate_jvp(const grbda_plan *p, const T *qd_next, double dt, const T *dq, const T *dqd, const T *dydd, T *dq_next, T *dqd_next, size_t B, int device,
                  void *stream)
{
    const auto rules = [&](int *base) {
        const size_t bv = B * p->host.nv * sizeof(T);
        return product_rules(p, {{qd_next, bv}}, {{dq, bv}, {dqd, bv}, {dydd, bv}}, kNoTangent, {{dq_next, bv}, {dqd_next, bv}}, 2, &dt, true, false, 0.0,
                             base);
    };
    return product_entry(p, B, device, false, rules, [&](ProductArrays &, const DeviceTables &t, int base) {
        hipError_t e = integrate_jvp_launch<T>(t, base, qd_next, dt, dq, dqd, dydd, dq_next, dqd_next, static_cast<int>(p->host.nv), B, stream);
        return e == hipSuccess ? GRBDA_OK : hip_err(e, "integrate jvp launch");
    });
}
// The two stages of grbda_step_jvp_* (arguments checked, B > 0, device found): grbda_aba_jvp_* into the [B][nv] work array, then the
// integrate kernel on it.
template <class T>
int step_jvp_run(const grbda_plan *p, const DeviceTables &t, int base, const T *q, const T *qd, const T *tau, const T *qd_next, double dt, const T *dq,
                 const T *dqd, const T *dtau, double step, T *dq_next, T *dqd_next, size_t B, int device, void *stream)
{
    T *dydd = nullptr;
    if (int rc = rows_slab<T>(p, p->work_step_jvp, 1, B, device, stream, &dydd)) return rc;
    if (int rc = jvp_run<T>(p, t, true, q, qd, tau, dq, dqd, dtau, step, dydd, nullptr, B, device, stream)) return rc;
    hipError_t e = integrate_jvp_launch<T>(t, base, qd_next, dt, dq, dqd, dydd, dq_next, dqd_next, static_cast<int>(p->host.nv), B, stream);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "integrate jvp launch");
}
template <class T>
int step_jvp(const grbda_plan *p, const T *q, const T *qd, const T *tau, const T *qd_next, double dt, const T *dq, const T *dqd, const T *dtau, double step,
             T *dq_next, T *dqd_next, size_t B, int device, void *stream, bool host = false)
{
    const auto rules = [&](int *base) {
        const size_t bq = B * p->host.nq * sizeof(T), bv = B * p->host.nv * sizeof(T);
        return product_rules(p, {{q, bq}, {qd, bv}, {tau, bv}, {qd_next, bv}}, {{dq, bv}, {dqd, bv}, {dtau, bv}}, kNoTangent,
                             {{dq_next, bv}, {dqd_next, bv}}, 2, &dt, true, dq, step, base);
    };
    return product_entry(p, B, device, host, rules, [&](ProductArrays &a, const DeviceTables &t, int base) {
        const size_t nq = p->host.nq, nv = p->host.nv;
        const T *bq = a.in(q, B * nq), *bqd = a.in(qd, B * nv), *bt = a.in(tau, B * nv), *bn = a.in(qd_next, B * nv);
        const T *bdq = a.in(dq, B * nv), *bdqd = a.in(dqd, B * nv), *bdt = a.in(dtau, B * nv);
        T *o1 = a.out(dq_next, B * nv), *o2 = a.out(dqd_next, B * nv);
        return a.run([&] { return step_jvp_run<T>(p, t, base, bq, bqd, bt, bn, dt, bdq, bdqd, bdt, step, o1, o2, B, device, stream); });
    });
}

// the kernel of a route (choose_aba / choose_rnea) by name; the template arguments mirror the launchers' own dispatch in chain_kernels.hip
template <class T>
static std::string kernel_name_of(const grbda_plan *p, int kind, int n_cu, size_t B, bool interpreter = false)  // interpreter: that route's name, whatever the batch
{
    const HostPlan &h = p->host;
    const char *tn = sizeof(T) == 4 ? "float" : "double";
    const char *alg = kind == 0 ? "aba" : "rnea";
    const Route r = kind == 0 ? choose_aba<T>(p, n_cu, B, false) : choose_rnea<T>(p, n_cu, B, false);
    char buf[160];
    const auto format = [&](const auto &cp, int gen1_waves, bool inreg = false) {
        const int segs = !cp.gens.empty() ? 2 : (!cp.diffs.empty() ? 1 : 0);
        if (r.path == ROUTE_GEN1)
            std::snprintf(buf, sizeof buf, "grbda_hip::%s_gen1_kernel<%s, %d, %s, %d>", alg, tn, cp.gens[0].n, cp.gens[0].kind ? "true" : "false", gen1_waves);
        else if (r.path == ROUTE_LM)
            std::snprintf(buf, sizeof buf, "grbda_hip::%s_chain_lm_kernel<%s, %d%s>", alg, tn, r.lm_waves, cp.diffs.empty() ? "" : ", true");
        else if (kind == 0)
            std::snprintf(buf, sizeof buf, "grbda_hip::aba_chain_kernel<%s, %d, %d>", tn, (sizeof(T) == 8 && !cp.gens.empty()) ? 1 : 2,
                          inreg ? kModeInReg : segs);
        else
            std::snprintf(buf, sizeof buf, "grbda_hip::rnea_chain_kernel<%s, %d, %s>", tn, segs, cp.n_glb > 0 ? "true" : "false");
    };
    if (r.path == ROUTE_INTERPRETER || interpreter) {
        bool loop = false;
        for (const ClusterRec &cr : h.lay64.clusters) loop = loop || cr.kind == CK_LOOP;
        std::snprintf(buf, sizeof buf, "grbda_hip::%s_kernel<%s, %s>", alg, tn, loop ? "true" : "false");
    } else if (kind == 0) {
        const ChainProgram &cp = h.chain[r.slot];
        format(cp, r.path == ROUTE_GEN1 ? gen1_waves_per_simd<T>(cp.gens[0].n) : 0,
               chain_inputs_in_registers(sizeof(T), static_cast<int>(cp.gens.size()), static_cast<int>(cp.diffs.size()), cp.sv_global ? 1 : 0, h.nq, h.nv));
    } else {
        // (The four-wavefronts-per-SIMD route keeps the name of the two-per-SIMD program, as it always has: the batch-ladder tests compare
        // the names either side of a threshold.  Its own program may spill where that one does not -- Mini Cheetah then runs
        // rnea_chain_kernel<float, 0, true> under the name <float, 0, false>.)
        const RneaChainProgram &rp = h.rchain[r.slot == SLOT_F32_WIDE ? SLOT_F32 : r.slot];
        format(rp, r.path == ROUTE_GEN1 ? rnea_gen1_waves_per_simd<T>(rp.gens[0].n) : 0);
    }
    return buf;
}

// what a call with body wrenches launches for its dynamics (wrench_route): a wrench-carrying chain kernel, or the interpreter on the dense chunk
template <class T>
static int wrench_kernel_name_of(const grbda_plan *p, int kind, int n, const int *bodies, int frame, size_t B, int device, std::string &name)
{
    if (n < 0 || n > kMaxWrenches) return set_err(GRBDA_EINVAL, "0..16 body wrenches per call");
    if (frame != GRBDA_WRENCH_BODY && frame != GRBDA_WRENCH_WORLD) return set_err(GRBDA_EINVAL, "frame must be GRBDA_WRENCH_BODY or GRBDA_WRENCH_WORLD");
    if (n > 0 && !bodies) return set_err(GRBDA_EINVAL, "null argument");
    WrenchList<T> W{};
    W.n = n;
    for (int i = 0; i < n; i++) {
        if (bodies[i] < 0 || bodies[i] >= p->host.n_bodies) return set_err(GRBDA_EINVAL, "body index out of range");
        W.body[i] = bodies[i];
    }
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const char *tn = sizeof(T) == 4 ? "float" : "double";
    if (n == 0) {
        name = kernel_name_of<T>(p, kind, t->n_cu, B);
    } else if (wrench_route<T>(p, kind == 1, t->n_cu, B, W).path != ROUTE_CHAIN) {
        name = kernel_name_of<T>(p, kind, t->n_cu, B, true);
    } else if (kind == 0) {
        name = std::string("grbda_hip::aba_chain_wrench_kernel<") + tn + ">";
    } else {
        name = std::string("grbda_hip::rnea_chain_wrench_kernel<") + tn + (p->host.rchain[chain_slot(sizeof(T) == 8)].n_glb > 0 ? ", true>" : ", false>");
    }
    return GRBDA_OK;
}

// ---- one process, several devices: contiguous batch shards, plan replicated ------------------------
template <class T>
int run_sharded(const grbda_plan *p, bool rnea, const T *q, const T *qd, const T *x, T *out, size_t B, int n_gpus)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !qd || !x || !out) return set_err(GRBDA_EINVAL, "null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return set_err(GRBDA_ENODEVICE, "no HIP device available (there is no CPU fallback)");
    if (n_gpus < 1 || n_gpus > count) return set_err(GRBDA_EINVAL, "n_gpus out of range");
    if (B == 0) return GRBDA_OK;
    const size_t nq = p->host.nq, nv = p->host.nv;
    struct Shard {
        size_t b0 = 0, nb = 0;
        T *dq = nullptr, *dqd = nullptr, *dx = nullptr, *dout = nullptr;
        hipStream_t s = nullptr;
    };
    std::vector<Shard> sh(n_gpus);
    int rc = GRBDA_OK;
    hipError_t e = hipSuccess;
    for (int g = 0; g < n_gpus && rc == GRBDA_OK; g++) {
        Shard &S = sh[g];
        S.b0 = B * g / n_gpus;
        S.nb = B * (g + 1) / n_gpus - S.b0;
        if (S.nb == 0) continue;
        if ((e = hipSetDevice(g)) != hipSuccess || (e = hipStreamCreate(&S.s)) != hipSuccess ||
            (e = hipMalloc((void **)&S.dq, S.nb * nq * sizeof(T))) != hipSuccess ||
            (e = hipMalloc((void **)&S.dqd, S.nb * nv * sizeof(T))) != hipSuccess ||
            (e = hipMalloc((void **)&S.dx, S.nb * nv * sizeof(T))) != hipSuccess ||
            (e = hipMalloc((void **)&S.dout, S.nb * nv * sizeof(T))) != hipSuccess ||
            (e = hipMemcpyAsync(S.dq, q + S.b0 * nq, S.nb * nq * sizeof(T), hipMemcpyHostToDevice, S.s)) != hipSuccess ||
            (e = hipMemcpyAsync(S.dqd, qd + S.b0 * nv, S.nb * nv * sizeof(T), hipMemcpyHostToDevice, S.s)) != hipSuccess ||
            (e = hipMemcpyAsync(S.dx, x + S.b0 * nv, S.nb * nv * sizeof(T), hipMemcpyHostToDevice, S.s)) != hipSuccess) {
            rc = hip_err(e, "shard setup");
            break;
        }
        rc = run<T>(p, rnea, S.dq, S.dqd, S.dx, nullptr, S.dout, S.nb, g, S.s);
        if (rc == GRBDA_OK &&
            (e = hipMemcpyAsync(out + S.b0 * nv, S.dout, S.nb * nv * sizeof(T), hipMemcpyDeviceToHost, S.s)) != hipSuccess)
            rc = hip_err(e, "shard copy back");
    }
    for (int g = 0; g < n_gpus; g++) {
        Shard &S = sh[g];
        if (!S.s) continue;
        (void)hipSetDevice(g);
        if ((e = hipStreamSynchronize(S.s)) != hipSuccess && rc == GRBDA_OK) rc = hip_err(e, "shard execution");
        if (S.dq) (void)hipFree(S.dq);
        if (S.dqd) (void)hipFree(S.dqd);
        if (S.dx) (void)hipFree(S.dx);
        if (S.dout) (void)hipFree(S.dout);
        {   // the scratch slab this call made for its private stream goes with the stream
            std::lock_guard<std::recursive_mutex> lk(p->mu);
            auto it = p->scratch.find({g, S.s});
            if (it != p->scratch.end()) {
                if (it->second.ptr) (void)hipFree(it->second.ptr);
                p->scratch.erase(it);
            }
        }
        (void)hipStreamDestroy(S.s);
    }
    return rc;
}

// ---- one process, several devices, DEVICE-resident shards: launch every shard on its own device / stream, optionally gather the
// result slabs on the first device over the peer links (hipMemcpyPeerAsync: xGMI, no host hop).  Enqueues only.
template <class T>
int run_sharded_dev(const grbda_plan *p, bool rnea, int n_gpus, const int *devices, const T *const *q, const T *const *qd, const T *const *x,
                    T *const *out, const size_t *B, void *const *streams, T *gathered)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    if (n_gpus < 1 || !q || !qd || !x || !B || (!out && !gathered)) return set_err(GRBDA_EINVAL, "null argument or n_gpus < 1");
    GRBDA_CALL_SCOPE(p);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return set_err(GRBDA_ENODEVICE, "no HIP device available (there is no CPU fallback)");
    const size_t nv = p->host.nv;
    for (int g = 0; g < n_gpus; g++) {
        const int dev = devices ? devices[g] : g;
        if (dev < 0 || dev >= count) return set_err(GRBDA_EINVAL, "device index out of range");
        for (int h = 0; h < g; h++)
            if ((devices ? devices[h] : h) == dev && (streams ? streams[h] : nullptr) == (streams ? streams[g] : nullptr) && B[g] && B[h])
                return set_err(GRBDA_EINVAL, "two shards on one (device, stream): they would share one scratch slab -- give them distinct streams");
        if (B[g] && (!q[g] || !qd[g] || !x[g] || (!gathered && (!out || !out[g])))) return set_err(GRBDA_EINVAL, "null shard pointer");
    }
    const int dev0 = devices ? devices[0] : 0;
    void *const s0 = streams ? streams[0] : nullptr;
    size_t off = 0;
    hipError_t e = hipSuccess;
    for (int g = 0; g < n_gpus; g++) {
        const int dev = devices ? devices[g] : g;
        void *const sg = streams ? streams[g] : nullptr;
        const size_t nb = B[g];
        if (nb == 0) continue;
        // a shard on the gather device computes straight into its place of the gathered array
        T *dst = gathered ? gathered + off * nv : nullptr;
        T *o = (out && out[g]) ? out[g] : nullptr;
        if (gathered && dev == dev0 && !o) o = dst;
        if (!o) return set_err(GRBDA_EINVAL, "a shard on another device than the gather device needs its own output slab (out[g])");
        if (const int rc = run<T>(p, rnea, q[g], qd[g], x[g], nullptr, o, nb, dev, sg)) return rc;
        if (gathered && o != dst) {
            if ((e = hipSetDevice(dev)) != hipSuccess) return hip_err(e, "hipSetDevice");
            if (dev != dev0) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, dev, dev0) == hipSuccess && can) {
                    e = hipDeviceEnablePeerAccess(dev0, 0);  // (direct over the link; without it the runtime stages the copy)
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
                    (void)hipGetLastError();
                }
                e = hipMemcpyPeerAsync(dst, dev0, o, dev, nb * nv * sizeof(T), static_cast<hipStream_t>(sg));
            } else {
                e = hipMemcpyAsync(dst, o, nb * nv * sizeof(T), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(sg));
            }
            if (e != hipSuccess) return hip_err(e, "gather copy");
        }
        // the first shard's stream is the join point: work enqueued on it after this call sees every slab of `gathered`
        if (gathered && (dev != dev0 || sg != s0)) {
            hipEvent_t ev = nullptr;
            if ((e = hipSetDevice(dev)) != hipSuccess || (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess ||
                (e = hipEventRecord(ev, static_cast<hipStream_t>(sg))) != hipSuccess)
                return hip_err(e, "gather event");
            if ((e = hipSetDevice(dev0)) != hipSuccess || (e = hipStreamWaitEvent(static_cast<hipStream_t>(s0), ev, 0)) != hipSuccess) {
                (void)hipEventDestroy(ev);
                return hip_err(e, "gather join");
            }
            (void)hipEventDestroy(ev);  // (released by the runtime once the recorded work has completed)
        }
        off += nb;
    }
    return GRBDA_OK;
}

}  // namespace

extern "C" {

const char *grbda_strerror(int code)
{
    switch (code) {
        case GRBDA_OK: return "ok";
        case GRBDA_EINVAL: return "invalid argument or malformed model description";
        case GRBDA_EUNSUPPORTED: return "model feature not supported by the HIP kernels";
        case GRBDA_ENODEVICE: return "no usable HIP device";
        case GRBDA_EHIP: return "HIP runtime error";
        case GRBDA_ENOMEM: return "out of memory";
        case GRBDA_EPARSE: return "URDF parse error";
        case GRBDA_ESTATE: return "invalid spanning state";
        default: return "unknown error";
    }
}
const char *grbda_last_error(void) { return g_last_error.c_str(); }

// nv x nv, 1 where two velocity coordinates lie on one root path (same cluster, or one cluster an ancestor of the other): what
// DerivProgram::related holds as one 64-bit word per coordinate, for plans beyond 64 coordinates (manifold_kernels.hip, kernels 2w and 4)
static void build_related_table(HostPlan &h)
{
    const std::vector<ClusterRec> &cl = h.lay64.clusters;
    const int nc = static_cast<int>(cl.size()), nv = h.nv;
    std::vector<int> body_cluster(h.n_bodies, 0), parent(nc, -1);
    for (int c = 0; c < nc; c++)
        for (int i = 0; i < cl[c].k; i++) body_cluster[cl[c].first_body + i] = c;
    for (int c = 0; c < nc; c++) parent[c] = cl[c].parent_body >= 0 ? body_cluster[cl[c].parent_body] : -1;
    auto dof = [&](int c) { return cl[c].kind == CK_FREE ? 6 : cl[c].n; };
    h.related_table.assign(static_cast<size_t>(nv) * nv, 0);
    for (int c = 0; c < nc; c++)
        for (int a = c; a >= 0; a = parent[a])
            for (int i = 0; i < dof(c); i++)
                for (int j = 0; j < dof(a); j++) {
                    h.related_table[static_cast<size_t>(cl[c].v_index + i) * nv + cl[a].v_index + j] = 1;
                    h.related_table[static_cast<size_t>(cl[a].v_index + j) * nv + cl[c].v_index + i] = 1;
                }
}

}  // extern "C"

namespace {

// the GRBDA_* variables of INTEGRATION.md section 3 (PlanOptions): read once, when a plan is made
PlanOptions plan_options_from_env()
{
    PlanOptions o;
    auto flag = [](const char *name) { return env_int(name, 0) != 0; };
    auto clamp = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
    // launch shapes: GRBDA_LDS_BYTES_PER_WAVE / GRBDA_WAVES_PER_CU set all four kernels, the suffixed forms one of them
    static const char *const suffix[4] = {"_ABA32", "_ABA64", "_RNEA32", "_RNEA64"};
    for (int k = 0; k < 4; k++) {
        int v = env_int("GRBDA_LDS_BYTES_PER_WAVE", o.lds_bytes_per_wave[k]);
        v = env_int((std::string("GRBDA_LDS_BYTES_PER_WAVE") + suffix[k]).c_str(), v);
        o.lds_bytes_per_wave[k] = clamp(v, 0, 160 * 1024);
        int w = env_int("GRBDA_WAVES_PER_CU", o.waves_per_cu[k]);
        w = env_int((std::string("GRBDA_WAVES_PER_CU") + suffix[k]).c_str(), w);
        o.waves_per_cu[k] = clamp(w, 1, 32);
    }
    o.waves_per_cu_f64_wide_regs = clamp(env_int("GRBDA_WAVES_PER_CU_ABA64", env_int("GRBDA_WAVES_PER_CU", o.waves_per_cu_f64_wide_regs)), 1, 32);
    o.gen1_waves_cap = env_int("GRBDA_GEN1_WAVES_PER_CU", o.gen1_waves_cap);
    o.gen1_tiles_per_wave = env_int("GRBDA_GEN1_TILES_PER_WAVE", o.gen1_tiles_per_wave);
    o.lm_waves = env_int("GRBDA_LM_WAVES", o.lm_waves);
    o.minv_wpc = env_int("GRBDA_MINV_WPC", o.minv_wpc);
    o.deriv_waves = std::max(0, env_int("GRBDA_DERIV_WAVES_PER_CU", o.deriv_waves));
    o.crba_waves = env_int("GRBDA_CRBA_WAVES_PER_CU", o.crba_waves);
    if (o.crba_waves < 1 || o.crba_waves > 16) o.crba_waves = 16;
    // routes
    o.no_chain = flag("GRBDA_NO_CHAIN");
    o.no_latency_mode = flag("GRBDA_NO_LATENCY_MODE");
    o.no_gen1 = std::getenv("GRBDA_NO_GEN1") != nullptr;
    o.no_crba = flag("GRBDA_NO_CRBA");
    o.no_minv = flag("GRBDA_NO_MINV");
    o.solve_f64 = flag("GRBDA_SOLVE_F64");
    o.no_analytic = flag("GRBDA_NO_ANALYTIC");
    o.no_manifold = flag("GRBDA_NO_MANIFOLD");
    o.no_small_constraint = flag("GRBDA_NO_SMALL_CONSTRAINT");
    o.no_efpa = flag("GRBDA_NO_EFPA");
    o.no_projection = std::getenv("GRBDA_NO_PROJECTION") != nullptr;
    return o;
}

int plan_from_blob(const void *blob, size_t bytes, const PlanOptions &opt, grbda_plan **out)
{
    if (!out) return set_err(GRBDA_EINVAL, "null out pointer");
    *out = nullptr;
    std::unique_ptr<grbda_plan> p(new (std::nothrow) grbda_plan());
    if (!p) return set_err(GRBDA_ENOMEM, "allocation failed");
    char msg[256] = {0};
    p->opt = opt;
    int rc = compile_plan(blob, bytes, p->opt, p->host, msg, sizeof msg);
    if (rc) return set_err(rc, msg);
    p->blob.assign(static_cast<const unsigned char *>(blob), static_cast<const unsigned char *>(blob) + bytes);
    bool implicit = false;
    for (const ClusterRec &cr : p->host.lay64.clusters) implicit = implicit || cr.kind == CK_LOOP;
    // (plans with big clusters: up to 128 velocities -- tables instead of the one-word masks, build_related_table)
    if ((implicit || p->host.projection_only) && p->host.nv <= (p->host.big_clusters ? 2 * kWave : kWave)) {
        // the spanning-tree model for the derivatives on the constraint manifold (at most 64 spanning velocities: the masks of
        // DerivProgram::related)
        std::vector<unsigned char> sb;
        if (make_spanning_blob(blob, bytes, sb, p->span_q, p->span_v, msg, sizeof msg) == 0) {
            grbda_plan *sp = nullptr;
            if (plan_from_blob(sb.data(), sb.size(), p->opt, &sp) == GRBDA_OK) {
                if (sp->host.nv <= (p->host.big_clusters ? 2 * kWave : kWave) && sp->host.deriv.ok) {
                    p->span = sp;
                    if (p->host.nv > kWave || sp->host.nv > kWave) {
                        build_related_table(p->host);
                        build_related_table(sp->host);
                    }
                    std::memcpy(sp->host.gravity, p->host.gravity, sizeof sp->host.gravity);
                    p->crow.assign(p->host.n_clusters, 0);
                    int rows = 0;
                    for (int c = 0; c < p->host.n_clusters; c++) {
                        const ClusterRec &cr = p->host.lay64.clusters[c];
                        p->crow[c] = rows;
                        if (cr.kind == CK_LOOP) rows += cr.k * (p->host.big_clusters ? cr.n : cr.n * (4 + cr.n));  // (manifold_kernels.hip, cpl_stride)
                        else if (cr.kind == CK_STATIC && p->host.big_clusters) rows += cr.k * cr.n;  // (wide plans keep every cluster's G rows in the slab)
                    }
                    p->n_cpl_rows = rows;
                    // (every implicit cluster within 4 bodies / 2 independent coordinates: the constraint kernel's half-size build)
                    bool small = !p->host.big_clusters;
                    for (int c = 0; c < p->host.n_clusters; c++) {
                        const ClusterRec &cr = p->host.lay64.clusters[c];
                        if (cr.kind == CK_LOOP && (cr.k > 4 || cr.n > 2)) small = false;
                        if (cr.kind == CK_LOOP && cr.cons_type != 0) p->has_trig = true;
                    }
                    p->constraint_shape = p->host.big_clusters ? 1 : (small && !p->opt.no_small_constraint ? 2 : 0);
                } else {
                    grbda_plan_free(sp);
                }
            }
        }
    }
    *out = p.release();
    return GRBDA_OK;
}

}  // namespace

extern "C" {

int grbda_plan_from_blob(const void *blob, size_t bytes, grbda_plan **out)
{
    return plan_from_blob(blob, bytes, plan_options_from_env(), out);
}

int grbda_urdf_to_blob(const char *const *paths, int n_paths, int ori_repr, void *buf, size_t cap, size_t *needed)
{
    if (!paths || n_paths <= 0) return set_err(GRBDA_EINVAL, "no URDF path");
    std::vector<unsigned char> blob;
    std::string err;
    int rc = urdf_to_blob(paths, n_paths, ori_repr, blob, err);
    if (rc) return set_err(rc, err);
    if (needed) *needed = blob.size();
    if (buf) {
        if (cap < blob.size()) return set_err(GRBDA_EINVAL, "buffer too small");
        std::memcpy(buf, blob.data(), blob.size());
    }
    return GRBDA_OK;
}

int grbda_plan_from_urdf(const char *path, int ori_repr, grbda_plan **out)
{
    if (!path || !out) return set_err(GRBDA_EINVAL, "null argument");
    std::vector<unsigned char> blob;
    std::string err;
    const char *paths[1] = {path};
    int rc = urdf_to_blob(paths, 1, ori_repr, blob, err);
    if (rc) return set_err(rc, err);
    return grbda_plan_from_blob(blob.data(), blob.size(), out);
}

void grbda_plan_free(grbda_plan *p)
{
    if (!p) return;
    DeviceGuard device_guard_;
    for (auto &kv : p->dev) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        DeviceTables &t = kv.second;
        (void)hipFree(t.aba_steps); (void)hipFree(t.rnea_steps); (void)hipFree(t.consts64); (void)hipFree(t.consts32);
        (void)hipFree(t.cints); (void)hipFree(t.dq_map); (void)hipFree(t.crba_bodies); (void)hipFree(t.deriv_bodies); (void)hipFree(t.deriv_related); (void)hipFree(t.related_table); (void)hipFree(t.minv_bodies); (void)hipFree(t.minv_coltab);
        (void)hipFree(t.span_q); (void)hipFree(t.span_v); (void)hipFree(t.crow);
        (void)hipFree(t.centroidal_rows);
        for (int w = 0; w < kChainSlots; w++) {
            free_chain_tables(t.rchain[w]);
            free_chain_tables(t.chain[w]);
        }
        for (int w = 0; w < kLayouts; w++) { (void)hipFree(t.acc_k[w]); (void)hipFree(t.clusters[w]); (void)hipFree(t.rnea_clusters[w]); (void)hipFree(t.bodies[w]); (void)hipFree(t.rnea_bodies[w]); }
    }
    for (auto *m : {&p->scratch, &p->work, &p->work_cvt, &p->work_proj, &p->work_vjp, &p->work_step_vjp, &p->work_jvp, &p->work_step_jvp, &p->work_contact})
        for (auto &kv : *m) {
            if (hipSetDevice(kv.first.first) != hipSuccess) continue;
            if (kv.second.ptr) (void)hipFree(kv.second.ptr);
        }
    delete p;
}

// A stream that is capturing must not lose a buffer its graph refers to, and hipFree would wait for the capture: every slab of the plan
// (and of its spanning-tree plan) is checked first, so that a refused release frees nothing.
static bool holds_capturing_slab(const grbda_plan *p)
{
    for (auto *m : {&p->work, &p->work_cvt, &p->work_proj, &p->work_vjp, &p->work_step_vjp, &p->work_jvp, &p->work_step_jvp, &p->work_contact})
        for (auto &kv : *m)
            if (kv.second.ptr && is_capturing(kv.first.second)) return true;
    return p->span && holds_capturing_slab(p->span);
}

int grbda_plan_release_work(grbda_plan *p, unsigned long long *bytes_released)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (holds_capturing_slab(p))
        return set_err(GRBDA_EINVAL, "a stream of this plan is capturing: its work buffers cannot be released now");
    unsigned long long total = 0;
    for (auto *m : {&p->work, &p->work_cvt, &p->work_proj, &p->work_vjp, &p->work_step_vjp, &p->work_jvp, &p->work_step_jvp, &p->work_contact})
        for (auto &kv : *m) {
            if (!kv.second.ptr) continue;
            hipError_t e = hipSetDevice(kv.first.first);
            if (e != hipSuccess) return hip_err(e, "hipSetDevice");
            if ((e = hipFree(kv.second.ptr)) != hipSuccess) return hip_err(e, "hipFree");  // (waits for the work enqueued on it)
            total += kv.second.bytes;
            kv.second.ptr = nullptr;
            kv.second.bytes = 0;
        }
    if (p->span) {
        unsigned long long more = 0;
        if (const int rc = grbda_plan_release_work(p->span, &more)) return rc;
        total += more;
    }
    if (bytes_released) *bytes_released = total;
    return GRBDA_OK;
}

int grbda_plan_dims(const grbda_plan *p, int *nq, int *nv, int *n_bodies, int *n_clusters)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    if (nq) *nq = p->host.nq;
    if (nv) *nv = p->host.nv;
    if (n_bodies) *n_bodies = p->host.n_bodies;
    if (n_clusters) *n_clusters = p->host.n_clusters;
    return GRBDA_OK;
}

int grbda_plan_set_gravity(grbda_plan *p, const double g[3])
{
    if (!p || !g) return set_err(GRBDA_EINVAL, "null argument");
    for (int i = 0; i < 3; i++) p->host.gravity[3 + i] = g[i];
    if (p->span) grbda_plan_set_gravity(p->span, g);
    // keep the stored description in sync so that grbda_plan_blob() round-trips
    std::memcpy(reinterpret_cast<grbda_desc_header *>(p->blob.data())->gravity, p->host.gravity, sizeof(double) * 6);
    return GRBDA_OK;
}
int grbda_plan_get_gravity(const grbda_plan *p, double g[3])
{
    if (!p || !g) return set_err(GRBDA_EINVAL, "null argument");
    for (int i = 0; i < 3; i++) g[i] = p->host.gravity[3 + i];
    return GRBDA_OK;
}

int grbda_plan_blob(const grbda_plan *p, const void **blob, size_t *bytes)
{
    if (!p || !blob || !bytes) return set_err(GRBDA_EINVAL, "null argument");
    *blob = p->blob.data();
    *bytes = p->blob.size();
    return GRBDA_OK;
}

int grbda_plan_info(const grbda_plan *p, grbda_plan_info_t *info)
{
    if (!p || !info) return set_err(GRBDA_EINVAL, "null argument");
    std::memset(info, 0, sizeof *info);
    info->n_slots = p->host.lay32.n_lds_aba + p->host.lay32.n_glb_aba;
    info->n_lds_slots_f32 = p->host.lay32.n_lds_aba;
    info->n_lds_slots_f64 = p->host.lay64.n_lds_aba;
    info->lds_bytes_f32 = static_cast<size_t>(info->n_lds_slots_f32) * kWave * 4;
    info->lds_bytes_f64 = static_cast<size_t>(info->n_lds_slots_f64) * kWave * 8;
    info->scratch_bytes_per_wave_f32 = static_cast<size_t>(p->host.lay32.n_glb_aba) * kWave * 4;
    info->scratch_bytes_per_wave_f64 = static_cast<size_t>(p->host.lay64.n_glb_aba) * kWave * 8;
    info->flops_aba = p->host.flops_aba;
    info->flops_rnea = p->host.flops_rnea;
    info->bytes_aba_f32 = (p->host.nq + 3.0 * p->host.nv) * 4;
    info->bytes_aba_f64 = (p->host.nq + 3.0 * p->host.nv) * 8;
    for (const BodyRec &b : p->host.lay32.bodies) info->n_axisym_bodies += b.axisym;
    for (const ClusterRec &c : p->host.lay32.clusters) info->n_carry_clusters += c.carry_out;
    info->split_aba_f32 = p->host.lay32s.split_aba;
    info->split_rnea_f32 = p->host.lay32s.split_rnea;
    info->n_lds_slots_split_f32 = p->host.lay32s.n_lds_aba;
    info->chain_aba_f32 = p->host.chain[SLOT_F32].ok && !p->opt.no_chain;
    info->n_lds_slots_chain_f32 = p->host.chain[SLOT_F32].n_lds;
    info->n_chain_segments = static_cast<int>(p->host.chain[SLOT_F32].segs.size());
    info->chain_aba_f64 = p->host.chain[SLOT_F64].ok && !p->opt.no_chain;
    info->chain_rnea_f32 = p->host.rchain[SLOT_F32].ok && !p->opt.no_chain;
    info->chain_rnea_f64 = p->host.rchain[SLOT_F64].ok && !p->opt.no_chain;
    info->analytic_derivatives = (analytic_covers(p) || manifold_covers(p)) ? 1 : 0;
    info->n_chain_differentials = p->opt.no_chain ? 0 : static_cast<int>(p->host.chain[SLOT_F32].diffs.size());
    info->latency_mode_f32 = p->host.chain[SLOT_LM2_F32].ok && !p->opt.no_chain && !p->opt.no_latency_mode;
    info->latency_mode_f64 = p->host.chain[SLOT_LM2_F64].ok && !p->opt.no_chain && !p->opt.no_latency_mode;
    info->n_chain_generic = p->opt.no_chain ? 0 : static_cast<int>(p->host.chain[SLOT_F32].gens.size());
    info->spanning_tree_route = p->host.projection_only ? 1 : 0;
    return GRBDA_OK;
}

int grbda_aba_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *f_ext,
                  double *ydd, size_t B, int device, void *stream)
{
    return run<double>(p, false, q, qd, tau, f_ext, ydd, B, device, stream);
}
int grbda_aba_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, const float *f_ext,
                  float *ydd, size_t B, int device, void *stream)
{
    return run<float>(p, false, q, qd, tau, f_ext, ydd, B, device, stream);
}
int grbda_rnea_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, const double *f_ext,
                   double *tau, size_t B, int device, void *stream)
{
    return run<double>(p, true, q, qd, ydd, f_ext, tau, B, device, stream);
}
int grbda_rnea_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, const float *f_ext,
                   float *tau, size_t B, int device, void *stream)
{
    return run<float>(p, true, q, qd, ydd, f_ext, tau, B, device, stream);
}

int grbda_bias_f64(const grbda_plan *p, const double *q, const double *qd, const double *f_ext, double *out, size_t B, int device, void *stream)
{
    return derived<double>(p, DM_BIAS, q, qd, nullptr, f_ext, out, B, device, stream);
}
int grbda_bias_f32(const grbda_plan *p, const float *q, const float *qd, const float *f_ext, float *out, size_t B, int device, void *stream)
{
    return derived<float>(p, DM_BIAS, q, qd, nullptr, f_ext, out, B, device, stream);
}
int grbda_mass_matrix_f64(const grbda_plan *p, const double *q, double *H, size_t B, int device, void *stream)
{
    return mass_matrix<double>(p, q, H, B, device, stream);
}
int grbda_mass_matrix_f32(const grbda_plan *p, const float *q, float *H, size_t B, int device, void *stream)
{
    return mass_matrix<float>(p, q, H, B, device, stream);
}
int grbda_fd_dtau_f64(const grbda_plan *p, const double *q, double *Hinv, size_t B, int device, void *stream)
{
    return fd_dtau<double>(p, q, Hinv, B, device, stream);
}
int grbda_fd_dtau_f32(const grbda_plan *p, const float *q, float *Hinv, size_t B, int device, void *stream)
{
    return fd_dtau<float>(p, q, Hinv, B, device, stream);
}
int grbda_fd_dqd_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, double *J, size_t B, int device, void *stream)
{
    return fd_dqd<double>(p, q, qd, tau, J, B, device, stream);
}
int grbda_fd_dqd_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, float *J, size_t B, int device, void *stream)
{
    return fd_dqd<float>(p, q, qd, tau, J, B, device, stream);
}
int grbda_fd_dq_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, double step, double *J, size_t B, int device, void *stream)
{
    return fd_dq<double>(p, q, qd, tau, step, J, B, device, stream);
}
int grbda_fd_dq_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, double step, float *J, size_t B, int device, void *stream)
{
    return fd_dq<float>(p, q, qd, tau, step, J, B, device, stream);
}
int grbda_fd_derivatives_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, double *dq, double *dqd, double *dtau, size_t B, int device, void *stream)
{
    return fd_derivatives<double>(p, q, qd, tau, dq, dqd, dtau, B, device, stream);
}
int grbda_fd_derivatives_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, float *dq, float *dqd, float *dtau, size_t B, int device, void *stream)
{
    return fd_derivatives<float>(p, q, qd, tau, dq, dqd, dtau, B, device, stream);
}
int grbda_rnea_derivatives_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double step, double *dtau_dq,
                               double *dtau_dqd, double *dtau_dydd, size_t B, int device, void *stream)
{
    return rnea_derivatives<double>(p, q, qd, ydd, step, dtau_dq, dtau_dqd, dtau_dydd, B, device, stream);
}
int grbda_rnea_derivatives_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, double step, float *dtau_dq,
                               float *dtau_dqd, float *dtau_dydd, size_t B, int device, void *stream)
{
    return rnea_derivatives<float>(p, q, qd, ydd, step, dtau_dq, dtau_dqd, dtau_dydd, B, device, stream);
}
int grbda_kernel_name(const grbda_plan *p, int kind, int precision, size_t B, int device, char *buf, size_t cap)
{
    if (!p || !buf || cap == 0 || (kind != 0 && kind != 1) || (precision != 32 && precision != 64)) return set_err(GRBDA_EINVAL, "bad argument");
    GRBDA_CALL_SCOPE(p);
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const std::string name = precision == 32 ? kernel_name_of<float>(p, kind, t->n_cu, B) : kernel_name_of<double>(p, kind, t->n_cu, B);
    std::snprintf(buf, cap, "%s", name.c_str());
    return GRBDA_OK;
}
int grbda_aba_wrench_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, int n, const int *bodies, const double *wrench,
                         int frame, double *ydd, size_t B, int device, void *stream)
{
    return wrench_run<double>(p, false, q, qd, tau, n, bodies, wrench, frame, ydd, B, device, stream);
}
int grbda_aba_wrench_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, int n, const int *bodies, const float *wrench,
                         int frame, float *ydd, size_t B, int device, void *stream)
{
    return wrench_run<float>(p, false, q, qd, tau, n, bodies, wrench, frame, ydd, B, device, stream);
}
int grbda_rnea_wrench_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, int n, const int *bodies, const double *wrench,
                          int frame, double *tau, size_t B, int device, void *stream)
{
    return wrench_run<double>(p, true, q, qd, ydd, n, bodies, wrench, frame, tau, B, device, stream);
}
int grbda_rnea_wrench_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, int n, const int *bodies, const float *wrench,
                          int frame, float *tau, size_t B, int device, void *stream)
{
    return wrench_run<float>(p, true, q, qd, ydd, n, bodies, wrench, frame, tau, B, device, stream);
}
int grbda_aba_wrench_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, int n, const int *bodies,
                              const double *wrench, int frame, double *ydd, size_t B, int device)
{
    return wrench_host_f64(p, false, q, qd, tau, n, bodies, wrench, frame, ydd, B, device);
}
int grbda_rnea_wrench_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, int n, const int *bodies,
                               const double *wrench, int frame, double *tau, size_t B, int device)
{
    return wrench_host_f64(p, true, q, qd, ydd, n, bodies, wrench, frame, tau, B, device);
}
int grbda_wrench_kernel_name(const grbda_plan *p, int algo, int precision, int n, const int *bodies, int frame, size_t B, int device, char *buf,
                             size_t cap)
{
    if (!p || !buf || cap == 0 || (algo != 0 && algo != 1) || (precision != 32 && precision != 64)) return set_err(GRBDA_EINVAL, "bad argument");
    GRBDA_CALL_SCOPE(p);
    std::string name;
    if (int rc = precision == 32 ? wrench_kernel_name_of<float>(p, algo, n, bodies, frame, B, device, name)
                                 : wrench_kernel_name_of<double>(p, algo, n, bodies, frame, B, device, name))
        return rc;
    std::snprintf(buf, cap, "%s", name.c_str());
    return GRBDA_OK;
}
int grbda_spd_bad_pivots(int device, unsigned long long *count, int reset)
{
    if (!count) return set_err(GRBDA_EINVAL, "null argument");
    DeviceGuard device_guard_;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_err(GRBDA_ENODEVICE, "no HIP device available");
    if (device < 0 || device >= n) return set_err(GRBDA_EINVAL, "device index out of range");
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = spd_bad_pivots(count, reset);
    return e == hipSuccess ? GRBDA_OK : hip_err(e, "grbda_spd_bad_pivots");
}
int grbda_body_twists_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double *V, size_t B, int device,
                          void *stream)
{
    return twists<double>(p, q, qd, ydd, V, B, device, stream);
}
int grbda_body_twists_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, float *V, size_t B, int device,
                          void *stream)
{
    return twists<float>(p, q, qd, ydd, V, B, device, stream);
}
int grbda_body_poses_list_f64(const grbda_plan *p, const double *q, int n, const int *bodies, double *Xa_list, size_t B, int device, void *stream)
{
    return body_list_run<double>(p, false, q, nullptr, nullptr, n, bodies, Xa_list, B, device, stream);
}
int grbda_body_poses_list_f32(const grbda_plan *p, const float *q, int n, const int *bodies, float *Xa_list, size_t B, int device, void *stream)
{
    return body_list_run<float>(p, false, q, nullptr, nullptr, n, bodies, Xa_list, B, device, stream);
}
int grbda_body_poses_list_host_f64(const grbda_plan *p, const double *q, int n, const int *bodies, double *Xa_list, size_t B, int device)
{
    return body_list_host_f64(p, false, q, nullptr, nullptr, n, bodies, Xa_list, B, device);
}
int grbda_body_twists_list_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, int n, const int *bodies, double *V_list,
                               size_t B, int device, void *stream)
{
    return body_list_run<double>(p, true, q, qd, ydd, n, bodies, V_list, B, device, stream);
}
int grbda_body_twists_list_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, int n, const int *bodies, float *V_list,
                               size_t B, int device, void *stream)
{
    return body_list_run<float>(p, true, q, qd, ydd, n, bodies, V_list, B, device, stream);
}
int grbda_body_twists_list_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, int n, const int *bodies,
                                    double *V_list, size_t B, int device)
{
    return body_list_host_f64(p, true, q, qd, ydd, n, bodies, V_list, B, device);
}
int grbda_body_list_walk(const grbda_plan *p, int n, const int *bodies, int *walk_len, int *max_saved, int *route)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = body_list_check(p, n, bodies, bodies)) return rc;
    const BodyWalkHost H = build_body_walk(p->host, p->host.lay64, n, bodies);
    if (walk_len) *walk_len = H.walk_len;
    if (max_saved) *max_saved = H.max_saved;
    if (route) *route = H.route;
    return GRBDA_OK;
}
int grbda_frame_jacobians_f64(const grbda_plan *p, const double *q, const double *qd, int n, const int *bodies, const double *offsets, int frame,
                              double *J, double *drift, size_t B, int device, void *stream)
{
    return frame_jacobians_run<double>(p, q, qd, n, bodies, offsets, frame, J, drift, B, device, stream);
}
int grbda_frame_jacobians_f32(const grbda_plan *p, const float *q, const float *qd, int n, const int *bodies, const double *offsets, int frame,
                              float *J, float *drift, size_t B, int device, void *stream)
{
    return frame_jacobians_run<float>(p, q, qd, n, bodies, offsets, frame, J, drift, B, device, stream);
}
int grbda_frame_jacobians_host_f64(const grbda_plan *p, const double *q, const double *qd, int n, const int *bodies, const double *offsets,
                                   int frame, double *J, double *drift, size_t B, int device)
{
    return frame_jacobians_host_f64(p, q, qd, n, bodies, offsets, frame, J, drift, B, device);
}
int grbda_frame_jacobians_route(const grbda_plan *p, int n, const int *bodies, int *route, int *walk_len, int *max_saved)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = body_list_check(p, n, bodies, bodies)) return rc;
    const JacWalkHost H = build_jac_walk(p->host, p->host.lay64, n, bodies);
    if (route) *route = H.route;
    if (walk_len) *walk_len = H.walk_len;
    if (max_saved) *max_saved = H.max_saved;
    return GRBDA_OK;
}
int grbda_frame_jacobian_products_f64(const grbda_plan *p, const double *q, const double *v, const double *f, int n, const int *bodies,
                                      const double *offsets, int frame, double *Jv, double *JTf, size_t B, int device, void *stream)
{
    return frame_products_run<double>(p, q, v, f, n, bodies, offsets, frame, Jv, JTf, B, device, stream);
}
int grbda_frame_jacobian_products_f32(const grbda_plan *p, const float *q, const float *v, const float *f, int n, const int *bodies,
                                      const double *offsets, int frame, float *Jv, float *JTf, size_t B, int device, void *stream)
{
    return frame_products_run<float>(p, q, v, f, n, bodies, offsets, frame, Jv, JTf, B, device, stream);
}
int grbda_frame_jacobian_products_host_f64(const grbda_plan *p, const double *q, const double *v, const double *f, int n, const int *bodies,
                                           const double *offsets, int frame, double *Jv, double *JTf, size_t B, int device)
{
    return frame_products_host_f64(p, q, v, f, n, bodies, offsets, frame, Jv, JTf, B, device);
}
int grbda_body_poses_f64(const grbda_plan *p, const double *q, double *Xa, size_t B, int device, void *stream)
{
    return poses<double>(p, q, Xa, B, device, stream);
}
int grbda_body_poses_f32(const grbda_plan *p, const float *q, float *Xa, size_t B, int device, void *stream)
{
    return poses<float>(p, q, Xa, B, device, stream);
}
int grbda_apply_test_force_f64(const grbda_plan *p, const double *q, int body, const double offset[3], const double *force,
                               double *lambda_inv, double *dstate, size_t B, int device, void *stream)
{
    return test_force<double>(p, q, body, offset, force, lambda_inv, dstate, B, device, stream);
}
int grbda_apply_test_force_f32(const grbda_plan *p, const float *q, int body, const double offset[3], const float *force,
                               float *lambda_inv, float *dstate, size_t B, int device, void *stream)
{
    return test_force<float>(p, q, body, offset, force, lambda_inv, dstate, B, device, stream);
}
int grbda_inv_osim_f64(const grbda_plan *p, const double *q, int n_contacts, const int *bodies, const double *offsets,
                       double *Linv, double *J, size_t B, int device, void *stream)
{
    return inv_osim<double>(p, q, n_contacts, bodies, offsets, Linv, J, B, device, stream);
}
int grbda_inv_osim_f32(const grbda_plan *p, const float *q, int n_contacts, const int *bodies, const double *offsets,
                       float *Linv, float *J, size_t B, int device, void *stream)
{
    return inv_osim<float>(p, q, n_contacts, bodies, offsets, Linv, J, B, device, stream);
}
int grbda_contact_points_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, int n_contacts, const int *bodies,
                             const double *offsets, double *pos, double *vel, double *acc, size_t B, int device, void *stream)
{
    return contact_points<double>(p, q, qd, ydd, n_contacts, bodies, offsets, pos, vel, acc, B, device, stream);
}
int grbda_contact_points_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, int n_contacts, const int *bodies,
                             const double *offsets, float *pos, float *vel, float *acc, size_t B, int device, void *stream)
{
    return contact_points<float>(p, q, qd, ydd, n_contacts, bodies, offsets, pos, vel, acc, B, device, stream);
}
int grbda_contact_dynamics_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *f_ext, int n_contacts,
                               const int *bodies, const double *offsets, const double *a_des, double damping, double *ydd, double *lambda,
                               double *ydd_free, size_t B, int device, void *stream)
{
    return contact_dynamics<double>(p, q, qd, tau, f_ext, n_contacts, bodies, offsets, a_des, damping, ydd, lambda, ydd_free, B, device, stream);
}
int grbda_contact_dynamics_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, const float *f_ext, int n_contacts,
                               const int *bodies, const double *offsets, const float *a_des, double damping, float *ydd, float *lambda,
                               float *ydd_free, size_t B, int device, void *stream)
{
    return contact_dynamics<float>(p, q, qd, tau, f_ext, n_contacts, bodies, offsets, a_des, damping, ydd, lambda, ydd_free, B, device, stream);
}
int grbda_contact_solve_launch(int n_contacts, int precision, int device, int *lanes, size_t *lds_bytes, size_t *grid_cap)
{
    if (!lanes || !lds_bytes || !grid_cap || (precision != 32 && precision != 64)) return set_err(GRBDA_EINVAL, "bad argument");
    if (int rc = contact_count(n_contacts, "points")) return rc;
    const ContactSolveLaunch L = contact_solve_launch(n_contacts, precision == 32 ? sizeof(float) : sizeof(double));
    if (L.lanes == 0) return set_err(GRBDA_EINVAL, "the contact solve does not fit the LDS");
    int n_cu = 1;
    if (device >= 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_err(GRBDA_ENODEVICE, "no HIP device available");
        if (device >= n) return set_err(GRBDA_EINVAL, "device index out of range");
        if (hipError_t e = device_cu_count(device, &n_cu); e != hipSuccess) return hip_err(e, "hipGetDeviceProperties");
    }
    *lanes = L.lanes;
    *lds_bytes = L.lds_bytes;
    *grid_cap = static_cast<size_t>(n_cu) * L.per_cu;
    return GRBDA_OK;
}
int grbda_contact_points_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, int n_contacts, const int *bodies,
                                  const double *offsets, double *pos, double *vel, double *acc, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<double> cs;
    if (int rc = contact_points_args<double>(p, q, qd, ydd, n_contacts, bodies, offsets, pos, vel, acc, B, cs)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, no = B * static_cast<size_t>(n_contacts) * 3;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = qd ? st.in(qd, B * nv) : nullptr, *dy = ydd ? st.in(ydd, B * nv) : nullptr;
    double *dp = pos ? st.out(pos, no) : nullptr, *dv = vel ? st.out(vel, no) : nullptr, *da = acc ? st.out(acc, no) : nullptr;
    return st.run([&] { return contact_points<double>(p, dq, dqd, dy, n_contacts, bodies, offsets, dp, dv, da, B, device, nullptr); });
}
int grbda_contact_dynamics_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *f_ext, int n_contacts,
                                    const int *bodies, const double *offsets, const double *a_des, double damping, double *ydd, double *lambda,
                                    double *ydd_free, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<double> cs;
    if (int rc = contact_dynamics_args<double>(p, q, qd, tau, f_ext, n_contacts, bodies, offsets, a_des, damping, ydd, lambda, ydd_free, B, cs))
        return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, nfe = static_cast<size_t>(p->host.n_bodies) * 6, no = B * static_cast<size_t>(n_contacts) * 3;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = st.in(qd, B * nv), *dt = st.in(tau, B * nv);
    const double *dfe = f_ext ? st.in(f_ext, B * nfe) : nullptr, *dad = a_des ? st.in(a_des, no) : nullptr;
    double *dy = st.out(ydd, B * nv), *dl = st.out(lambda, no), *dyf = ydd_free ? st.out(ydd_free, B * nv) : nullptr;
    return st.run([&] {
        return contact_dynamics<double>(p, dq, dqd, dt, dfe, n_contacts, bodies, offsets, dad, damping, dy, dl, dyf, B, device, nullptr);
    });
}
int grbda_contact_impulse_f64(const grbda_plan *p, const double *q, const double *qd, int n_contacts, const int *bodies, const double *offsets,
                              const double *v_des, double restitution, double damping, double *qd_next, double *impulse, size_t B, int device,
                              void *stream)
{
    return contact_impulse<double>(p, q, qd, n_contacts, bodies, offsets, v_des, restitution, damping, qd_next, impulse, B, device, stream);
}
int grbda_contact_impulse_f32(const grbda_plan *p, const float *q, const float *qd, int n_contacts, const int *bodies, const double *offsets,
                              const float *v_des, double restitution, double damping, float *qd_next, float *impulse, size_t B, int device,
                              void *stream)
{
    return contact_impulse<float>(p, q, qd, n_contacts, bodies, offsets, v_des, restitution, damping, qd_next, impulse, B, device, stream);
}
int grbda_contact_impulse_host_f64(const grbda_plan *p, const double *q, const double *qd, int n_contacts, const int *bodies, const double *offsets,
                                   const double *v_des, double restitution, double damping, double *qd_next, double *impulse, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<double> cs;
    if (int rc = contact_impulse_args<double>(p, q, qd, n_contacts, bodies, offsets, v_des, restitution, damping, qd_next, impulse, B, cs)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, no = B * static_cast<size_t>(n_contacts) * 3;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = st.in(qd, B * nv), *dvd = v_des ? st.in(v_des, no) : nullptr;
    double *dqn = st.out(qd_next, B * nv), *di = st.out(impulse, no);  // (qd_next == qd on the host: two device arrays, the input copied first)
    return st.run([&] {
        return contact_impulse<double>(p, dq, dqd, n_contacts, bodies, offsets, dvd, restitution, damping, dqn, di, B, device, nullptr);
    });
}
int grbda_aba_sharded_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, float *ydd, size_t B,
                          int n_gpus)
{
    return run_sharded<float>(p, false, q, qd, tau, ydd, B, n_gpus);
}
int grbda_aba_sharded_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, double *ydd, size_t B,
                          int n_gpus)
{
    return run_sharded<double>(p, false, q, qd, tau, ydd, B, n_gpus);
}
int grbda_rnea_sharded_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, float *tau, size_t B,
                           int n_gpus)
{
    return run_sharded<float>(p, true, q, qd, ydd, tau, B, n_gpus);
}
int grbda_aba_sharded_dev_f32(const grbda_plan *p, int n_gpus, const int *devices, const float *const *q, const float *const *qd,
                              const float *const *tau, float *const *ydd, const size_t *B, void *const *streams, float *gathered)
{
    return run_sharded_dev<float>(p, false, n_gpus, devices, q, qd, tau, ydd, B, streams, gathered);
}
int grbda_aba_sharded_dev_f64(const grbda_plan *p, int n_gpus, const int *devices, const double *const *q, const double *const *qd,
                              const double *const *tau, double *const *ydd, const size_t *B, void *const *streams, double *gathered)
{
    return run_sharded_dev<double>(p, false, n_gpus, devices, q, qd, tau, ydd, B, streams, gathered);
}
int grbda_rnea_sharded_dev_f32(const grbda_plan *p, int n_gpus, const int *devices, const float *const *q, const float *const *qd,
                               const float *const *ydd, float *const *tau, const size_t *B, void *const *streams, float *gathered)
{
    return run_sharded_dev<float>(p, true, n_gpus, devices, q, qd, ydd, tau, B, streams, gathered);
}
int grbda_rnea_sharded_dev_f64(const grbda_plan *p, int n_gpus, const int *devices, const double *const *q, const double *const *qd,
                               const double *const *ydd, double *const *tau, const size_t *B, void *const *streams, double *gathered)
{
    return run_sharded_dev<double>(p, true, n_gpus, devices, q, qd, ydd, tau, B, streams, gathered);
}
int grbda_rnea_sharded_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double *tau, size_t B,
                           int n_gpus)
{
    return run_sharded<double>(p, true, q, qd, ydd, tau, B, n_gpus);
}
int grbda_body_poses_host_f64(const grbda_plan *p, const double *q, double *Xa, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !Xa) return set_err(GRBDA_EINVAL, "null argument");
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nb = p->host.n_bodies;
    HostStage st;
    const double *dq = st.in(q, B * nq);
    double *dX = st.out(Xa, B * nb * 12);
    return st.run([&] { return poses<double>(p, dq, dX, B, device, nullptr); });
}
int grbda_body_twists_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double *V, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !qd || !ydd || !V) return set_err(GRBDA_EINVAL, "null argument");
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, nb = p->host.n_bodies;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = st.in(qd, B * nv), *dy = st.in(ydd, B * nv);
    double *dV = st.out(V, B * nb * 12);
    return st.run([&] { return twists<double>(p, dq, dqd, dy, dV, B, device, nullptr); });
}
int grbda_apply_test_force_host_f64(const grbda_plan *p, const double *q, int body, const double offset[3],
                                    const double *force, double *lambda_inv, double *dstate, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !force || !lambda_inv || !dstate) return set_err(GRBDA_EINVAL, "null argument");
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv;
    HostStage st;
    const double *dq = st.in(q, B * nq), *df = st.in(force, B * 3);
    double *dl = st.out(lambda_inv, B), *dd = st.out(dstate, B * nv);
    return st.run([&] { return test_force<double>(p, dq, body, offset, df, dl, dd, B, device, nullptr); });
}
int grbda_inv_osim_host_f64(const grbda_plan *p, const double *q, int n_contacts, const int *bodies, const double *offsets,
                            double *Linv, double *J, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !Linv) return set_err(GRBDA_EINVAL, "null argument");
    if (int rc = contact_count(n_contacts, "frames")) return rc;  // (the arrays and the body indices: the inner call's, once the device is found)
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, m = 6 * static_cast<size_t>(n_contacts);
    HostStage st;
    const double *dq = st.in(q, B * nq);
    double *dL = st.out(Linv, B * m * m), *dJ = J ? st.out(J, B * m * nv) : nullptr;
    return st.run([&] { return inv_osim<double>(p, dq, n_contacts, bodies, offsets, dL, dJ, B, device, nullptr); });
}
// host arrays: mass matrix and the derivatives of the forward dynamics (facade: getMassMatrix, forwardDynamicsDerivativesBatch)
int grbda_mass_matrix_host_f64(const grbda_plan *p, const double *q, double *H, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !H) return set_err(GRBDA_EINVAL, "null argument");
    DeviceTables *t = nullptr;
    if (int rc0 = ensure_device(p, device, &t)) return rc0;  // `device` current before anything is allocated on it
    const size_t nq = p->host.nq, nv = p->host.nv;
    HostStage st;
    const double *dq = st.in(q, B * nq);
    double *dH = st.out(H, B * nv * nv);
    return st.run([&] { return grbda_mass_matrix_f64(p, dq, dH, B, device, nullptr); });
}
int grbda_fd_derivatives_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, double *dq, double *dqd,
                                  double *dtau, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q || !qd || !tau) return set_err(GRBDA_EINVAL, "null argument");
    DeviceTables *t = nullptr;
    if (int rc0 = ensure_device(p, device, &t)) return rc0;  // `device` current before anything is allocated on it
    const size_t nq = p->host.nq, nv = p->host.nv, nn = nv * nv;
    HostStage st;
    const double *bq = st.in(q, B * nq), *bqd = st.in(qd, B * nv), *bt = st.in(tau, B * nv);
    double *b1 = dq ? st.out(dq, B * nn) : nullptr, *b2 = dqd ? st.out(dqd, B * nn) : nullptr, *b3 = dtau ? st.out(dtau, B * nn) : nullptr;
    return st.run([&] { return grbda_fd_derivatives_f64(p, bq, bqd, bt, b1, b2, b3, B, device, nullptr); });
}
int grbda_rnea_derivatives_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double step, double *dtau_dq,
                                    double *dtau_dqd, double *dtau_dydd, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = rnea_derivatives_args<double>(p, q, qd, ydd, dtau_dq, dtau_dqd, dtau_dydd, B)) return rc;
    if (B == 0) return GRBDA_OK;
    const size_t nq = p->host.nq, nv = p->host.nv, nn = nv * nv;
    DeviceTables *t = nullptr;
    if (int rc0 = ensure_device(p, device, &t)) return rc0;  // `device` current before anything is allocated on it
    HostStage st;
    const double *bq = st.in(q, B * nq), *bqd = st.in(qd, B * nv), *by = st.in(ydd, B * nv);
    double *b1 = dtau_dq ? st.out(dtau_dq, B * nn) : nullptr, *b2 = dtau_dqd ? st.out(dtau_dqd, B * nn) : nullptr,
           *b3 = dtau_dydd ? st.out(dtau_dydd, B * nn) : nullptr;
    return st.run([&] { return grbda_rnea_derivatives_f64(p, bq, bqd, by, step, b1, b2, b3, B, device, nullptr); });
}
int grbda_rnea_vjp_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, const double *g_tau, double step, double *grad_q,
                       double *grad_qd, double *grad_ydd, size_t B, int device, void *stream)
{
    return vjp<double>(p, false, q, qd, ydd, g_tau, step, grad_q, grad_qd, grad_ydd, nullptr, B, device, stream);
}
int grbda_rnea_vjp_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, const float *g_tau, double step, float *grad_q,
                       float *grad_qd, float *grad_ydd, size_t B, int device, void *stream)
{
    return vjp<float>(p, false, q, qd, ydd, g_tau, step, grad_q, grad_qd, grad_ydd, nullptr, B, device, stream);
}
int grbda_rnea_vjp_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, const double *g_tau, double step,
                            double *grad_q, double *grad_qd, double *grad_ydd, size_t B, int device)
{
    return vjp<double>(p, false, q, qd, ydd, g_tau, step, grad_q, grad_qd, grad_ydd, nullptr, B, device, nullptr, true);
}
int grbda_aba_vjp_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *g_ydd, double step, double *grad_q,
                      double *grad_qd, double *grad_tau, double *ydd, size_t B, int device, void *stream)
{
    return vjp<double>(p, true, q, qd, tau, g_ydd, step, grad_q, grad_qd, grad_tau, ydd, B, device, stream);
}
int grbda_aba_vjp_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, const float *g_ydd, double step, float *grad_q,
                      float *grad_qd, float *grad_tau, float *ydd, size_t B, int device, void *stream)
{
    return vjp<float>(p, true, q, qd, tau, g_ydd, step, grad_q, grad_qd, grad_tau, ydd, B, device, stream);
}
int grbda_aba_vjp_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *g_ydd, double step,
                           double *grad_q, double *grad_qd, double *grad_tau, double *ydd, size_t B, int device)
{
    return vjp<double>(p, true, q, qd, tau, g_ydd, step, grad_q, grad_qd, grad_tau, ydd, B, device, nullptr, true);
}
int grbda_vjp_contract_launch(int nv, size_t nb, int n_cu, size_t *units, size_t *grid)
{
    if (nv < 1 || n_cu < 1) return set_err(GRBDA_EINVAL, "nv and n_cu must be positive");
    const VjpLaunch L = vjp_contract_launch(nv, sizeof(double), n_cu, nb);  // (units and grid do not depend on the precision)
    if (units) *units = L.units;
    if (grid) *grid = L.grid;
    return GRBDA_OK;
}
int grbda_integrate_vjp_f64(const grbda_plan *p, const double *qd_next, double dt, const double *g_q_next, const double *g_qd_next, double *grad_q,
                            double *grad_qd, double *grad_ydd, size_t B, int device, void *stream)
{
    return integrate_vjp<double>(p, qd_next, dt, g_q_next, g_qd_next, grad_q, grad_qd, grad_ydd, B, device, stream);
}
int grbda_integrate_vjp_f32(const grbda_plan *p, const float *qd_next, double dt, const float *g_q_next, const float *g_qd_next, float *grad_q,
                            float *grad_qd, float *grad_ydd, size_t B, int device, void *stream)
{
    return integrate_vjp<float>(p, qd_next, dt, g_q_next, g_qd_next, grad_q, grad_qd, grad_ydd, B, device, stream);
}
int grbda_step_vjp_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *qd_next, double dt,
                       const double *g_q_next, const double *g_qd_next, double step, double *grad_q, double *grad_qd, double *grad_tau, size_t B,
                       int device, void *stream)
{
    return step_vjp<double>(p, q, qd, tau, qd_next, dt, g_q_next, g_qd_next, step, grad_q, grad_qd, grad_tau, B, device, stream);
}
int grbda_step_vjp_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, const float *qd_next, double dt, const float *g_q_next,
                       const float *g_qd_next, double step, float *grad_q, float *grad_qd, float *grad_tau, size_t B, int device, void *stream)
{
    return step_vjp<float>(p, q, qd, tau, qd_next, dt, g_q_next, g_qd_next, step, grad_q, grad_qd, grad_tau, B, device, stream);
}
int grbda_step_vjp_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *qd_next, double dt,
                            const double *g_q_next, const double *g_qd_next, double step, double *grad_q, double *grad_qd, double *grad_tau,
                            size_t B, int device)
{
    return step_vjp<double>(p, q, qd, tau, qd_next, dt, g_q_next, g_qd_next, step, grad_q, grad_qd, grad_tau, B, device, nullptr, true);
}
int grbda_rollout_vjp_f64(const grbda_plan *p, const double *q0, const double *qd0, const double *q_traj, const double *qd_traj, const double *tau,
                          int tau_steps, double dt, int T, const double *g_q, const double *g_qd, int g_steps, double step, double *grad_q0,
                          double *grad_qd0, double *grad_tau, size_t B, int device, void *stream)
{
    return rollout_vjp<double>(p, q0, qd0, q_traj, qd_traj, tau, tau_steps, dt, T, g_q, g_qd, g_steps, step, grad_q0, grad_qd0, grad_tau, B, device,
                               stream);
}
int grbda_rollout_vjp_f32(const grbda_plan *p, const float *q0, const float *qd0, const float *q_traj, const float *qd_traj, const float *tau,
                          int tau_steps, double dt, int T, const float *g_q, const float *g_qd, int g_steps, double step, float *grad_q0,
                          float *grad_qd0, float *grad_tau, size_t B, int device, void *stream)
{
    return rollout_vjp<float>(p, q0, qd0, q_traj, qd_traj, tau, tau_steps, dt, T, g_q, g_qd, g_steps, step, grad_q0, grad_qd0, grad_tau, B, device,
                              stream);
}
int grbda_rnea_jvp_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, const double *dq, const double *dqd, const double *dydd,
                       double step, double *dtau_out, size_t B, int device, void *stream)
{
    return jvp<double>(p, false, q, qd, ydd, dq, dqd, dydd, step, dtau_out, nullptr, B, device, stream);
}
int grbda_rnea_jvp_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, const float *dq, const float *dqd, const float *dydd,
                       double step, float *dtau_out, size_t B, int device, void *stream)
{
    return jvp<float>(p, false, q, qd, ydd, dq, dqd, dydd, step, dtau_out, nullptr, B, device, stream);
}
int grbda_rnea_jvp_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, const double *dq, const double *dqd,
                            const double *dydd, double step, double *dtau_out, size_t B, int device)
{
    return jvp<double>(p, false, q, qd, ydd, dq, dqd, dydd, step, dtau_out, nullptr, B, device, nullptr, true);
}
int grbda_aba_jvp_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *dq, const double *dqd, const double *dtau,
                      double step, double *dydd_out, double *ydd, size_t B, int device, void *stream)
{
    return jvp<double>(p, true, q, qd, tau, dq, dqd, dtau, step, dydd_out, ydd, B, device, stream);
}
int grbda_aba_jvp_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, const float *dq, const float *dqd, const float *dtau,
                      double step, float *dydd_out, float *ydd, size_t B, int device, void *stream)
{
    return jvp<float>(p, true, q, qd, tau, dq, dqd, dtau, step, dydd_out, ydd, B, device, stream);
}
int grbda_aba_jvp_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *dq, const double *dqd,
                           const double *dtau, double step, double *dydd_out, double *ydd, size_t B, int device)
{
    return jvp<double>(p, true, q, qd, tau, dq, dqd, dtau, step, dydd_out, ydd, B, device, nullptr, true);
}
int grbda_integrate_jvp_f64(const grbda_plan *p, const double *qd_next, double dt, const double *dq, const double *dqd, const double *dydd,
                            double *dq_next, double *dqd_next, size_t B, int device, void *stream)
{
    return integrate_jvp<double>(p, qd_next, dt, dq, dqd, dydd, dq_next, dqd_next, B, device, stream);
}
int grbda_integrate_jvp_f32(const grbda_plan *p, const float *qd_next, double dt, const float *dq, const float *dqd, const float *dydd, float *dq_next,
                            float *dqd_next, size_t B, int device, void *stream)
{
    return integrate_jvp<float>(p, qd_next, dt, dq, dqd, dydd, dq_next, dqd_next, B, device, stream);
}
int grbda_step_jvp_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *qd_next, double dt, const double *dq,
                       const double *dqd, const double *dtau, double step, double *dq_next, double *dqd_next, size_t B, int device, void *stream)
{
    return step_jvp<double>(p, q, qd, tau, qd_next, dt, dq, dqd, dtau, step, dq_next, dqd_next, B, device, stream);
}
int grbda_step_jvp_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, const float *qd_next, double dt, const float *dq,
                       const float *dqd, const float *dtau, double step, float *dq_next, float *dqd_next, size_t B, int device, void *stream)
{
    return step_jvp<float>(p, q, qd, tau, qd_next, dt, dq, dqd, dtau, step, dq_next, dqd_next, B, device, stream);
}
int grbda_step_jvp_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *qd_next, double dt, const double *dq,
                            const double *dqd, const double *dtau, double step, double *dq_next, double *dqd_next, size_t B, int device)
{
    return step_jvp<double>(p, q, qd, tau, qd_next, dt, dq, dqd, dtau, step, dq_next, dqd_next, B, device, nullptr, true);
}
int grbda_jvp_contract_launch(int nv, size_t nb, int n_cu, size_t *units, size_t *grid)
{
    if (nv < 1 || n_cu < 1) return set_err(GRBDA_EINVAL, "nv and n_cu must be positive");
    // (the units do not depend on the precision; the grid is the fp64 launch's -- an fp32 tile is half the bytes, so where the LDS of a CU
    // and not kJvpWavesPerCu bounds the grid, from nv = 18 on, the fp32 launch may hold more workgroups per CU)
    const JvpLaunch L = jvp_contract_launch(nv, sizeof(double), n_cu, nb);
    if (units) *units = L.units;
    if (grid) *grid = L.grid;
    return GRBDA_OK;
}
int grbda_plan_span_dims(const grbda_plan *p, int *n_span_vel)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    if (n_span_vel) *n_span_vel = span_count(p);
    return GRBDA_OK;
}
int grbda_project_positions_f64(const grbda_plan *p, double *q, int32_t *ok, size_t B, int max_iter, double tol,
                                int device, void *stream)
{
    return project<double>(p, q, ok, B, max_iter, tol, device, stream);
}
int grbda_project_positions_f32(const grbda_plan *p, float *q, int32_t *ok, size_t B, int max_iter, double tol,
                                int device, void *stream)
{
    return project<float>(p, q, ok, B, max_iter, tol, device, stream);
}
int grbda_project_positions_host_f64(const grbda_plan *p, double *q, int32_t *ok, size_t B, int max_iter, double tol, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q) return set_err(GRBDA_EINVAL, "null argument");
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq;
    HostStage st;
    double *dq = st.inout(q, B * nq);
    int32_t *dok = st.out(ok, B);  // (the kernel always writes the flags; a null `ok` only drops the copy)
    return st.run([&] { return project<double>(p, dq, dok, B, max_iter, tol, device, nullptr); });
}
int grbda_state_input_dims(const grbda_plan *p, const uint8_t *pos_is_spanning, const uint8_t *vel_is_spanning, int *in_nq, int *in_nv)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    return state_widths(p, pos_is_spanning, vel_is_spanning, nullptr, in_nq, in_nv);
}
int grbda_state_to_independent_f64(const grbda_plan *p, const uint8_t *pos_is_spanning, const uint8_t *vel_is_spanning, const double *q_in,
                                   const double *qd_in, double *q, double *qd, int32_t *status, double *cond, size_t B, double tol,
                                   int device, void *stream)
{
    return state_convert<double>(p, pos_is_spanning, vel_is_spanning, q_in, qd_in, q, qd, status, cond, B, tol, device, stream);
}
int grbda_state_to_independent_f32(const grbda_plan *p, const uint8_t *pos_is_spanning, const uint8_t *vel_is_spanning, const float *q_in,
                                   const float *qd_in, float *q, float *qd, int32_t *status, float *cond, size_t B, double tol,
                                   int device, void *stream)
{
    return state_convert<float>(p, pos_is_spanning, vel_is_spanning, q_in, qd_in, q, qd, status, cond, B, tol, device, stream);
}
int grbda_state_to_independent_host_f64(const grbda_plan *p, const uint8_t *pos_is_spanning, const uint8_t *vel_is_spanning,
                                        const double *q_in, const double *qd_in, double *q, double *qd, size_t B, double tol, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!q_in || !qd_in || !q || !qd) return set_err(GRBDA_EINVAL, "null argument");
    int in_nq = 0, in_nv = 0;
    if (int rc = state_widths(p, pos_is_spanning, vel_is_spanning, nullptr, &in_nq, &in_nv)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv;
    std::vector<int32_t> status(B);
    HostStage st;
    const double *bqi = st.in(q_in, B * in_nq), *bvi = st.in(qd_in, B * in_nv);
    int32_t *bs = st.out(status.data(), B);  // (read back first, as it always was)
    double *bq = st.out(q, B * nq), *bv = st.out(qd, B * nv);
    if (int rc = st.run([&] { return state_convert<double>(p, pos_is_spanning, vel_is_spanning, bqi, bvi, bq, bv, bs, nullptr, B, tol, device, nullptr); }))
        return rc;
    for (size_t b = 0; b < B; b++)
        if (status[b]) {
            const int code = status[b] & 255, cluster = status[b] >> 8;
            return set_err(GRBDA_ESTATE, "state " + std::to_string(b) + ", cluster " + std::to_string(cluster) + ": " +
                                             (code == 1 ? "Spanning position is not valid" : "Spanning velocity is not valid"));
        }
    return GRBDA_OK;
}
int grbda_spanning_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double *qd_span,
                       double *qdd_span, size_t B, int device, void *stream)
{
    return spanning<double>(p, q, qd, ydd, qd_span, qdd_span, B, device, stream);
}
int grbda_spanning_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, float *qd_span,
                       float *qdd_span, size_t B, int device, void *stream)
{
    return spanning<float>(p, q, qd, ydd, qd_span, qdd_span, B, device, stream);
}

int grbda_integrate_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double dt, double *q_next, double *qd_next,
                        int32_t *ok, int max_iter, double tol, size_t B, int device, void *stream)
{
    return integrate<double>(p, q, qd, ydd, dt, q_next, qd_next, ok, max_iter, tol, B, device, stream);
}
int grbda_integrate_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, double dt, float *q_next, float *qd_next,
                        int32_t *ok, int max_iter, double tol, size_t B, int device, void *stream)
{
    return integrate<float>(p, q, qd, ydd, dt, q_next, qd_next, ok, max_iter, tol, B, device, stream);
}
int grbda_step_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *f_ext, double dt, double *ydd,
                   double *q_next, double *qd_next, int32_t *ok, size_t B, int device, void *stream)
{
    return step<double>(p, q, qd, tau, f_ext, dt, ydd, q_next, qd_next, ok, B, device, stream);
}
int grbda_step_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, const float *f_ext, double dt, float *ydd,
                   float *q_next, float *qd_next, int32_t *ok, size_t B, int device, void *stream)
{
    return step<float>(p, q, qd, tau, f_ext, dt, ydd, q_next, qd_next, ok, B, device, stream);
}
int grbda_rollout_f64(const grbda_plan *p, double *q, double *qd, const double *tau, int tau_steps, double dt, int T, double *ydd_work,
                      double *q_traj, double *qd_traj, int32_t *ok, size_t B, int device, void *stream)
{
    return rollout<double>(p, q, qd, tau, tau_steps, dt, T, ydd_work, q_traj, qd_traj, ok, B, device, stream);
}
int grbda_rollout_f32(const grbda_plan *p, float *q, float *qd, const float *tau, int tau_steps, double dt, int T, float *ydd_work,
                      float *q_traj, float *qd_traj, int32_t *ok, size_t B, int device, void *stream)
{
    return rollout<float>(p, q, qd, tau, tau_steps, dt, T, ydd_work, q_traj, qd_traj, ok, B, device, stream);
}
int grbda_integrate_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double dt, double *q_next,
                             double *qd_next, int32_t *ok, int max_iter, double tol, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = integrate_args<double>(p, q, qd, ydd, dt, q_next, qd_next, max_iter, tol, B)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = st.in(qd, B * nv), *dy = st.in(ydd, B * nv);
    double *dqn = st.out(q_next, B * nq), *dvn = st.out(qd_next, B * nv);
    int32_t *dok = st.out(ok, B);  // (a null `ok` only drops the copy)
    return st.run([&] { return integrate<double>(p, dq, dqd, dy, dt, dqn, dvn, dok, max_iter, tol, B, device, nullptr); });
}
int grbda_step_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, const double *f_ext, double dt, double *ydd,
                        double *q_next, double *qd_next, int32_t *ok, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = step_args<double>(p, q, qd, tau, f_ext, dt, ydd, q_next, qd_next, B)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, nfe = static_cast<size_t>(p->host.n_bodies) * 6;
    HostStage st;
    const double *dfe = f_ext ? st.in(f_ext, B * nfe) : nullptr;
    const double *dq = st.in(q, B * nq), *dqd = st.in(qd, B * nv), *dt_ = st.in(tau, B * nv);
    double *dy = st.out(ydd, B * nv), *dqn = st.out(q_next, B * nq), *dvn = st.out(qd_next, B * nv);
    int32_t *dok = st.out(ok, B);
    return st.run([&] { return step<double>(p, dq, dqd, dt_, dfe, dt, dy, dqn, dvn, dok, B, device, nullptr); });
}

// ---- include/grbda_hip_contact_step.h ---------------------------------------------------------------------------------------------------
int grbda_contact_dynamics_active_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, int n_contacts, const int *bodies,
                                      const double *offsets, const int32_t *active, const double *a_des, double kd, double damping, double *ydd,
                                      double *lambda, double *ydd_free, size_t B, int device, void *stream)
{
    return contact_dynamics_active<double>(p, q, qd, tau, n_contacts, bodies, offsets, active, a_des, kd, damping, ydd, lambda, ydd_free, B, device, stream);
}
int grbda_contact_dynamics_active_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, int n_contacts, const int *bodies,
                                      const double *offsets, const int32_t *active, const float *a_des, double kd, double damping, float *ydd,
                                      float *lambda, float *ydd_free, size_t B, int device, void *stream)
{
    return contact_dynamics_active<float>(p, q, qd, tau, n_contacts, bodies, offsets, active, a_des, kd, damping, ydd, lambda, ydd_free, B, device, stream);
}
int grbda_contact_impulse_active_f64(const grbda_plan *p, const double *q, const double *qd, int n_contacts, const int *bodies, const double *offsets,
                                     const int32_t *active, const double *v_des, double restitution, double damping, double *qd_next,
                                     double *impulse, size_t B, int device, void *stream)
{
    return contact_impulse_active<double>(p, q, qd, n_contacts, bodies, offsets, active, v_des, restitution, damping, qd_next, impulse, B, device, stream);
}
int grbda_contact_impulse_active_f32(const grbda_plan *p, const float *q, const float *qd, int n_contacts, const int *bodies, const double *offsets,
                                     const int32_t *active, const float *v_des, double restitution, double damping, float *qd_next, float *impulse,
                                     size_t B, int device, void *stream)
{
    return contact_impulse_active<float>(p, q, qd, n_contacts, bodies, offsets, active, v_des, restitution, damping, qd_next, impulse, B, device, stream);
}
int grbda_contact_step_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, int n_contacts, const int *bodies,
                           const double *offsets, const int32_t *active, const int32_t *prev_active, double kd, double restitution, double damping,
                           double dt, double *ydd, double *lambda, double *impulse, double *q_next, double *qd_next, int32_t *ok, size_t B,
                           int device, void *stream)
{
    return contact_step<double>(p, q, qd, tau, n_contacts, bodies, offsets, active, prev_active, kd, restitution, damping, dt, ydd, lambda, impulse, q_next,
                                qd_next, ok, B, device, stream);
}
int grbda_contact_step_f32(const grbda_plan *p, const float *q, const float *qd, const float *tau, int n_contacts, const int *bodies,
                           const double *offsets, const int32_t *active, const int32_t *prev_active, double kd, double restitution, double damping,
                           double dt, float *ydd, float *lambda, float *impulse, float *q_next, float *qd_next, int32_t *ok, size_t B, int device,
                           void *stream)
{
    return contact_step<float>(p, q, qd, tau, n_contacts, bodies, offsets, active, prev_active, kd, restitution, damping, dt, ydd, lambda, impulse, q_next,
                               qd_next, ok, B, device, stream);
}
int grbda_contact_step_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau, int n_contacts, const int *bodies,
                                const double *offsets, const int32_t *active, const int32_t *prev_active, double kd, double restitution,
                                double damping, double dt, double *ydd, double *lambda, double *impulse, double *q_next, double *qd_next,
                                int32_t *ok, size_t B, int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    ContactSet<double> cs;
    if (int rc = contact_step_args<double>(p, q, qd, tau, n_contacts, bodies, offsets, active, prev_active, kd, restitution, damping, dt, ydd, lambda,
                                           impulse, q_next, qd_next, ok, B, cs))
        return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv, no = B * static_cast<size_t>(n_contacts) * 3;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = st.in(qd, B * nv), *dt_ = st.in(tau, B * nv);
    const int32_t *da = st.in(active, B), *dp = prev_active ? st.in(prev_active, B) : nullptr;
    double *dy = st.out(ydd, B * nv), *dl = st.out(lambda, no), *di = impulse ? st.out(impulse, no) : nullptr;
    // (q_next == q, qd_next == qd on the host: two device arrays each, the inputs copied first)
    double *dqn = st.out(q_next, B * nq), *dvn = st.out(qd_next, B * nv);
    int32_t *dok = st.out(ok, B);
    return st.run([&] {
        return contact_step<double>(p, dq, dqd, dt_, n_contacts, bodies, offsets, da, dp, kd, restitution, damping, dt, dy, dl, di, dqn, dvn, dok, B, device,
                                    nullptr);
    });
}
int grbda_contact_rollout_f64(const grbda_plan *p, double *q, double *qd, const double *tau, int tau_steps, int n_contacts, const int *bodies,
                              const double *offsets, const int32_t *active, int active_steps, const int32_t *active_prev, int with_impulses,
                              double kd, double restitution, double damping, double dt, int T, double *ydd_work, double *q_traj, double *qd_traj,
                              double *lambda_traj, int32_t *ok, size_t B, int device, void *stream)
{
    return contact_rollout<double>(p, q, qd, tau, tau_steps, n_contacts, bodies, offsets, active, active_steps, active_prev, with_impulses, kd, restitution,
                                   damping, dt, T, ydd_work, q_traj, qd_traj, lambda_traj, ok, B, device, stream);
}
int grbda_contact_rollout_f32(const grbda_plan *p, float *q, float *qd, const float *tau, int tau_steps, int n_contacts, const int *bodies,
                              const double *offsets, const int32_t *active, int active_steps, const int32_t *active_prev, int with_impulses,
                              double kd, double restitution, double damping, double dt, int T, float *ydd_work, float *q_traj, float *qd_traj,
                              float *lambda_traj, int32_t *ok, size_t B, int device, void *stream)
{
    return contact_rollout<float>(p, q, qd, tau, tau_steps, n_contacts, bodies, offsets, active, active_steps, active_prev, with_impulses, kd, restitution,
                                  damping, dt, T, ydd_work, q_traj, qd_traj, lambda_traj, ok, B, device, stream);
}

int grbda_plan_total_mass(const grbda_plan *p, double *mass)
{
    if (!p || !mass) return set_err(GRBDA_EINVAL, "null argument");
    *mass = plan_total_mass(p);
    return GRBDA_OK;
}
int grbda_energy_f64(const grbda_plan *p, const double *q, const double *qd, double *kinetic, double *potential, size_t B, int device, void *stream)
{
    CentroidalOut<double> o{};
    o.kinetic = kinetic;
    o.potential = potential;
    return centroidal<double>(p, q, qd, nullptr, o, B, device, stream);
}
int grbda_energy_f32(const grbda_plan *p, const float *q, const float *qd, float *kinetic, float *potential, size_t B, int device, void *stream)
{
    CentroidalOut<float> o{};
    o.kinetic = kinetic;
    o.potential = potential;
    return centroidal<float>(p, q, qd, nullptr, o, B, device, stream);
}
int grbda_centroidal_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double *com, double *com_vel, double *h,
                         double *hdot, size_t B, int device, void *stream)
{
    CentroidalOut<double> o{};
    o.com = com;
    o.com_vel = com_vel;
    o.h = h;
    o.hdot = hdot;
    return centroidal<double>(p, q, qd, ydd, o, B, device, stream);
}
int grbda_centroidal_f32(const grbda_plan *p, const float *q, const float *qd, const float *ydd, float *com, float *com_vel, float *h, float *hdot,
                         size_t B, int device, void *stream)
{
    CentroidalOut<float> o{};
    o.com = com;
    o.com_vel = com_vel;
    o.h = h;
    o.hdot = hdot;
    return centroidal<float>(p, q, qd, ydd, o, B, device, stream);
}
int grbda_centroidal_matrix_f64(const grbda_plan *p, const double *q, double *A, size_t B, int device, void *stream)
{
    return centroidal_matrix<double>(p, q, A, B, device, stream);
}
int grbda_centroidal_matrix_f32(const grbda_plan *p, const float *q, float *A, size_t B, int device, void *stream)
{
    return centroidal_matrix<float>(p, q, A, B, device, stream);
}
// host arrays: the checks of the device entry points first, then the device, then the staging
static int centroidal_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, const CentroidalOut<double> &o, size_t B,
                               int device)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (int rc = centroidal_args<double>(p, q, qd, ydd, o, B)) return rc;
    if (B == 0) return GRBDA_OK;
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    const size_t nq = p->host.nq, nv = p->host.nv;
    HostStage st;
    const double *dq = st.in(q, B * nq), *dqd = qd ? st.in(qd, B * nv) : nullptr, *dy = ydd ? st.in(ydd, B * nv) : nullptr;
    CentroidalOut<double> d{};
    d.kinetic = o.kinetic ? st.out(o.kinetic, B) : nullptr;
    d.potential = o.potential ? st.out(o.potential, B) : nullptr;
    d.com = o.com ? st.out(o.com, B * 3) : nullptr;
    d.com_vel = o.com_vel ? st.out(o.com_vel, B * 3) : nullptr;
    d.h = o.h ? st.out(o.h, B * 6) : nullptr;
    d.hdot = o.hdot ? st.out(o.hdot, B * 6) : nullptr;
    return st.run([&] { return centroidal<double>(p, dq, dqd, dy, d, B, device, nullptr); });
}
int grbda_energy_host_f64(const grbda_plan *p, const double *q, const double *qd, double *kinetic, double *potential, size_t B, int device)
{
    CentroidalOut<double> o{};
    o.kinetic = kinetic;
    o.potential = potential;
    return centroidal_host_f64(p, q, qd, nullptr, o, B, device);
}
int grbda_centroidal_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd, double *com, double *com_vel, double *h,
                              double *hdot, size_t B, int device)
{
    CentroidalOut<double> o{};
    o.com = com;
    o.com_vel = com_vel;
    o.h = h;
    o.hdot = hdot;
    return centroidal_host_f64(p, q, qd, ydd, o, B, device);
}

int grbda_aba_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *tau,
                       const double *f_ext, double *ydd, size_t B, int device)
{
    return run_host_f64(p, false, q, qd, tau, f_ext, ydd, B, device);
}
int grbda_rnea_host_f64(const grbda_plan *p, const double *q, const double *qd, const double *ydd,
                        const double *f_ext, double *tau, size_t B, int device)
{
    return run_host_f64(p, true, q, qd, ydd, f_ext, tau, B, device);
}

int grbda_time_kernel(const grbda_plan *p, int kind, int precision, const void *q, const void *qd, const void *x,
                      void *out, size_t B, int device, void *stream, int iters, float *avg_ms)
{
    if (!p) return set_err(GRBDA_EINVAL, "null plan");
    GRBDA_CALL_SCOPE(p);
    if (!avg_ms || iters <= 0 || (precision != 32 && precision != 64) || (kind != 0 && kind != 1))
        return set_err(GRBDA_EINVAL, "bad timing arguments");
    DeviceTables *t = nullptr;
    if (int rc = ensure_device(p, device, &t)) return rc;
    hipEvent_t e0, e1;
    hipError_t e;
    if ((e = hipEventCreate(&e0)) != hipSuccess || (e = hipEventCreate(&e1)) != hipSuccess) return hip_err(e, "hipEventCreate");
    auto once = [&]() -> int {
        if (precision == 32)
            return run<float>(p, kind == 1, static_cast<const float *>(q), static_cast<const float *>(qd),
                              static_cast<const float *>(x), nullptr, static_cast<float *>(out), B, device, stream);
        return run<double>(p, kind == 1, static_cast<const double *>(q), static_cast<const double *>(qd),
                           static_cast<const double *>(x), nullptr, static_cast<double *>(out), B, device, stream);
    };
    int rc = once();  // warm-up: uploads tables, sizes scratch
    if (rc == GRBDA_OK) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if ((e = hipEventRecord(e0, s)) != hipSuccess) rc = hip_err(e, "hipEventRecord");
        for (int i = 0; i < iters && rc == GRBDA_OK; i++) rc = once();
        if (rc == GRBDA_OK && (e = hipEventRecord(e1, s)) != hipSuccess) rc = hip_err(e, "hipEventRecord");
        if (rc == GRBDA_OK && (e = hipEventSynchronize(e1)) != hipSuccess) rc = hip_err(e, "hipEventSynchronize");
        float ms = 0;
        if (rc == GRBDA_OK && (e = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) rc = hip_err(e, "hipEventElapsedTime");
        if (rc == GRBDA_OK) *avg_ms = ms / static_cast<float>(iters);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

int grbda_device_count(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count < 0 ? 0 : count;
}

}  // extern "C"
