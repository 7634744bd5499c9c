// body_list_kernels.hip -- poses and twists of a listed few bodies (include/grbda_hip_bodies.h; capi.cpp, body_list_run).
//
// poses_kernel / twists_kernel (kernels.hip) write every body of every state and read each parent back from that global output row.  The
// kernels here follow a WALK (walk.h, BodyWalkStep; devplan.h, BodyWalk) over the listed bodies' ancestors only: one state per lane, a
// grid-stride loop over tiles of 64 states, the running [E | r] (poses) or [v | a] (twists) of the current root path in registers, the
// values of branch points in LDS ([slot][value][lane]: a lane reads what it wrote, lane == bank, no barrier), and nothing read back from
// global memory.  The walk is wave-uniform -- it sits in the kernel arguments and is read through the scalar unit -- so every branch on it is
// a scalar branch and no per-lane array is indexed at run time.  The LDS slots, the joint angle and the pose step are walk_dev.h's, which
// frame_jacobian_kernels.hip uses too.  The per-body formulas are those of poses_kernel / twists_kernel, term by term, on the same device
// functions; as there, values are composed in the plan's canonical body frames and permuted to the reference's axes as they are stored.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

#include "devmath.h"
#include "walk_dev.h"

namespace {

// one row of the output in the reference's body axes.  ROWS 3: a pose, the rows of E move (E_ref = Rc^T E) and r stays; ROWS 4: a twist, the
// components of each of the four 3-vectors move (poses_kernel / twists_kernel, tail loops)
template <class T, int ROWS>
__device__ __forceinline__ void store_row(T *o, const T (&x)[12], int canon)
{
    if (canon == 2) {
#pragma unroll
        for (int k = 0; k < 12; k++) o[k] = x[k];
        return;
    }
    const int to0 = canon == 0 ? 1 : 2, to1 = canon == 0 ? 2 : 0, to2 = canon == 0 ? 0 : 1;
    if constexpr (ROWS == 3) {
#pragma unroll
        for (int w = 0; w < 3; w++) {
            o[3 * to0 + w] = x[w];
            o[3 * to1 + w] = x[3 + w];
            o[3 * to2 + w] = x[6 + w];
            o[9 + w] = x[9 + w];
        }
    } else {
#pragma unroll
        for (int h = 0; h < 4; h++) {
            o[3 * h + to0] = x[3 * h];
            o[3 * h + to1] = x[3 * h + 1];
            o[3 * h + to2] = x[3 * h + 2];
        }
    }
}

}  // namespace

// X = [E 9 | r 3] of the step's body from its parent's (walk_dev.h, walk_pose_step)
template <class T>
__global__ __launch_bounds__(kWave, 1) void body_poses_list_kernel(BodyWalk<T> W, const T *__restrict__ q, T *__restrict__ out, size_t B)
{
    cptr<T> consts = (cptr<T>)W.consts;
    const int lane = threadIdx.x;
    const size_t n_tiles = (B + kWave - 1) / kWave;
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t r = tile * kWave + lane;
        if (r >= B) continue;  // (no cross-lane operation below)
        const T *qr = q + r * (size_t)W.nq;
        T *orow = out + r * (size_t)W.n_list * 12;
        T X[12];
#pragma unroll
        for (int k = 0; k < 12; k++) X[k] = 0;
        int oi = 0;
        for (int s = 0; s < W.n_steps; s++) {
            const BodyWalkStep st = W.step[s];
            walk_pose_step(st, consts, W.ori_repr, qr, lane, X);
            for (int k = 0; k < st.n_out; k++) store_row<T, 3>(orow + (size_t)W.slot[oi++] * 12, X, st.canon);
        }
    }
}

// V = [v 6 | a 6] of the step's body from its parent's (TreeNode::v_ / a_; twists_kernel): the spanning rates come from spanning_kernel
template <class T>
__global__ __launch_bounds__(kWave, 1) void body_twists_list_kernel(BodyWalk<T> W, const T *__restrict__ q, const T *__restrict__ qd_span,
                                                                    const T *__restrict__ qdd_span, T *__restrict__ out, size_t B)
{
    cptr<T> consts = (cptr<T>)W.consts;
    const int lane = threadIdx.x;
    const size_t n_tiles = (B + kWave - 1) / kWave;
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t r = tile * kWave + lane;
        if (r >= B) continue;  // (no cross-lane operation below)
        const T *qr = q + r * (size_t)W.nq;
        const T *vs = qd_span + r * (size_t)W.n_span, *as = qdd_span + r * (size_t)W.n_span;
        T *orow = out + r * (size_t)W.n_list * 12;
        T X[12];
#pragma unroll
        for (int k = 0; k < 12; k++) X[k] = 0;
        int oi = 0;
        for (int s = 0; s < W.n_steps; s++) {
            const BodyWalkStep st = W.step[s];
            if (st.restore != kWalkNone) slot_get(st.restore, lane, X);
            T v[6], a[6];
            if (st.free) {  // S = 1, the rates are the base twist; a = X (-gravity) + ydd
                T o[4], E[9];
                const int nori = W.ori_repr == 0 ? 4 : 3;
                for (int j = 0; j < 4; j++) o[j] = j < nori ? qr[st.q_col + 3 + j] : T(0);
                free_rotation(W.ori_repr, o, E);
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    v[j] = vs[st.span_col + j];
                    a[j] = as[st.span_col + j];
                }
#pragma unroll
                for (int u = 0; u < 3; u++) {
                    a[u] += E[3 * u] * W.a_root[0] + E[3 * u + 1] * W.a_root[1] + E[3 * u + 2] * W.a_root[2];
                    a[3 + u] += E[3 * u] * W.a_root[3] + E[3 * u + 1] * W.a_root[4] + E[3 * u + 2] * W.a_root[5];
                }
            } else {
                cptr<T> C = consts + st.cofs;
                const T qi = joint_angle(st, C, qr);
                T sn, cs, El[9], vp[6], ap[6];
                sincos_t(qi, &sn, &cs);
                build_E((int)st.axis, sn, cs, C, El);
                if (!st.root) {
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        vp[j] = X[j];
                        ap[j] = X[6 + j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        vp[j] = 0;
                        ap[j] = W.a_root[j];
                    }
                }
                xmotion(El, C + 9, vp, v);
                xmotion(El, C + 9, ap, a);
                const T qdi = vs[st.span_col], qddi = as[st.span_col];
                // v x (S qdi), S the unit angular axis e: [w x e; v_lin x e] qdi.  The axis is wave-uniform: three scalar branches of
                // statically indexed code
                if (st.axis == 0) {
                    v[0] += qdi;
                    a[1] += v[2] * qdi;
                    a[2] -= v[1] * qdi;
                    a[4] += v[5] * qdi;
                    a[5] -= v[4] * qdi;
                    a[0] += qddi;
                } else if (st.axis == 1) {
                    v[1] += qdi;
                    a[2] += v[0] * qdi;
                    a[0] -= v[2] * qdi;
                    a[5] += v[3] * qdi;
                    a[3] -= v[5] * qdi;
                    a[1] += qddi;
                } else {
                    v[2] += qdi;
                    a[0] += v[1] * qdi;
                    a[1] -= v[0] * qdi;
                    a[3] += v[4] * qdi;
                    a[4] -= v[3] * qdi;
                    a[2] += qddi;
                }
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                X[j] = v[j];
                X[6 + j] = a[j];
            }
            if (st.save != kWalkNone) slot_put(st.save, lane, X);
            for (int k = 0; k < st.n_out; k++) store_row<T, 4>(orow + (size_t)W.slot[oi++] * 12, X, st.canon);
        }
    }
}

// the fallback's second half: one (state, slot) per thread
template <class T>
__global__ void body_gather_kernel(BodyList L, const T *__restrict__ full, int n_bodies, size_t nb, T *__restrict__ out)
{
    const size_t total = nb * (size_t)L.n;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t b = t / L.n;
        const int i = (int)(t % L.n);
        const T *src = full + (b * n_bodies + L.body[i]) * 12;
        T *dst = out + t * 12;
#pragma unroll
        for (int k = 0; k < 12; k++) dst[k] = src[k];
    }
}

template <class T>
static size_t saved_bytes(const BodyWalk<T> &W)
{
    return (size_t)W.n_saved * 12 * kWave * sizeof(T);
}
template <class T>
hipError_t launch_body_poses_list(const BodyWalk<T> &W, const T *q, T *out, size_t nb, int grid, hipStream_t stream)
{
    if (nb == 0 || W.n_list == 0) return hipSuccess;
    hipLaunchKernelGGL((body_poses_list_kernel<T>), dim3(grid), dim3(kWave), saved_bytes(W), stream, W, q, out, nb);
    return hipGetLastError();
}
template <class T>
hipError_t launch_body_twists_list(const BodyWalk<T> &W, const T *q, const T *qd_span, const T *qdd_span, T *out, size_t nb, int grid,
                                   hipStream_t stream)
{
    if (nb == 0 || W.n_list == 0) return hipSuccess;
    hipLaunchKernelGGL((body_twists_list_kernel<T>), dim3(grid), dim3(kWave), saved_bytes(W), stream, W, q, qd_span, qdd_span, out, nb);
    return hipGetLastError();
}
template <class T>
hipError_t launch_body_gather(const BodyList &L, const T *full, int n_bodies, size_t nb, T *out, hipStream_t stream)
{
    if (nb == 0 || L.n == 0) return hipSuccess;
    const int grid = (int)std::min<size_t>((nb * L.n + 255) / 256, 65535);
    hipLaunchKernelGGL((body_gather_kernel<T>), dim3(grid), dim3(256), 0, stream, L, full, n_bodies, nb, out);
    return hipGetLastError();
}
template hipError_t launch_body_poses_list<float>(const BodyWalk<float> &, const float *, float *, size_t, int, hipStream_t);
template hipError_t launch_body_poses_list<double>(const BodyWalk<double> &, const double *, double *, size_t, int, hipStream_t);
template hipError_t launch_body_twists_list<float>(const BodyWalk<float> &, const float *, const float *, const float *, float *, size_t, int,
                                                   hipStream_t);
template hipError_t launch_body_twists_list<double>(const BodyWalk<double> &, const double *, const double *, const double *, double *, size_t,
                                                    int, hipStream_t);
template hipError_t launch_body_gather<float>(const BodyList &, const float *, int, size_t, float *, hipStream_t);
template hipError_t launch_body_gather<double>(const BodyList &, const double *, int, size_t, double *, hipStream_t);

}  // namespace grbda_hip
