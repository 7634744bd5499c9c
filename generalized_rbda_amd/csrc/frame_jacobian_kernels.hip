// frame_jacobian_kernels.hip -- frame Jacobians and their drift at a listed few body frames (include/grbda_hip_jacobians.h; capi.cpp,
// frame_jacobians_run).
//
// Route 0, frame_jacobian_walk_kernel: the execution model of body_list_kernels.hip -- one state per lane, one-wavefront workgroups, a
// grid-stride loop over tiles of 64 states, the walk (walk.h, JacWalkStep; devplan.h, JacWalk) in the kernel arguments and read through the
// scalar unit, every branch on it a scalar branch, no per-lane array indexed at run time, saved values in LDS as [slot][value][lane] (a lane
// reads what it wrote: no barrier), global memory written once and never read back.  The LDS slots and the pose step are walk_dev.h's, the
// ones body_poses_list_kernel runs.  Two passes over the walk per tile:
//   1. the poses of the root paths (walk_pose_step); a listed frame leaves [E | p], p = r + E^T offset its point in world coordinates, in
//      LDS slot n_saved + i;
//   2. the poses again, and from each the joint's screw axis in WORLD coordinates about the world origin: a revolute joint [w ; r x w] with
//      w = E^T e, the base its six body axes [E^T e_j ; r x E^T e_j], [0 ; E^T e_j].  World-frame axes of one cluster add, so a cluster's
//      n columns A[a] = sum over its bodies on the root path of G[body][a] [w ; r x w] accumulate in registers while the walk stays inside
//      the cluster, and a frame takes them at the deepest such body: [w ; m + w x p], turned with the frame's E for body axes.
// Columns off a frame's root path are written as zeros from the host's column masks before the passes.
//
// Route 1 and the drift: element-wise finishing kernels over the listed twists of the existing path (body_list_kernels.hip), which arrive in
// the reference's body axes like the offsets.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

#include "devmath.h"
#include "walk_dev.h"

namespace {

// one column of one frame: the world-frame axis S = [w ; m] about the world origin, seen at the frame F = [E | p].  o: the column's first
// row, rows nv apart; body axes are permuted to the reference's as store_row permutes a twist
template <class T>
__device__ __forceinline__ void emit_column(const T (&F)[12], const T (&S)[6], int world, int canon, T *o, size_t nv)
{
    const T v[3] = {S[3] + S[1] * F[11] - S[2] * F[10], S[4] + S[2] * F[9] - S[0] * F[11], S[5] + S[0] * F[10] - S[1] * F[9]};
    if (world) {
#pragma unroll
        for (int u = 0; u < 3; u++) {
            o[u * nv] = S[u];
            o[(3 + u) * nv] = v[u];
        }
        return;
    }
    const int to[3] = {(canon + 1) % 3, (canon + 2) % 3, canon % 3};
#pragma unroll
    for (int u = 0; u < 3; u++) {
        o[to[u] * nv] = F[3 * u] * S[0] + F[3 * u + 1] * S[1] + F[3 * u + 2] * S[2];
        o[(3 + to[u]) * nv] = F[3 * u] * v[0] + F[3 * u + 1] * v[1] + F[3 * u + 2] * v[2];
    }
}

}  // namespace

template <class T>
__global__ __launch_bounds__(kWave, 1) void frame_jacobian_walk_kernel(JacWalk<T> W, const T *__restrict__ q, T *__restrict__ J, size_t B)
{
    cptr<T> consts = (cptr<T>)W.consts;
    const int lane = threadIdx.x;
    const size_t n_tiles = (B + kWave - 1) / kWave, nv = (size_t)W.nv;
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t r = tile * kWave + lane;
        if (r >= B) continue;  // (no cross-lane operation below)
        const T *qr = q + r * (size_t)W.nq;
        T *Jr = J + r * (size_t)W.n_list * 6 * nv;
        // the structural zeros
        for (int i = 0; i < W.n_list; i++)
            for (int c = 0; c < W.nv; c++)
                if (!((W.cols[i][c >> 6] >> (c & 63)) & 1)) {
                    T *o = Jr + (size_t)i * 6 * nv + c;
#pragma unroll
                    for (int u = 0; u < 6; u++) o[u * nv] = 0;
                }
        T X[12];
#pragma unroll
        for (int k = 0; k < 12; k++) X[k] = 0;
        // pass 1: the frames, [E | p]
        for (int s = 0; s < W.n_steps; s++) {
            const JacWalkStep st = W.step[s];
            walk_pose_step(st, consts, W.ori_repr, qr, lane, X);
            if (st.own == 0) continue;
            for (int i = 0; i < W.n_list; i++) {
                if (!((st.own >> i) & 1)) continue;
                const T ox = W.off[i][0], oy = W.off[i][1], oz = W.off[i][2];
                T F[12];
#pragma unroll
                for (int u = 0; u < 9; u++) F[u] = X[u];
#pragma unroll
                for (int u = 0; u < 3; u++) F[9 + u] = X[9 + u] + X[u] * ox + X[3 + u] * oy + X[6 + u] * oz;
                slot_put(W.n_saved + i, lane, F);
            }
        }
        // pass 2: the columns
        T A[kJacMaxDof][6];
#pragma unroll
        for (int a = 0; a < kJacMaxDof; a++)
#pragma unroll
            for (int u = 0; u < 6; u++) A[a][u] = 0;
        for (int s = 0; s < W.n_steps; s++) {
            const JacWalkStep st = W.step[s];
            walk_pose_step(st, consts, W.ori_repr, qr, lane, X);
            if (st.free) {
                for (int i = 0; i < W.n_list; i++) {
                    if (!((st.below >> i) & 1)) continue;
                    T F[12];
                    slot_get(W.n_saved + i, lane, F);
                    T *o = Jr + (size_t)i * 6 * nv + st.v_col;
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const T w[3] = {X[3 * j], X[3 * j + 1], X[3 * j + 2]};
                        const T Sa[6] = {w[0], w[1], w[2], X[10] * w[2] - X[11] * w[1], X[11] * w[0] - X[9] * w[2], X[9] * w[1] - X[10] * w[0]};
                        const T Sl[6] = {0, 0, 0, w[0], w[1], w[2]};
                        emit_column(F, Sa, W.world, (int)W.canon[i], o + j, nv);
                        emit_column(F, Sl, W.world, (int)W.canon[i], o + 3 + j, nv);
                    }
                }
                continue;
            }
            // w = E^T e: row `axis` of E (the axis is wave-uniform: selects, no indexed register)
            const T w0 = st.axis == 0 ? X[0] : st.axis == 1 ? X[3] : X[6];
            const T w1 = st.axis == 0 ? X[1] : st.axis == 1 ? X[4] : X[7];
            const T w2 = st.axis == 0 ? X[2] : st.axis == 1 ? X[5] : X[8];
            const T S[6] = {w0, w1, w2, X[10] * w2 - X[11] * w1, X[11] * w0 - X[9] * w2, X[9] * w1 - X[10] * w0};
            cptr<T> G = consts + st.cofs + kBodyConstFixed;
#pragma unroll
            for (int a = 0; a < kJacMaxDof; a++) {
                if (a < st.n) {
                    const T g = G[a];
#pragma unroll
                    for (int u = 0; u < 6; u++) A[a][u] = st.cont ? A[a][u] + g * S[u] : g * S[u];
                }
            }
            if (st.emit == 0) continue;
            for (int i = 0; i < W.n_list; i++) {
                if (!((st.emit >> i) & 1)) continue;
                T F[12];
                slot_get(W.n_saved + i, lane, F);
                T *o = Jr + (size_t)i * 6 * nv + st.v_col;
#pragma unroll
                for (int a = 0; a < kJacMaxDof; a++)
                    if (a < st.n) emit_column(F, A[a], W.world, (int)W.canon[i], o + a, nv);
            }
        }
    }
}

// route 1: one (state, frame, column) per thread, consecutive threads on consecutive columns
template <class T>
__global__ void frame_jacobian_columns_kernel(FrameSet<T> F, const T *__restrict__ Vx, const T *__restrict__ Xa, int nv, size_t nb,
                                              T *__restrict__ J)
{
    const size_t per = (size_t)F.n * nv, total = nb * per;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t b = t / per;
        const int i = (int)((t % per) / nv), k = (int)(t % nv);
        T *o = J + ((b * F.n + i) * 6) * (size_t)nv + k;
        if (!((F.cols[i][(k >> 6) % kJacMaskWords] >> (k & 63)) & 1)) {
            for (int u = 0; u < 6; u++) o[(size_t)u * nv] = 0;
            continue;
        }
        const T *v = Vx + (((b * nv + k) * F.n) + i) * 12;
        const T ox = F.off[i][0], oy = F.off[i][1], oz = F.off[i][2];
        T y[6] = {v[0], v[1], v[2], v[3] + v[1] * oz - v[2] * oy, v[4] + v[2] * ox - v[0] * oz, v[5] + v[0] * oy - v[1] * ox};
        if (F.world) {
            const T *E = Xa + (b * F.n + i) * 12;
            T z[6];
            for (int u = 0; u < 3; u++) {
                z[u] = E[u] * y[0] + E[3 + u] * y[1] + E[6 + u] * y[2];
                z[3 + u] = E[u] * y[3] + E[3 + u] * y[4] + E[6 + u] * y[5];
            }
            for (int u = 0; u < 6; u++) y[u] = z[u];
        }
        for (int u = 0; u < 6; u++) o[(size_t)u * nv] = y[u];
    }
}

// the drift: one (state, frame) per thread.  Body axes: the spatial acceleration moved to the point, [al ; a + al x o].  World axes:
// [E^T al ; E^T (a + al x o + w x (v + w x o))], the classical acceleration of the point
template <class T>
__global__ void frame_drift_kernel(FrameSet<T> F, const T *__restrict__ V, const T *__restrict__ Xa, size_t nb, T *__restrict__ drift)
{
    const size_t total = nb * (size_t)F.n;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(t % F.n);
        const T *v = V + t * 12, *a = v + 6;
        const T ox = F.off[i][0], oy = F.off[i][1], oz = F.off[i][2];
        T y[6] = {a[0], a[1], a[2], a[3] + a[1] * oz - a[2] * oy, a[4] + a[2] * ox - a[0] * oz, a[5] + a[0] * oy - a[1] * ox};
        if (F.world) {
            const T p[3] = {v[3] + v[1] * oz - v[2] * oy, v[4] + v[2] * ox - v[0] * oz, v[5] + v[0] * oy - v[1] * ox};  // v + w x o
            y[3] += v[1] * p[2] - v[2] * p[1];
            y[4] += v[2] * p[0] - v[0] * p[2];
            y[5] += v[0] * p[1] - v[1] * p[0];
            const T *E = Xa + t * 12;
            T z[6];
            for (int u = 0; u < 3; u++) {
                z[u] = E[u] * y[0] + E[3 + u] * y[1] + E[6 + u] * y[2];
                z[3 + u] = E[u] * y[3] + E[3 + u] * y[4] + E[6 + u] * y[5];
            }
            for (int u = 0; u < 6; u++) y[u] = z[u];
        }
        for (int u = 0; u < 6; u++) drift[t * 6 + u] = y[u];
    }
}

template <class T>
hipError_t launch_frame_jacobian_walk(const JacWalk<T> &W, const T *q, T *J, size_t nb, int grid, hipStream_t stream)
{
    if (nb == 0 || W.n_list == 0) return hipSuccess;
    const size_t lds = (size_t)(W.n_saved + W.n_list) * 12 * kWave * sizeof(T);
    hipLaunchKernelGGL((frame_jacobian_walk_kernel<T>), dim3(grid), dim3(kWave), lds, stream, W, q, J, nb);
    return hipGetLastError();
}
static int element_blocks(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 65535); }
template <class T>
hipError_t launch_frame_jacobian_columns(const FrameSet<T> &F, const T *Vx, const T *Xa, int nv, size_t nb, T *J, hipStream_t stream)
{
    if (nb == 0 || F.n == 0) return hipSuccess;
    hipLaunchKernelGGL((frame_jacobian_columns_kernel<T>), dim3(element_blocks(nb * F.n * nv)), dim3(256), 0, stream, F, Vx, Xa, nv, nb, J);
    return hipGetLastError();
}
template <class T>
hipError_t launch_frame_drift(const FrameSet<T> &F, const T *V, const T *Xa, size_t nb, T *drift, hipStream_t stream)
{
    if (nb == 0 || F.n == 0) return hipSuccess;
    hipLaunchKernelGGL((frame_drift_kernel<T>), dim3(element_blocks(nb * F.n)), dim3(256), 0, stream, F, V, Xa, nb, drift);
    return hipGetLastError();
}
template hipError_t launch_frame_jacobian_walk<float>(const JacWalk<float> &, const float *, float *, size_t, int, hipStream_t);
template hipError_t launch_frame_jacobian_walk<double>(const JacWalk<double> &, const double *, double *, size_t, int, hipStream_t);
template hipError_t launch_frame_jacobian_columns<float>(const FrameSet<float> &, const float *, const float *, int, size_t, float *, hipStream_t);
template hipError_t launch_frame_jacobian_columns<double>(const FrameSet<double> &, const double *, const double *, int, size_t, double *, hipStream_t);
template hipError_t launch_frame_drift<float>(const FrameSet<float> &, const float *, const float *, size_t, float *, hipStream_t);
template hipError_t launch_frame_drift<double>(const FrameSet<double> &, const double *, const double *, size_t, double *, hipStream_t);

}  // namespace grbda_hip
