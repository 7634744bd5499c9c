// frame_product_kernels.hip -- the products J v and J^T f with the frame Jacobians of a listed few body frames, J itself never formed
// (include/grbda_hip_jacobian_products.h; capi.cpp, frame_products_run).  J is the J of frame_jacobian_kernels.hip for the same list.
//
// Route 0, frame_product_walk_kernel: the execution model of frame_jacobian_walk_kernel -- one state per lane, one-wavefront workgroups, a
// grid-stride loop over tiles of 64 states, the walk (walk.h, JacWalkStep; devplan.h, JacWalk) in the kernel arguments, every branch on it
// a scalar branch, no per-lane array indexed at run time, LDS through walk_dev.h (a lane reads what it wrote: no barrier).  Everything is
// done in WORLD coordinates about the world origin, where the axes of a root path add:
//   pass 1  the poses of the root paths (walk_pose_step) and, for J v, next to the running pose the running world twist
//           Tw += (sum_a G[a] v[v_col + a]) [w ; r x w]  (the base: its six axes times v[v_col .. v_col + 5]),
//           saved and restored with the pose at branch points.  A listed frame with point p stores [w ; m + w x p] (body axes: turned with
//           E, permuted to the reference's axes) -- Jv, six stores per frame -- and, for J^T f, turns its wrench into the world wrench about
//           the world origin, F_w = E^T f_lin, N_w = E^T f_ang + p x F_w, which it leaves in the frame's six LDS rows;
//   pass 2  (J^T f) the poses again and the cluster's world-frame axes A[a] as in frame_jacobian_walk_kernel; a run of in-cluster steps adds
//           A[a] . sum over the frames in `emit` of [N_w ; F_w] into one register per column and adds it to tau[v_col + a] when the walk
//           leaves the cluster.  Two runs may meet the same cluster (a link and its rotor, both children of the link before), so tau is
//           zeroed first and every run ADDS to it; a lane reads back only what it wrote itself.
// LDS rows of kWave lanes: saved poses [0, 12 n_saved), saved twists [12 n_saved, 18 n_saved), frame wrenches [18 n_saved, 18 n_saved + 6 n).
//
// Route 1: element-wise finishing kernels over the listed twists at (q, v, 0) (J v) and over a chunk's J of the existing route-1 path
// (J^T f).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

#include "devmath.h"
#include "walk_dev.h"

template <class T, bool JV, bool JTF>
__global__ __launch_bounds__(kWave, 1) void frame_product_walk_kernel(JacWalk<T> W, const T *__restrict__ q, const T *__restrict__ v,
                                                                      const T *__restrict__ f, T *__restrict__ Jv, T *JTf, size_t B)
{
    cptr<T> consts = (cptr<T>)W.consts;
    const int lane = threadIdx.x;
    const size_t n_tiles = (B + kWave - 1) / kWave, nv = (size_t)W.nv;
    const int tw_row = W.n_saved * 12, fr_row = W.n_saved * 18;
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t r = tile * kWave + lane;
        if (r >= B) continue;  // (no cross-lane operation below)
        const T *qr = q + r * (size_t)W.nq;
        const T *vr = JV ? v + r * nv : nullptr;
        T X[12], Tw[6];
#pragma unroll
        for (int k = 0; k < 12; k++) X[k] = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) Tw[k] = 0;
        // pass 1: the poses; the running twist and Jv; the frames' world wrenches
        for (int s = 0; s < W.n_steps; s++) {
            const JacWalkStep st = W.step[s];
            if (JV) {
                if (st.restore != kWalkNone) rows6_get(tw_row + st.restore * 6, lane, Tw);
                if (st.root) {
#pragma unroll
                    for (int k = 0; k < 6; k++) Tw[k] = 0;
                }
            }
            walk_pose_step(st, consts, W.ori_repr, qr, lane, X);
            if (JV) {
                if (st.free) {
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const T w[3] = {X[3 * j], X[3 * j + 1], X[3 * j + 2]};
                        const T a = vr[st.v_col + j], l = vr[st.v_col + 3 + j];
                        Tw[0] += a * w[0];
                        Tw[1] += a * w[1];
                        Tw[2] += a * w[2];
                        Tw[3] += a * (X[10] * w[2] - X[11] * w[1]) + l * w[0];
                        Tw[4] += a * (X[11] * w[0] - X[9] * w[2]) + l * w[1];
                        Tw[5] += a * (X[9] * w[1] - X[10] * w[0]) + l * w[2];
                    }
                } else {
                    const T w0 = st.axis == 0 ? X[0] : st.axis == 1 ? X[3] : X[6];
                    const T w1 = st.axis == 0 ? X[1] : st.axis == 1 ? X[4] : X[7];
                    const T w2 = st.axis == 0 ? X[2] : st.axis == 1 ? X[5] : X[8];
                    cptr<T> G = consts + st.cofs + kBodyConstFixed;
                    T c = 0;
#pragma unroll
                    for (int a = 0; a < kJacMaxDof; a++)
                        if (a < st.n) c += G[a] * vr[st.v_col + a];
                    Tw[0] += c * w0;
                    Tw[1] += c * w1;
                    Tw[2] += c * w2;
                    Tw[3] += c * (X[10] * w2 - X[11] * w1);
                    Tw[4] += c * (X[11] * w0 - X[9] * w2);
                    Tw[5] += c * (X[9] * w1 - X[10] * w0);
                }
                if (st.save != kWalkNone) rows6_put(tw_row + st.save * 6, lane, Tw);
            }
            if (st.own == 0) continue;
            for (int i = 0; i < W.n_list; i++) {
                if (!((st.own >> i) & 1)) continue;
                const T ox = W.off[i][0], oy = W.off[i][1], oz = W.off[i][2];
                T p[3];
#pragma unroll
                for (int u = 0; u < 3; u++) p[u] = X[9 + u] + X[u] * ox + X[3 + u] * oy + X[6 + u] * oz;
                // component u of a vector in the plan's body axes is component to[u] in the reference's
                const int canon = (int)W.canon[i];
                const int to[3] = {(canon + 1) % 3, (canon + 2) % 3, canon % 3};
                if (JV) {
                    const T y[3] = {Tw[3] + Tw[1] * p[2] - Tw[2] * p[1], Tw[4] + Tw[2] * p[0] - Tw[0] * p[2], Tw[5] + Tw[0] * p[1] - Tw[1] * p[0]};
                    T *o = Jv + (r * (size_t)W.n_list + i) * 6;
                    if (W.world) {
#pragma unroll
                        for (int u = 0; u < 3; u++) {
                            o[u] = Tw[u];
                            o[3 + u] = y[u];
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < 3; u++) {
                            o[to[u]] = X[3 * u] * Tw[0] + X[3 * u + 1] * Tw[1] + X[3 * u + 2] * Tw[2];
                            o[3 + to[u]] = X[3 * u] * y[0] + X[3 * u + 1] * y[1] + X[3 * u + 2] * y[2];
                        }
                    }
                }
                if (JTF) {
                    const T *fi = f + (r * (size_t)W.n_list + i) * 6;
                    T Wr[6];  // [N_w ; F_w]
                    if (W.world) {
#pragma unroll
                        for (int u = 0; u < 6; u++) Wr[u] = fi[u];
                    } else {
                        const T na[3] = {fi[to[0]], fi[to[1]], fi[to[2]]}, fa[3] = {fi[3 + to[0]], fi[3 + to[1]], fi[3 + to[2]]};
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            Wr[k] = X[k] * na[0] + X[3 + k] * na[1] + X[6 + k] * na[2];
                            Wr[3 + k] = X[k] * fa[0] + X[3 + k] * fa[1] + X[6 + k] * fa[2];
                        }
                    }
                    Wr[0] += p[1] * Wr[5] - p[2] * Wr[4];
                    Wr[1] += p[2] * Wr[3] - p[0] * Wr[5];
                    Wr[2] += p[0] * Wr[4] - p[1] * Wr[3];
                    rows6_put(fr_row + i * 6, lane, Wr);
                }
            }
        }
        if (!JTF) continue;
        // pass 2: tau = sum over the frames of (world axis) . (world wrench)
        T *tr = JTf + r * nv;
        for (int c = 0; c < W.nv; c++) tr[c] = 0;
        T A[kJacMaxDof][6], acc[kJacMaxDof];
#pragma unroll
        for (int a = 0; a < kJacMaxDof; a++) {
            acc[a] = 0;
#pragma unroll
            for (int u = 0; u < 6; u++) A[a][u] = 0;
        }
        for (int s = 0; s < W.n_steps; s++) {
            const JacWalkStep st = W.step[s];
            walk_pose_step(st, consts, W.ori_repr, qr, lane, X);
            // the wrenches that take this step's columns, summed: the base gives its columns to every frame below it
            const unsigned take = st.free ? st.below : st.emit;
            T Ws[6];
#pragma unroll
            for (int u = 0; u < 6; u++) Ws[u] = 0;
            for (int i = 0; i < W.n_list; i++) {
                if (!((take >> i) & 1)) continue;
                T Wr[6];
                rows6_get(fr_row + i * 6, lane, Wr);
#pragma unroll
                for (int u = 0; u < 6; u++) Ws[u] += Wr[u];
            }
            if (st.free) {
                T *o = tr + st.v_col;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const T w[3] = {X[3 * j], X[3 * j + 1], X[3 * j + 2]};
                    const T m[3] = {X[10] * w[2] - X[11] * w[1], X[11] * w[0] - X[9] * w[2], X[9] * w[1] - X[10] * w[0]};
                    o[j] += w[0] * Ws[0] + w[1] * Ws[1] + w[2] * Ws[2] + m[0] * Ws[3] + m[1] * Ws[4] + m[2] * Ws[5];
                    o[3 + j] += w[0] * Ws[3] + w[1] * Ws[4] + w[2] * Ws[5];
                }
                continue;
            }
            const T w0 = st.axis == 0 ? X[0] : st.axis == 1 ? X[3] : X[6];
            const T w1 = st.axis == 0 ? X[1] : st.axis == 1 ? X[4] : X[7];
            const T w2 = st.axis == 0 ? X[2] : st.axis == 1 ? X[5] : X[8];
            const T S[6] = {w0, w1, w2, X[10] * w2 - X[11] * w1, X[11] * w0 - X[9] * w2, X[9] * w1 - X[10] * w0};
            cptr<T> G = consts + st.cofs + kBodyConstFixed;
            const bool leaves = s + 1 == W.n_steps || !W.step[s + 1].cont;  // the next step is not this body's in-cluster child
#pragma unroll
            for (int a = 0; a < kJacMaxDof; a++) {
                if (a < st.n) {
                    const T g = G[a];
#pragma unroll
                    for (int u = 0; u < 6; u++) A[a][u] = st.cont ? A[a][u] + g * S[u] : g * S[u];
                    T d = 0;
#pragma unroll
                    for (int u = 0; u < 6; u++) d += A[a][u] * Ws[u];
                    acc[a] = st.cont ? acc[a] + d : d;
                    if (leaves) tr[st.v_col + a] += acc[a];
                }
            }
        }
    }
}

// route 1, J v: one (state, frame) per thread.  V[nb][n][12], the listed twists at (q, v, 0) in the reference's body axes; the velocity half
// moved to the point, [w ; v + w x o]; world frames turn it with the listed poses, [E^T w ; E^T (v + w x o)]
template <class T>
__global__ void frame_jv_kernel(FrameSet<T> F, const T *__restrict__ V, const T *__restrict__ Xa, size_t nb, T *__restrict__ Jv)
{
    const size_t total = nb * (size_t)F.n;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(t % F.n);
        const T *x = V + t * 12;
        const T ox = F.off[i][0], oy = F.off[i][1], oz = F.off[i][2];
        T y[6] = {x[0], x[1], x[2], x[3] + x[1] * oz - x[2] * oy, x[4] + x[2] * ox - x[0] * oz, x[5] + x[0] * oy - x[1] * ox};
        if (F.world) {
            const T *E = Xa + t * 12;
            T z[6];
            for (int u = 0; u < 3; u++) {
                z[u] = E[u] * y[0] + E[3 + u] * y[1] + E[6 + u] * y[2];
                z[3 + u] = E[u] * y[3] + E[3 + u] * y[4] + E[6 + u] * y[5];
            }
            for (int u = 0; u < 6; u++) y[u] = z[u];
        }
        for (int u = 0; u < 6; u++) Jv[t * 6 + u] = y[u];
    }
}

// route 1, J^T f: one (state, column) per thread, consecutive threads on consecutive columns.  J[nb][n][6][nv], f[nb][n][6] -> JTf[nb][nv]
template <class T>
__global__ void frame_jtf_kernel(const T *__restrict__ J, const T *__restrict__ f, int n, int nv, size_t nb, T *__restrict__ JTf)
{
    const size_t total = nb * (size_t)nv;
    const int rows = n * 6;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t b = t / nv;
        const int k = (int)(t % nv);
        const T *Jb = J + b * (size_t)rows * nv + k, *fb = f + b * (size_t)rows;
        T sum = 0;
        for (int u = 0; u < rows; u++) sum += Jb[(size_t)u * nv] * fb[u];
        JTf[t] = sum;
    }
}

// dynamic LDS of the walk: (18 n_saved + 6 n_list) rows of kWave lanes
template <class T>
hipError_t launch_frame_product_walk(const JacWalk<T> &W, const T *q, const T *v, const T *f, T *Jv, T *JTf, size_t nb, int grid,
                                     hipStream_t stream)
{
    if (nb == 0 || W.n_list == 0 || (!Jv && !JTf)) return hipSuccess;
    const size_t lds = (size_t)(18 * W.n_saved + 6 * W.n_list) * kWave * sizeof(T);
    if (Jv && JTf) hipLaunchKernelGGL((frame_product_walk_kernel<T, true, true>), dim3(grid), dim3(kWave), lds, stream, W, q, v, f, Jv, JTf, nb);
    else if (Jv) hipLaunchKernelGGL((frame_product_walk_kernel<T, true, false>), dim3(grid), dim3(kWave), lds, stream, W, q, v, f, Jv, JTf, nb);
    else hipLaunchKernelGGL((frame_product_walk_kernel<T, false, true>), dim3(grid), dim3(kWave), lds, stream, W, q, v, f, Jv, JTf, nb);
    return hipGetLastError();
}
static int element_blocks(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 65535); }
template <class T>
hipError_t launch_frame_jv(const FrameSet<T> &F, const T *V, const T *Xa, size_t nb, T *Jv, hipStream_t stream)
{
    if (nb == 0 || F.n == 0) return hipSuccess;
    hipLaunchKernelGGL((frame_jv_kernel<T>), dim3(element_blocks(nb * F.n)), dim3(256), 0, stream, F, V, Xa, nb, Jv);
    return hipGetLastError();
}
template <class T>
hipError_t launch_frame_jtf(const T *J, const T *f, int n, int nv, size_t nb, T *JTf, hipStream_t stream)
{
    if (nb == 0 || n == 0 || nv == 0) return hipSuccess;
    hipLaunchKernelGGL((frame_jtf_kernel<T>), dim3(element_blocks(nb * nv)), dim3(256), 0, stream, J, f, n, nv, nb, JTf);
    return hipGetLastError();
}
template hipError_t launch_frame_product_walk<float>(const JacWalk<float> &, const float *, const float *, const float *, float *, float *, size_t, int,
                                                     hipStream_t);
template hipError_t launch_frame_product_walk<double>(const JacWalk<double> &, const double *, const double *, const double *, double *, double *, size_t,
                                                      int, hipStream_t);
template hipError_t launch_frame_jv<float>(const FrameSet<float> &, const float *, const float *, size_t, float *, hipStream_t);
template hipError_t launch_frame_jv<double>(const FrameSet<double> &, const double *, const double *, size_t, double *, hipStream_t);
template hipError_t launch_frame_jtf<float>(const float *, const float *, int, int, size_t, float *, hipStream_t);
template hipError_t launch_frame_jtf<double>(const double *, const double *, int, int, size_t, double *, hipStream_t);

}  // namespace grbda_hip
