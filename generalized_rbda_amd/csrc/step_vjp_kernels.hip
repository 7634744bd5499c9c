// step_vjp_kernels.hip -- the two kernels of the step / rollout vector-Jacobian products (include/grbda_hip_step_vjp.h), and
// integrate_jvp_kernel, the forward map of the first (include/grbda_hip_jvp.h; described where it stands).
//
// integrate_vjp_kernel: the cotangents (g_q', g_qd') of a stepped state pulled back through qd' = qd + dt ydd, q' = q (+) dt qd'.  One
// thread per scalar of [B][nv], consecutive threads consecutive addresses.  Explicit coordinates are element-wise:
//     g_v = g_qd' + dt g_q',   grad_q = g_q',   grad_qd = g_v,   grad_ydd = dt g_v.
// The six coordinates of a quaternion base are done by the thread of the base's first coordinate, in registers (the five threads behind
// it do nothing): with phi = omega' dt, theta = |phi|, E = I + a [phi]x + b [phi]x^2 and J_r^T = I + b [phi]x + c [phi]x^2,
//     a = sin(theta) / theta,   b = 2 (sin(theta / 2) / theta)^2,   c = (theta - sin(theta)) / theta^3  (its series below kSeriesBelow),
//     grad_q[rot] = E g_r' + dt v' x (E g_p'),   grad_q[pos] = E g_p',   g_v[omega] = g_qd'[omega] + dt J_r^T g_r',   g_v[v] = g_qd'[v] + dt E g_p'
// and a = 1, b = 1/2, c = 1/6 at theta = 0 (E = J_r = I).  Only qd' and dt enter.  No LDS, no atomics, no scratch.  Every output is
// optional and computed the same way whichever others are asked for: a subset of the outputs has the bits of the full call.
//
// vjp_add_kernel: out = a + b, one rounding.  The sums of grbda_step_vjp_* and of the loop of grbda_rollout_vjp_* all go through it, so the
// two cannot round differently; there is no multiplication for the compiler to fuse with.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

namespace {

constexpr int kStepVjpThreads = 256;
constexpr size_t kStepVjpMaxGrid = size_t(1) << 20;  // beyond that the threads stride over the array

template <class T>
__device__ inline void cross3(const T a[3], const T b[3], T out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
// (I + k1 [phi]x + k2 [phi]x^2) g
template <class T>
__device__ inline void rodrigues(const T phi[3], T k1, T k2, const T g[3], T out[3])
{
    T x1[3], x2[3];
    cross3(phi, g, x1);
    cross3(phi, x1, x2);
    for (int i = 0; i < 3; i++) out[i] = g[i] + k1 * x1[i] + k2 * x2[i];
}

// phi = w dt, and the coefficients a, b, c of E and J_r at theta = |phi| (a = 1, b = 1/2, c = 1/6 at theta = 0; c by its series below 0.1):
// the one evaluation integrate_vjp_kernel and integrate_jvp_kernel share
template <class T>
__device__ inline void so3_coefficients(const T w[3], T dt, T phi[3], T &ka, T &kb, T &kc)
{
    constexpr T kSeriesBelow = T(0.1);
    for (int a = 0; a < 3; a++) phi[a] = w[a] * dt;
    const T theta = sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    ka = T(1), kb = T(0.5), kc = T(1.0 / 6.0);
    if (theta > T(0)) {
        const T sn = sin(theta), sh = sin(T(0.5) * theta) / theta, t2 = theta * theta;
        ka = sn / theta;
        kb = T(2) * sh * sh;
        kc = theta < kSeriesBelow ? T(1.0 / 6.0) - t2 * (T(1.0 / 120.0) - t2 * T(1.0 / 5040.0)) : (theta - sn) / (t2 * theta);
    }
}

template <class T>
__global__ void __launch_bounds__(kStepVjpThreads) integrate_vjp_kernel(const ClusterRec *__restrict__ base, const T *__restrict__ qd_next, T dt,
                                                                        const T *__restrict__ g_q, const T *__restrict__ g_qd,
                                                                        T *__restrict__ grad_q, T *__restrict__ grad_qd,
                                                                        T *__restrict__ grad_ydd, int nv, size_t n)
{
    const int bv = base ? base->v_index : -1;  // (wave-uniform: one record)
    const size_t stride = static_cast<size_t>(gridDim.x) * kStepVjpThreads;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kStepVjpThreads + threadIdx.x; i < n; i += stride) {
        const int j = static_cast<int>(i % static_cast<size_t>(nv));
        if (bv >= 0 && j >= bv && j < bv + 6) {
            if (j != bv) continue;
            T w[3], v[3], gr[3], gp[3], hw[3], hv[3];  // i .. i + 5 are this state's base entries: bv + 6 <= nv
            for (int a = 0; a < 3; a++) {
                w[a] = qd_next[i + a];
                v[a] = qd_next[i + 3 + a];
                gr[a] = g_q ? g_q[i + a] : T(0);
                gp[a] = g_q ? g_q[i + 3 + a] : T(0);
                hw[a] = g_qd ? g_qd[i + a] : T(0);
                hv[a] = g_qd ? g_qd[i + 3 + a] : T(0);
            }
            T phi[3], ka, kb, kc;
            so3_coefficients(w, dt, phi, ka, kb, kc);
            T Egr[3], Egp[3], Jgr[3], vx[3];
            rodrigues(phi, ka, kb, gr, Egr);
            rodrigues(phi, ka, kb, gp, Egp);
            rodrigues(phi, kb, kc, gr, Jgr);
            cross3(v, Egp, vx);
            for (int a = 0; a < 3; a++) {
                const T gw = hw[a] + dt * Jgr[a], gl = hv[a] + dt * Egp[a];
                if (grad_q) {
                    grad_q[i + a] = Egr[a] + dt * vx[a];
                    grad_q[i + 3 + a] = Egp[a];
                }
                if (grad_qd) {
                    grad_qd[i + a] = gw;
                    grad_qd[i + 3 + a] = gl;
                }
                if (grad_ydd) {
                    grad_ydd[i + a] = dt * gw;
                    grad_ydd[i + 3 + a] = dt * gl;
                }
            }
            continue;
        }
        const T gq = g_q ? g_q[i] : T(0);
        const T gv = (g_qd ? g_qd[i] : T(0)) + dt * gq;
        if (grad_q) grad_q[i] = gq;
        if (grad_qd) grad_qd[i] = gv;
        if (grad_ydd) grad_ydd[i] = dt * gv;
    }
}

// The forward map of the same step (include/grbda_hip_jvp.h), shaped as its twin above: one thread per scalar, the six base coordinates in
// the registers of the thread of the first.  E^T = I - a [phi]x + b [phi]x^2 and J_r = I - b [phi]x + c [phi]x^2 are the transposes of what
// the pull-back applies, so the same rodrigues() with the first coefficient negated:
//     dqd' = dqd + dt dydd,   d' = d + dt dqd',   d_r' = E^T d_r + dt J_r dw',   d_p' = E^T (d_p - dt v' x d_r + dt dv').
template <class T>
__global__ void __launch_bounds__(kStepVjpThreads) integrate_jvp_kernel(const ClusterRec *__restrict__ base, const T *__restrict__ qd_next, T dt,
                                                                        const T *__restrict__ dq, const T *__restrict__ dqd,
                                                                        const T *__restrict__ dydd, T *__restrict__ dq_next,
                                                                        T *__restrict__ dqd_next, int nv, size_t n)
{
    const int bv = base ? base->v_index : -1;  // (wave-uniform: one record)
    const size_t stride = static_cast<size_t>(gridDim.x) * kStepVjpThreads;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kStepVjpThreads + threadIdx.x; i < n; i += stride) {
        const int j = static_cast<int>(i % static_cast<size_t>(nv));
        if (bv >= 0 && j >= bv && j < bv + 6) {
            if (j != bv) continue;
            T w[3], v[3], dr[3], dp[3], dw[3], dv[3];  // i .. i + 5 are this state's base entries: bv + 6 <= nv
            for (int a = 0; a < 3; a++) {
                w[a] = qd_next[i + a];
                v[a] = qd_next[i + 3 + a];
                dr[a] = dq ? dq[i + a] : T(0);
                dp[a] = dq ? dq[i + 3 + a] : T(0);
                dw[a] = (dqd ? dqd[i + a] : T(0)) + dt * (dydd ? dydd[i + a] : T(0));
                dv[a] = (dqd ? dqd[i + 3 + a] : T(0)) + dt * (dydd ? dydd[i + 3 + a] : T(0));
            }
            T phi[3], ka, kb, kc;
            so3_coefficients(w, dt, phi, ka, kb, kc);
            T Edr[3], Jdw[3], vx[3], t[3], Et[3];
            rodrigues(phi, -ka, kb, dr, Edr);
            rodrigues(phi, -kb, kc, dw, Jdw);
            cross3(v, dr, vx);
            for (int a = 0; a < 3; a++) t[a] = dp[a] - dt * vx[a] + dt * dv[a];
            rodrigues(phi, -ka, kb, t, Et);
            for (int a = 0; a < 3; a++) {
                if (dq_next) {
                    dq_next[i + a] = Edr[a] + dt * Jdw[a];
                    dq_next[i + 3 + a] = Et[a];
                }
                if (dqd_next) {
                    dqd_next[i + a] = dw[a];
                    dqd_next[i + 3 + a] = dv[a];
                }
            }
            continue;
        }
        const T vn = (dqd ? dqd[i] : T(0)) + dt * (dydd ? dydd[i] : T(0));
        if (dq_next) dq_next[i] = (dq ? dq[i] : T(0)) + dt * vn;
        if (dqd_next) dqd_next[i] = vn;
    }
}

template <class T>
__global__ void __launch_bounds__(kStepVjpThreads) vjp_add_kernel(const T *a, const T *b, T *out, size_t n)
{
    const size_t stride = static_cast<size_t>(gridDim.x) * kStepVjpThreads;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kStepVjpThreads + threadIdx.x; i < n; i += stride) out[i] = a[i] + b[i];
}

unsigned step_vjp_grid(size_t n)
{
    return static_cast<unsigned>(std::min((n + kStepVjpThreads - 1) / kStepVjpThreads, kStepVjpMaxGrid));
}

}  // namespace

template <class T>
hipError_t launch_integrate_vjp(const ClusterRec *base, const T *qd_next, T dt, const T *g_q, const T *g_qd, T *grad_q, T *grad_qd, T *grad_ydd,
                                int nv, size_t nb, hipStream_t stream)
{
    const size_t n = nb * static_cast<size_t>(nv);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((integrate_vjp_kernel<T>), dim3(step_vjp_grid(n)), dim3(kStepVjpThreads), 0, stream, base, qd_next, dt, g_q, g_qd, grad_q, grad_qd,
                       grad_ydd, nv, n);
    return hipGetLastError();
}
template hipError_t launch_integrate_vjp<float>(const ClusterRec *, const float *, float, const float *, const float *, float *, float *, float *, int,
                                                size_t, hipStream_t);
template hipError_t launch_integrate_vjp<double>(const ClusterRec *, const double *, double, const double *, const double *, double *, double *, double *,
                                                 int, size_t, hipStream_t);

template <class T>
hipError_t launch_integrate_jvp(const ClusterRec *base, const T *qd_next, T dt, const T *dq, const T *dqd, const T *dydd, T *dq_next, T *dqd_next,
                                int nv, size_t nb, hipStream_t stream)
{
    const size_t n = nb * static_cast<size_t>(nv);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((integrate_jvp_kernel<T>), dim3(step_vjp_grid(n)), dim3(kStepVjpThreads), 0, stream, base, qd_next, dt, dq, dqd, dydd, dq_next,
                       dqd_next, nv, n);
    return hipGetLastError();
}
template hipError_t launch_integrate_jvp<float>(const ClusterRec *, const float *, float, const float *, const float *, const float *, float *, float *, int,
                                                size_t, hipStream_t);
template hipError_t launch_integrate_jvp<double>(const ClusterRec *, const double *, double, const double *, const double *, const double *, double *,
                                                 double *, int, size_t, hipStream_t);

template <class T>
hipError_t launch_vjp_add(const T *a, const T *b, T *out, size_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((vjp_add_kernel<T>), dim3(step_vjp_grid(n)), dim3(kStepVjpThreads), 0, stream, a, b, out, n);
    return hipGetLastError();
}
template hipError_t launch_vjp_add<float>(const float *, const float *, float *, size_t, hipStream_t);
template hipError_t launch_vjp_add<double>(const double *, const double *, double *, size_t, hipStream_t);

}  // namespace grbda_hip
