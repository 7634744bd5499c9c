// wrench_kernels.hip -- the frames of the sparse body wrenches behind grbda_aba_wrench_* / grbda_rnea_wrench_* (include/grbda_hip_wrench.h;
// capi.cpp, wrench_run).
//
// A wrench is a spatial force [moment 3; force 3] on a body.  With Xa = [E 9 | r 3] the body's pose (E: world -> body axes, r: the body's
// origin in world coordinates) -- row i of Xa[nb][n][12], the poses of the LISTED bodies in list order (body_list_kernels.hip) -- the two
// frames are related as the interpreter relates a row of f_ext to the body
// (kernels.hip, subtract_external_force = Xa.transformForceVector, SpatialTransforms.cpp:62-71):
//     world -> body   f_b = E f_w,      n_b = E (n_w - r x f_w)
//     body -> world   f_w = E^T f_b,    n_w = E^T n_b + r x f_w
// wrench_to_body_kernel stands in front of the chain route (the wrench-carrying chain kernels take body-frame wrenches and hold no absolute
// transform); wrench_scatter_kernel builds the dense world-frame chunk fext[nb][n_bodies][6] the interpreter route reads.  Neither is a hot
// path: 12 n scalars per state against the dynamics' thousands of operations.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

// one (state, entry) per thread
template <class T>
__global__ void wrench_to_body_kernel(WrenchList<T> W, const T *__restrict__ Xa, size_t nb, T *__restrict__ out)
{
    const size_t total = nb * (size_t)W.n;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const T *X = Xa + t * 12;  // (entry t = state * n + slot of both arrays)
        const T *w = W.w + t * 6;
        const T f[3] = {w[3], w[4], w[5]}, r[3] = {X[9], X[10], X[11]};
        const T m[3] = {w[0] - (r[1] * f[2] - r[2] * f[1]), w[1] - (r[2] * f[0] - r[0] * f[2]), w[2] - (r[0] * f[1] - r[1] * f[0])};
        T *o = out + t * 6;
        for (int k = 0; k < 3; k++) {
            o[k] = X[3 * k] * m[0] + X[3 * k + 1] * m[1] + X[3 * k + 2] * m[2];
            o[3 + k] = X[3 * k] * f[0] + X[3 * k + 1] * f[1] + X[3 * k + 2] * f[2];
        }
    }
}

// one state per thread, the entries in list order: wrenches on one body add up in that order, and no two threads touch one row
template <class T>
__global__ void wrench_scatter_kernel(WrenchList<T> W, const T *__restrict__ Xa, int from_body, int n_bodies, size_t nb, T *__restrict__ fext)
{
    for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < nb; b += (size_t)gridDim.x * blockDim.x) {
        for (int i = 0; i < W.n; i++) {
            const T *w = W.w + (b * W.n + i) * 6;
            T v[6];
            if (from_body) {
                const T *X = Xa + (b * W.n + i) * 12;
                for (int k = 0; k < 3; k++) {
                    v[k] = X[k] * w[0] + X[3 + k] * w[1] + X[6 + k] * w[2];
                    v[3 + k] = X[k] * w[3] + X[3 + k] * w[4] + X[6 + k] * w[5];
                }
                const T r[3] = {X[9], X[10], X[11]};
                v[0] += r[1] * v[5] - r[2] * v[4];
                v[1] += r[2] * v[3] - r[0] * v[5];
                v[2] += r[0] * v[4] - r[1] * v[3];
            } else {
                for (int k = 0; k < 6; k++) v[k] = w[k];
            }
            T *o = fext + (b * n_bodies + W.body[i]) * 6;
            for (int k = 0; k < 6; k++) o[k] += v[k];
        }
    }
}

static int wrench_grid(size_t threads)
{
    return (int)std::min<size_t>((threads + 255) / 256, 65535);
}
template <class T>
hipError_t launch_wrench_to_body(const WrenchList<T> &W, const T *Xa, size_t nb, T *out, hipStream_t stream)
{
    if (nb == 0 || W.n == 0) return hipSuccess;
    hipLaunchKernelGGL((wrench_to_body_kernel<T>), dim3(wrench_grid(nb * W.n)), dim3(256), 0, stream, W, Xa, nb, out);
    return hipGetLastError();
}
template <class T>
hipError_t launch_wrench_scatter(const WrenchList<T> &W, const T *Xa, int from_body, int n_bodies, size_t nb, T *fext, hipStream_t stream)
{
    if (nb == 0 || W.n == 0) return hipSuccess;
    hipLaunchKernelGGL((wrench_scatter_kernel<T>), dim3(wrench_grid(nb)), dim3(256), 0, stream, W, Xa, from_body, n_bodies, nb, fext);
    return hipGetLastError();
}
template hipError_t launch_wrench_to_body<float>(const WrenchList<float> &, const float *, size_t, float *, hipStream_t);
template hipError_t launch_wrench_to_body<double>(const WrenchList<double> &, const double *, size_t, double *, hipStream_t);
template hipError_t launch_wrench_scatter<float>(const WrenchList<float> &, const float *, int, int, size_t, float *, hipStream_t);
template hipError_t launch_wrench_scatter<double>(const WrenchList<double> &, const double *, int, int, size_t, double *, hipStream_t);

}  // namespace grbda_hip
