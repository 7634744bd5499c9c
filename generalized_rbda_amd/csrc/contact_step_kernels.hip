// contact_step_kernels.hip -- the per-state solve of the scheduled contacts behind grbda_contact_dynamics_active_*,
// grbda_contact_impulse_active_*, grbda_contact_step_* and grbda_contact_rollout_* (include/grbda_hip_contact_step.h; capi.cpp, "scheduled
// contacts").
//
// The contacts are those of contact_kernels.hip -- point cs.off[c] fixed in body cs.body[c] -- and every state b carries a mask active[b]:
// bit c set, contact c is closed in that state.  The kernel reads the LISTED poses Xl[B][n][12] = [E 9 | r 3] and twists Vl[B][n][12] =
// [v 6 | a 6] (body_list_kernels.hip; slot c is the body of contact c, so no body index is read here), and the force-force blocks of the
// inverse operational-space inertia Linv[B][6 n][6 n] of ALL n contact frames.
//
// contact_active_solve_kernel<T, VEL>: one STATE per lane, the packed lower triangle and the right-hand side in dynamic LDS, lane-minor, no
// barrier, nothing in the private segment -- the mapping and the launch record of contact_solve_kernel (contact_solve_launch).  Per state,
// with S the active contacts, m = 3 n:
//     A_ij = (R Linv_ff R^T)_ij + mu delta_ij     both contacts in S
//     A_ij = delta_ij                             either contact not in S
//     rhs  = a_des - kd p_dot - p_ddot            VEL = false (the twists are those at the unconstrained accelerations)
//     rhs  = v_des - (1 + e) p_dot                VEL = true  (the velocity halves alone)
//     rhs  = 0                                    contact not in S
// The rows and columns of an open contact are those of the identity, exactly: the factor keeps them (l_jj = 1, zeros beside it), both
// triangular solves return 0 for them, and what is left is the Cholesky solve of the principal sub-matrix of S -- the sub-list solve of
// contact_solve_kernel / impulse_solve_kernel with terms that are exactly zero added.  The loop bounds depend on n alone, so they stay
// wavefront-uniform whatever the masks of the 64 states are.  A state with an empty set factors the identity: it can never count as a bad
// pivot.  Written: lambda (or the impulses) [B][n][3], exactly 0 off S, and the wrench list [B][n][6] of the sparse-wrench forward dynamics
// in BODY frame (wrench_kernels.hip: f_b = E f_w, n_b = E (n_w - r x f_w), which for a force at p = r + E^T o is [o x (E lambda); E lambda]).
//
// The assembly and the factorisation are a COPY of contact_solve_kernel's text with the masks put in: folding them into device functions
// shared with that kernel and impulse_solve_kernel changed their instruction streams (DESIGN.md 7g'), so they keep their text and this
// kernel has its own.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

namespace {

template <class T>
__device__ __forceinline__ void cross3(const T a[3], const T b[3], T out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace

extern __shared__ __align__(16) unsigned char contact_step_smem[];

// des: a_des / v_des [nb][n][3] or null; c_vel: kd (VEL = false) or 1 + e (VEL = true); g: the plan's gravity, linear part (VEL = false)
template <class T, bool VEL>
__global__ __launch_bounds__(kWave) void contact_active_solve_kernel(ContactSet<T> cs, const T *__restrict__ Linv, const T *__restrict__ Xl,
                                                                     const T *__restrict__ Vl, const T *__restrict__ des,
                                                                     const int *__restrict__ active, T mu, T c_vel, T gx, T gy, T gz, size_t nb,
                                                                     T *__restrict__ out, T *__restrict__ wrench, unsigned long long *bad_count)
{
    const int W = (int)blockDim.x, lane = (int)threadIdx.x;
    const int n = cs.n, m = 3 * n, m6 = 6 * n, tri = m * (m + 1) / 2;
    T *A = reinterpret_cast<T *>(contact_step_smem) + lane;  // packed lower triangle: entry (i, j <= i) at A[(i (i + 1) / 2 + j) W]
    T *y = A + (size_t)tri * W;                              // right-hand side, then lambda: y[i W]
    const T g[3] = {gx, gy, gz};
    for (size_t b = blockIdx.x * (size_t)W + lane; b < nb; b += (size_t)gridDim.x * W) {
        const T *Lb = Linv + b * (size_t)m6 * m6;
        const T *Xb = Xl + b * (size_t)n * 12, *Vb = Vl + b * (size_t)n * 12;
        const unsigned mask = (unsigned)active[b];  // (bits at n and above are never looked at)
        // A = R Linv_ff R^T + mu I on S, the identity off it, block by block of the lower triangle
        for (int c1 = 0; c1 < n; c1++) {
            const bool on1 = (mask >> c1) & 1u;
            T E1[9];
            {
                const T *X1 = Xb + (size_t)c1 * 12;
                for (int i = 0; i < 9; i++) E1[i] = X1[i];
            }
            for (int c2 = 0; c2 <= c1; c2++) {
                const bool on = on1 && ((mask >> c2) & 1u);
                const T *X2 = Xb + (size_t)c2 * 12;
                const T *Lc = Lb + (size_t)(6 * c1 + 3) * m6 + 6 * c2 + 3;
                T tmp[3][3];  // Linv block times E2
                for (int k = 0; k < 3; k++)
                    for (int j = 0; j < 3; j++) tmp[k][j] = Lc[k * m6] * X2[j] + Lc[k * m6 + 1] * X2[3 + j] + Lc[k * m6 + 2] * X2[6 + j];
                for (int i = 0; i < 3; i++) {
                    const int ri = 3 * c1 + i, row = ri * (ri + 1) / 2 + 3 * c2;
                    for (int j = 0; j < 3; j++) {
                        T v = E1[i] * tmp[0][j] + E1[3 + i] * tmp[1][j] + E1[6 + i] * tmp[2][j];
                        if (c1 == c2) {
                            if (j > i) continue;
                            if (j == i) v += mu;
                        }
                        if (!on) v = (c1 == c2 && j == i) ? T(1) : T(0);
                        A[(size_t)(row + j) * W] = v;
                    }
                }
            }
        }
        // the right-hand side, from the twist halves of the contact's own slot
        for (int c = 0; c < n; c++) {
            const bool on = (mask >> c) & 1u;
            const T *E = Xb + (size_t)c * 12, *Wc = Vb + (size_t)c * 12;
            const T o[3] = {cs.off[c][0], cs.off[c][1], cs.off[c][2]};
            const T w[3] = {Wc[0], Wc[1], Wc[2]};
            T u[3], s[3];  // u = v + omega x o: the point's velocity in body axes
            cross3(w, o, u);
            for (int i = 0; i < 3; i++) u[i] += Wc[3 + i];
            if (VEL) {
                for (int i = 0; i < 3; i++) s[i] = c_vel * u[i];
            } else {
                // kd u + a + alpha x o + omega x u: E^T of it is kd p_dot + p_ddot - g
                const T al[3] = {Wc[6], Wc[7], Wc[8]};
                T ao[3], wu[3];
                cross3(al, o, ao);
                cross3(w, u, wu);
                for (int i = 0; i < 3; i++) s[i] = c_vel * u[i] + (Wc[9 + i] + ao[i] + wu[i]);
            }
            for (int i = 0; i < 3; i++) {
                T r = E[i] * s[0] + E[3 + i] * s[1] + E[6 + i] * s[2];
                if (!VEL) r += g[i];
                const T d = des ? des[(b * n + c) * 3 + i] : T(0);
                y[(size_t)(3 * c + i) * W] = on ? d - r : T(0);
            }
        }
        // A = L L^T in place
        bool bad = false;
        for (int j = 0; j < m; j++) {
            const int rj = j * (j + 1) / 2;
            T d = A[(size_t)(rj + j) * W];
            for (int k = 0; k < j; k++) {
                const T l = A[(size_t)(rj + k) * W];
                d -= l * l;
            }
            if (!(d > T(0)) || !(d < T(INFINITY))) bad = true;
            const T ljj = sqrt(d), inv = T(1) / ljj;
            A[(size_t)(rj + j) * W] = ljj;
            for (int i = j + 1; i < m; i++) {
                const int ri = i * (i + 1) / 2;
                T s = A[(size_t)(ri + j) * W];
                for (int k = 0; k < j; k++) s -= A[(size_t)(ri + k) * W] * A[(size_t)(rj + k) * W];
                A[(size_t)(ri + j) * W] = s * inv;
            }
        }
        // L z = rhs, L^T lambda = z
        for (int i = 0; i < m; i++) {
            const int ri = i * (i + 1) / 2;
            T s = y[(size_t)i * W];
            for (int k = 0; k < i; k++) s -= A[(size_t)(ri + k) * W] * y[(size_t)k * W];
            y[(size_t)i * W] = s / A[(size_t)(ri + i) * W];
        }
        for (int i = m - 1; i >= 0; i--) {
            T s = y[(size_t)i * W];
            for (int k = i + 1; k < m; k++) s -= A[(size_t)(k * (k + 1) / 2 + i) * W] * y[(size_t)k * W];
            y[(size_t)i * W] = s / A[(size_t)(i * (i + 1) / 2 + i) * W];
        }
        // a pivot that is not positive or not finite: the state's active contacts get NaN, and it is counted (grbda_spd_bad_pivots)
        if (bad && bad_count) atomicAdd(bad_count, 1ull);
        // lambda and the body-frame wrench of every slot; an open contact writes zeros whatever the solve left in its rows
        for (int c = 0; c < n; c++) {
            const bool on = (mask >> c) & 1u;
            const T *E = Xb + (size_t)c * 12;
            const T o[3] = {cs.off[c][0], cs.off[c][1], cs.off[c][2]};
            T f[3], fb[3], mo[3];
            for (int i = 0; i < 3; i++) {
                f[i] = on ? (bad ? T(NAN) : y[(size_t)(3 * c + i) * W]) : T(0);
                out[(b * n + c) * 3 + i] = f[i];
            }
            for (int i = 0; i < 3; i++) fb[i] = E[3 * i] * f[0] + E[3 * i + 1] * f[1] + E[3 * i + 2] * f[2];
            cross3(o, fb, mo);
            T *wb = wrench + (b * n + c) * 6;
            for (int i = 0; i < 3; i++) {
                wb[i] = on ? mo[i] : T(0);
                wb[3 + i] = on ? fb[i] : T(0);
            }
        }
    }
}

// The contacts a step solves its impact with: every closed contact when any of them closes in this step, none otherwise.
__global__ void impact_mask_kernel(const int *__restrict__ active, const int *__restrict__ prev, int n, size_t nb, int *__restrict__ out)
{
    const unsigned all = (1u << n) - 1u;
    for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < nb; b += (size_t)gridDim.x * blockDim.x) {
        const unsigned a = (unsigned)active[b] & all;
        out[b] = (a & ~(unsigned)prev[b]) ? (int)a : 0;
    }
}

// A state with no closed contact keeps the unconstrained accelerations bit for bit: the forward dynamics that carry the (all-zero) wrench
// list are another kernel than the ones that carry none, and the two agree to rounding only.  A block is kFreeCopyRows states by
// kFreeCopyCols coordinates: threadIdx.y picks the state, whose mask is read once, threadIdx.x strides over its row.
constexpr int kFreeCopyCols = 32, kFreeCopyRows = 8;
template <class T>
__global__ void free_states_copy_kernel(const int *__restrict__ active, int n, const T *__restrict__ ydd_free, int nv, size_t nb,
                                        T *__restrict__ ydd)
{
    const unsigned all = (1u << n) - 1u;
    for (size_t b = blockIdx.x * (size_t)kFreeCopyRows + threadIdx.y; b < nb; b += (size_t)gridDim.x * kFreeCopyRows) {
        if (((unsigned)active[b] & all) != 0) continue;
        for (int j = (int)threadIdx.x; j < nv; j += kFreeCopyCols) ydd[b * (size_t)nv + j] = ydd_free[b * (size_t)nv + j];
    }
}

static int elementwise_grid(size_t threads)
{
    return (int)std::min<size_t>((threads + 255) / 256, 65535);
}

// The launch is contact_solve_kernel's (contact_solve_launch: the LDS footprint is the same triangle and one right-hand side).  As for
// that kernel, the trip of the grid-stride loop past the grid cap (n_cu x per_cu workgroups) is not reached by the batch sizes of the tests.
template <class T>
hipError_t launch_contact_active_solve(bool vel, const ContactSet<T> &cs, const T *Linv, const T *Xl, const T *Vl, const T *des, const int *active,
                                       T mu, T c_vel, const T g[3], size_t nb, T *out, T *wrench, unsigned long long *bad_count, int n_cu,
                                       hipStream_t stream)
{
    const ContactSolveLaunch L = contact_solve_launch(cs.n, sizeof(T));
    if (L.lanes == 0) return hipErrorInvalidValue;
    const size_t grid = std::min(static_cast<size_t>(n_cu) * L.per_cu, (nb + L.lanes - 1) / L.lanes);
    if (vel)
        hipLaunchKernelGGL((contact_active_solve_kernel<T, true>), dim3(static_cast<unsigned>(grid)), dim3(L.lanes), L.lds_bytes, stream, cs, Linv, Xl,
                           Vl, des, active, mu, c_vel, g[0], g[1], g[2], nb, out, wrench, bad_count);
    else
        hipLaunchKernelGGL((contact_active_solve_kernel<T, false>), dim3(static_cast<unsigned>(grid)), dim3(L.lanes), L.lds_bytes, stream, cs, Linv, Xl,
                           Vl, des, active, mu, c_vel, g[0], g[1], g[2], nb, out, wrench, bad_count);
    return hipGetLastError();
}
hipError_t launch_impact_mask(const int *active, const int *prev, int n, size_t nb, int *out, hipStream_t stream)
{
    hipLaunchKernelGGL(impact_mask_kernel, dim3(elementwise_grid(nb)), dim3(256), 0, stream, active, prev, n, nb, out);
    return hipGetLastError();
}
template <class T>
hipError_t launch_free_states_copy(const int *active, int n, const T *ydd_free, int nv, size_t nb, T *ydd, hipStream_t stream)
{
    const int blocks = (int)std::min<size_t>((nb + kFreeCopyRows - 1) / kFreeCopyRows, 65535);
    hipLaunchKernelGGL((free_states_copy_kernel<T>), dim3(blocks), dim3(kFreeCopyCols, kFreeCopyRows), 0, stream, active, n, ydd_free, nv, nb, ydd);
    return hipGetLastError();
}
template hipError_t launch_contact_active_solve<float>(bool, const ContactSet<float> &, const float *, const float *, const float *, const float *,
                                                       const int *, float, float, const float[3], size_t, float *, float *, unsigned long long *, int,
                                                       hipStream_t);
template hipError_t launch_contact_active_solve<double>(bool, const ContactSet<double> &, const double *, const double *, const double *,
                                                        const double *, const int *, double, double, const double[3], size_t, double *, double *,
                                                        unsigned long long *, int, hipStream_t);
template hipError_t launch_free_states_copy<float>(const int *, int, const float *, int, size_t, float *, hipStream_t);
template hipError_t launch_free_states_copy<double>(const int *, int, const double *, int, size_t, double *, hipStream_t);

// the solves ask for more dynamic LDS than the 64 KiB default (per device, as set_max_dynamic_lds_contact)
hipError_t set_max_dynamic_lds_contact_step()
{
    for (const void *f : {reinterpret_cast<const void *>(&contact_active_solve_kernel<float, false>),
                          reinterpret_cast<const void *>(&contact_active_solve_kernel<float, true>),
                          reinterpret_cast<const void *>(&contact_active_solve_kernel<double, false>),
                          reinterpret_cast<const void *>(&contact_active_solve_kernel<double, true>)}) {
        hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace grbda_hip
