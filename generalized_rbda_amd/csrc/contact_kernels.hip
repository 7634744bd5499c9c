// contact_kernels.hip -- contact-point kinematics and the per-state contact solve behind grbda_contact_points_* and
// grbda_contact_dynamics_* (include/grbda_hip.h "contact side"; capi.cpp, contact_points / contact_dynamics).
//
// Both kernels read what the engine already computes per state: the body poses Xa[B][n_bodies][12] = [E 9 | r 3] (poses_kernel), the body
// twists V[B][n_bodies][12] = [v 6 | a 6] in body axes with a carrying -gravity (twists_kernel), and, for the solve, the inverse
// operational-space inertia Linv[B][6 n][6 n] of the contact frames (grbda_inv_osim_*).  A contact c is the point cs.off[c] fixed in body
// cs.body[c]; with E, r of that body, o the offset, [omega; v] and [alpha; a] its twist halves and g the plan's gravity:
//     p      = r + E^T o
//     p_dot  = E^T (v + omega x o)
//     p_ddot = E^T (a + alpha x o + omega x (v + omega x o)) + g
// (TreeModel::contactPointForwardKinematics / contactPointForwardAccelerationKinematics, TreeModel.cpp:59-100, in body axes).
//
// contact_solve_kernel: one STATE per lane, as in the rest of the engine.  Per state, with m = 3 n:
//     A   = R Linv_ff R^T + mu I     (R = blockdiag E_c^T; only the force-force 3 x 3 blocks of Linv are read)
//     rhs = a_des - p_ddot           (the twists are those at the unconstrained accelerations)
//     lambda = A^-1 rhs              by Cholesky, in place
//     wrench row [n_bodies][6] = the caller's f_ext (or zeros) + [p x lambda_c ; lambda_c] on body[c], contacts on one body accumulating
// The packed lower triangle of A (m (m + 1) / 2 <= 300 entries) and the right-hand side live in dynamic LDS, lane-minor ([entry][lane]):
// lane l only ever touches column l, so every access is conflict-free and the kernel needs no barrier.  m is a run-time loop bound; the
// triangle is indexed through LDS addresses, never through a per-lane array, so nothing goes to the private segment.  A workgroup is one
// (possibly partial) wavefront of `lanes` states: contact_solve_lanes() picks 64, 32 or 16 so that the most states are resident per CU
// within its 160 KiB of LDS (fp64 with 8 contacts does not fit 64 lanes at all).
//
// impulse_solve_kernel (grbda_contact_impulse_*): the same mapping, matrix and factorisation with the velocity-level right-hand side
// v_des - (1 + e) p_dot; impulse_finish_kernel adds the velocity change to qd.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

namespace {

// E^T x for E = X[0..8] row-major (v_body = E v_world)
template <class T>
__device__ __forceinline__ void rot_t(const T *E, const T x[3], T out[3])
{
    for (int i = 0; i < 3; i++) out[i] = E[i] * x[0] + E[3 + i] * x[1] + E[6 + i] * x[2];
}
template <class T>
__device__ __forceinline__ void cross3(const T a[3], const T b[3], T out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
// u = v + omega x o (body axes): the point's velocity
template <class T>
__device__ __forceinline__ void point_velocity(const T *W, const T o[3], T u[3])
{
    const T w[3] = {W[0], W[1], W[2]};
    cross3(w, o, u);
    for (int i = 0; i < 3; i++) u[i] += W[3 + i];
}
// classical acceleration of the point in world axes (gravity added back)
template <class T>
__device__ __forceinline__ void point_acceleration(const T *E, const T *W, const T o[3], const T g[3], T acc[3])
{
    const T w[3] = {W[0], W[1], W[2]}, al[3] = {W[6], W[7], W[8]};
    T u[3], ao[3], wu[3], s[3];
    point_velocity(W, o, u);
    cross3(al, o, ao);
    cross3(w, u, wu);
    for (int i = 0; i < 3; i++) s[i] = W[9 + i] + ao[i] + wu[i];
    rot_t(E, s, acc);
    for (int i = 0; i < 3; i++) acc[i] += g[i];
}

}  // namespace

// one (state, contact) per thread; any of pos / vel / acc may be null (V is read for vel and acc only)
template <class T>
__global__ void contact_points_kernel(ContactSet<T> cs, const T *__restrict__ Xa, const T *__restrict__ V, int n_bodies, T gx, T gy, T gz,
                                      size_t nb, T *__restrict__ pos, T *__restrict__ vel, T *__restrict__ acc)
{
    const size_t total = nb * (size_t)cs.n;
    const T g[3] = {gx, gy, gz};
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t b = t / cs.n;
        const int c = (int)(t % cs.n);
        const size_t row = (b * n_bodies + cs.body[c]) * 12;
        const T *X = Xa + row;
        const T o[3] = {cs.off[c][0], cs.off[c][1], cs.off[c][2]};
        T E[9];
        for (int i = 0; i < 9; i++) E[i] = X[i];
        T out[3];
        if (pos) {
            rot_t(E, o, out);
            for (int i = 0; i < 3; i++) pos[3 * t + i] = X[9 + i] + out[i];
        }
        if (vel) {
            T u[3];
            point_velocity(V + row, o, u);
            rot_t(E, u, out);
            for (int i = 0; i < 3; i++) vel[3 * t + i] = out[i];
        }
        if (acc) {
            point_acceleration(E, V + row, o, g, out);
            for (int i = 0; i < 3; i++) acc[3 * t + i] = out[i];
        }
    }
}

extern __shared__ __align__(16) unsigned char contact_smem[];

template <class T>
__global__ __launch_bounds__(kWave) void contact_solve_kernel(ContactSet<T> cs, const T *__restrict__ Linv, const T *__restrict__ Xa,
                                                              const T *__restrict__ V, const T *__restrict__ a_des,
                                                              const T *__restrict__ fext_in, int n_bodies, T mu, T gx, T gy, T gz, size_t nb,
                                                              T *__restrict__ lambda, T *fext_out, unsigned long long *bad_count)
{
    const int W = (int)blockDim.x, lane = (int)threadIdx.x;
    const int n = cs.n, m = 3 * n, m6 = 6 * n, tri = m * (m + 1) / 2;
    T *A = reinterpret_cast<T *>(contact_smem) + lane;  // packed lower triangle: entry (i, j <= i) at A[(i (i + 1) / 2 + j) W]
    T *y = A + (size_t)tri * W;                         // right-hand side, then lambda: y[i W]
    const T g[3] = {gx, gy, gz};
    for (size_t b = blockIdx.x * (size_t)W + lane; b < nb; b += (size_t)gridDim.x * W) {
        const T *Lb = Linv + b * (size_t)m6 * m6;
        const T *Xb = Xa + b * (size_t)n_bodies * 12, *Vb = V + b * (size_t)n_bodies * 12;
        // A = R Linv_ff R^T + mu I, block by block of the lower triangle
        for (int c1 = 0; c1 < n; c1++) {
            T E1[9];
            {
                const T *X1 = Xb + (size_t)cs.body[c1] * 12;
                for (int i = 0; i < 9; i++) E1[i] = X1[i];
            }
            for (int c2 = 0; c2 <= c1; c2++) {
                const T *X2 = Xb + (size_t)cs.body[c2] * 12;
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
                        A[(size_t)(row + j) * W] = v;
                    }
                }
            }
        }
        // rhs = a_des - p_ddot(ydd_free)
        for (int c = 0; c < n; c++) {
            const size_t row = (size_t)cs.body[c] * 12;
            const T o[3] = {cs.off[c][0], cs.off[c][1], cs.off[c][2]};
            T acc[3];
            point_acceleration(Xb + row, Vb + row, o, g, acc);
            for (int i = 0; i < 3; i++) y[(size_t)(3 * c + i) * W] = (a_des ? a_des[(b * n + c) * 3 + i] : T(0)) - acc[i];
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
        if (bad) {
            // a pivot that is not positive or not finite: the state gets NaN, and is counted (grbda_spd_bad_pivots)
            for (int i = 0; i < m; i++) y[(size_t)i * W] = T(NAN);
            if (bad_count) atomicAdd(bad_count, 1ull);
        }
        // lambda, and the wrench row of the second forward-dynamics call
        T *w = fext_out + b * (size_t)n_bodies * 6;
        const T *fin = fext_in ? fext_in + b * (size_t)n_bodies * 6 : nullptr;
        for (int i = 0; i < n_bodies * 6; i++) w[i] = fin ? fin[i] : T(0);
        for (int c = 0; c < n; c++) {
            const T *X = Xb + (size_t)cs.body[c] * 12;
            const T o[3] = {cs.off[c][0], cs.off[c][1], cs.off[c][2]};
            T p[3], f[3], mo[3];
            rot_t(X, o, p);
            for (int i = 0; i < 3; i++) {
                p[i] += X[9 + i];
                f[i] = y[(size_t)(3 * c + i) * W];
                lambda[(b * n + c) * 3 + i] = f[i];
            }
            cross3(p, f, mo);
            T *wb = w + (size_t)cs.body[c] * 6;
            for (int i = 0; i < 3; i++) {
                wb[i] += mo[i];
                wb[3 + i] += f[i];
            }
        }
    }
}

// The velocity-level twin of contact_solve_kernel (grbda_contact_impulse_*): the same mapping, the same A and the same factorisation, with
//     rhs = v_des - (1 + e) p_dot,   p_dot = E^T (v + omega x o)
// from the velocity halves of the twist rows alone (the acceleration halves are never read; gravity does not enter).  Writes the impulses
// [nb][n][3] and the wrench row [nb][n_bodies][6] = zeros + [p x Lambda_c ; Lambda_c] on body[c], contacts on one body accumulating.
// The assembly of A and the factor / solve are a COPY of contact_solve_kernel's text: moving them into device functions both kernels call
// changed the instruction stream of the two existing instantiations (DESIGN.md 7g'), so that kernel's text stays as it was measured.
template <class T>
__global__ __launch_bounds__(kWave) void impulse_solve_kernel(ContactSet<T> cs, const T *__restrict__ Linv, const T *__restrict__ Xa,
                                                              const T *__restrict__ V, const T *__restrict__ v_des, int n_bodies, T mu,
                                                              T one_plus_e, size_t nb, T *__restrict__ impulse, T *__restrict__ wrench,
                                                              unsigned long long *bad_count)
{
    const int W = (int)blockDim.x, lane = (int)threadIdx.x;
    const int n = cs.n, m = 3 * n, m6 = 6 * n, tri = m * (m + 1) / 2;
    T *A = reinterpret_cast<T *>(contact_smem) + lane;  // packed lower triangle: entry (i, j <= i) at A[(i (i + 1) / 2 + j) W]
    T *y = A + (size_t)tri * W;                         // right-hand side, then the impulses: y[i W]
    for (size_t b = blockIdx.x * (size_t)W + lane; b < nb; b += (size_t)gridDim.x * W) {
        const T *Lb = Linv + b * (size_t)m6 * m6;
        const T *Xb = Xa + b * (size_t)n_bodies * 12, *Vb = V + b * (size_t)n_bodies * 12;
        // A = R Linv_ff R^T + mu I, block by block of the lower triangle
        for (int c1 = 0; c1 < n; c1++) {
            T E1[9];
            {
                const T *X1 = Xb + (size_t)cs.body[c1] * 12;
                for (int i = 0; i < 9; i++) E1[i] = X1[i];
            }
            for (int c2 = 0; c2 <= c1; c2++) {
                const T *X2 = Xb + (size_t)cs.body[c2] * 12;
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
                        A[(size_t)(row + j) * W] = v;
                    }
                }
            }
        }
        // rhs = v_des - (1 + e) p_dot
        for (int c = 0; c < n; c++) {
            const size_t row = (size_t)cs.body[c] * 12;
            const T o[3] = {cs.off[c][0], cs.off[c][1], cs.off[c][2]};
            T u[3], vel[3];
            point_velocity(Vb + row, o, u);
            rot_t(Xb + row, u, vel);
            for (int i = 0; i < 3; i++) y[(size_t)(3 * c + i) * W] = (v_des ? v_des[(b * n + c) * 3 + i] : T(0)) - one_plus_e * vel[i];
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
        // L z = rhs, L^T Lambda = z
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
        if (bad) {
            // a pivot that is not positive or not finite: the state gets NaN, and is counted (grbda_spd_bad_pivots)
            for (int i = 0; i < m; i++) y[(size_t)i * W] = T(NAN);
            if (bad_count) atomicAdd(bad_count, 1ull);
        }
        // the impulses, and the wrench row of the forward-dynamics call that turns them into a velocity change
        T *w = wrench + b * (size_t)n_bodies * 6;
        for (int i = 0; i < n_bodies * 6; i++) w[i] = T(0);
        for (int c = 0; c < n; c++) {
            const T *X = Xb + (size_t)cs.body[c] * 12;
            const T o[3] = {cs.off[c][0], cs.off[c][1], cs.off[c][2]};
            T p[3], f[3], mo[3];
            rot_t(X, o, p);
            for (int i = 0; i < 3; i++) {
                p[i] += X[9 + i];
                f[i] = y[(size_t)(3 * c + i) * W];
                impulse[(b * n + c) * 3 + i] = f[i];
            }
            cross3(p, f, mo);
            T *wb = w + (size_t)cs.body[c] * 6;
            for (int i = 0; i < 3; i++) {
                wb[i] += mo[i];
                wb[3 + i] += f[i];
            }
        }
    }
}

// qd_next = qd + (y1 - y0), element by element: y1, y0 the forward dynamics at rest with and without the impulses' wrenches.  qd_next may
// be qd (an element is read before it is written, by the same thread).
template <class T>
__global__ void impulse_finish_kernel(const T *qd, const T *__restrict__ y1, const T *__restrict__ y0, size_t total, T *qd_next)
{
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        qd_next[t] = qd[t] + (y1[t] - y0[t]);
}

size_t contact_solve_lds_bytes(int n_contacts, size_t elem, int lanes)
{
    const size_t m = 3 * static_cast<size_t>(n_contacts);
    return (m * (m + 1) / 2 + m) * static_cast<size_t>(lanes) * elem;
}
// states per workgroup: of 64, 32 and 16 the one that keeps the most states resident on a CU (lanes x workgroups whose LDS fits, at most
// 32 wavefronts), the wider one on a tie
int contact_solve_lanes(int n_contacts, size_t elem)
{
    int best = 16;
    size_t best_states = 0;
    for (const int lanes : {64, 32, 16}) {
        const size_t bytes = contact_solve_lds_bytes(n_contacts, elem, lanes);
        const size_t wg = bytes <= 160u * 1024u ? std::min<size_t>(32, lds_workgroups_per_cu(bytes)) : 0;
        if (wg * lanes > best_states) {
            best_states = wg * lanes;
            best = lanes;
        }
    }
    return best;
}

template <class T>
hipError_t launch_contact_points(const ContactSet<T> &cs, const T *Xa, const T *V, int n_bodies, const T g[3], size_t nb, T *pos, T *vel, T *acc,
                                 hipStream_t stream)
{
    const size_t total = nb * static_cast<size_t>(cs.n);
    const int blocks = static_cast<int>((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL((contact_points_kernel<T>), dim3(blocks), dim3(256), 0, stream, cs, Xa, V, n_bodies, g[0], g[1], g[2], nb, pos, vel, acc);
    return hipGetLastError();
}
// what one launch of the solve is made of: the width, its dynamic LDS and the workgroups a CU holds (the grid cap is n_cu times that);
// lanes == 0 when no width fits the 160 KiB.  launch_contact_solve and grbda_contact_solve_launch both read it from here.
ContactSolveLaunch contact_solve_launch(int n_contacts, size_t elem)
{
    ContactSolveLaunch L;
    L.lanes = contact_solve_lanes(n_contacts, elem);
    L.lds_bytes = contact_solve_lds_bytes(n_contacts, elem, L.lanes);
    if (L.lds_bytes > 160u * 1024u) L.lanes = 0;
    L.per_cu = std::max<size_t>(1, std::min<size_t>(32, lds_workgroups_per_cu(L.lds_bytes)));
    return L;
}
template <class T>
hipError_t launch_contact_solve(const ContactSet<T> &cs, const T *Linv, const T *Xa, const T *V, const T *a_des, const T *fext_in, int n_bodies,
                                T mu, const T g[3], size_t nb, T *lambda, T *fext_out, unsigned long long *bad_count, int n_cu,
                                hipStream_t stream)
{
    const ContactSolveLaunch L = contact_solve_launch(cs.n, sizeof(T));
    if (L.lanes == 0) return hipErrorInvalidValue;
    const size_t grid = std::min(static_cast<size_t>(n_cu) * L.per_cu, (nb + L.lanes - 1) / L.lanes);
    hipLaunchKernelGGL((contact_solve_kernel<T>), dim3(static_cast<unsigned>(grid)), dim3(L.lanes), L.lds_bytes, stream, cs, Linv, Xa, V, a_des,
                       fext_in, n_bodies, mu, g[0], g[1], g[2], nb, lambda, fext_out, bad_count);
    return hipGetLastError();
}
// the impulse solve launches from the same record: the same triangle and one right-hand side in LDS
template <class T>
hipError_t launch_impulse_solve(const ContactSet<T> &cs, const T *Linv, const T *Xa, const T *V, const T *v_des, int n_bodies, T mu, T restitution,
                                size_t nb, T *impulse, T *wrench, unsigned long long *bad_count, int n_cu, hipStream_t stream)
{
    const ContactSolveLaunch L = contact_solve_launch(cs.n, sizeof(T));
    if (L.lanes == 0) return hipErrorInvalidValue;
    const size_t grid = std::min(static_cast<size_t>(n_cu) * L.per_cu, (nb + L.lanes - 1) / L.lanes);
    hipLaunchKernelGGL((impulse_solve_kernel<T>), dim3(static_cast<unsigned>(grid)), dim3(L.lanes), L.lds_bytes, stream, cs, Linv, Xa, V, v_des,
                       n_bodies, mu, T(1) + restitution, nb, impulse, wrench, bad_count);
    return hipGetLastError();
}
template <class T>
hipError_t launch_impulse_finish(const T *qd, const T *y1, const T *y0, size_t total, T *qd_next, hipStream_t stream)
{
    const int blocks = static_cast<int>((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL((impulse_finish_kernel<T>), dim3(blocks), dim3(256), 0, stream, qd, y1, y0, total, qd_next);
    return hipGetLastError();
}
template hipError_t launch_impulse_solve<float>(const ContactSet<float> &, const float *, const float *, const float *, const float *, int, float,
                                                float, size_t, float *, float *, unsigned long long *, int, hipStream_t);
template hipError_t launch_impulse_solve<double>(const ContactSet<double> &, const double *, const double *, const double *, const double *, int,
                                                 double, double, size_t, double *, double *, unsigned long long *, int, hipStream_t);
template hipError_t launch_impulse_finish<float>(const float *, const float *, const float *, size_t, float *, hipStream_t);
template hipError_t launch_impulse_finish<double>(const double *, const double *, const double *, size_t, double *, hipStream_t);
template hipError_t launch_contact_points<float>(const ContactSet<float> &, const float *, const float *, int, const float[3], size_t, float *,
                                                 float *, float *, hipStream_t);
template hipError_t launch_contact_points<double>(const ContactSet<double> &, const double *, const double *, int, const double[3], size_t,
                                                  double *, double *, double *, hipStream_t);
template hipError_t launch_contact_solve<float>(const ContactSet<float> &, const float *, const float *, const float *, const float *,
                                                const float *, int, float, const float[3], size_t, float *, float *, unsigned long long *, int,
                                                hipStream_t);
template hipError_t launch_contact_solve<double>(const ContactSet<double> &, const double *, const double *, const double *, const double *,
                                                 const double *, int, double, const double[3], size_t, double *, double *, unsigned long long *,
                                                 int, hipStream_t);

// the solves ask for more dynamic LDS than the 64 KiB default (per device, as for the other kernel families)
hipError_t set_max_dynamic_lds_contact()
{
    for (const void *f : {reinterpret_cast<const void *>(&contact_solve_kernel<float>), reinterpret_cast<const void *>(&contact_solve_kernel<double>),
                          reinterpret_cast<const void *>(&impulse_solve_kernel<float>), reinterpret_cast<const void *>(&impulse_solve_kernel<double>)}) {
        hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace grbda_hip
