// centroidal_kernels.hip -- kinetic and potential energy, centre of mass and its velocity, centroidal momentum and its rate behind
// grbda_energy_*, grbda_centroidal_* and grbda_centroidal_matrix_* (include/grbda_hip.h "energy and centroidal quantities"; capi.cpp,
// centroidal_stage).  Pinocchio: computeKineticEnergy, computePotentialEnergy, centerOfMass, computeCentroidalMomentumTimeVariation, ccrba.
//
// One STATE per lane, one wavefront per workgroup, a grid-stride walk over tiles of 64 states, like poses_kernel / twists_kernel
// (kernels.hip).  The kernel walks clusters and bodies in plan order and builds every body's joint transform the way those two do
// (build_E, free_rotation, the spanning position itself for implicit clusters, the true joint angle for rotors), composes the world pose
// (E, r), the velocity v and -- when a rate is asked for -- the acceleration a that starts from a_root = -gravity, and sums per body, with
// I the body's 21 packed inertia constants, m and h = m c read from them and l = I v = [n; p]:
//     KE   += 1/2 v . l
//     mc_w += m r + E^T h
//     P    += E^T p                          h_O += E^T n + r x (E^T p)
//     f     = I a + v x* l
//     F    += E^T f_lin                      N_O += E^T f_ang + r x (E^T f_lin)
// and finishes with the total mass M and the gravity g of the launch:
//     c = mc_w / M      c_dot = P / M        h_G = h_O - c x P
//     PE = -g . mc_w    P_dot = F + M g      h_G_dot = N_O + mc_w x g - c x P_dot
// The sums are world-frame vectors: they do not depend on the frame a body's quantities are expressed in, so the plan's canonical-axis
// body frames (BodyRec::canon_axis) need no conversion back here -- unlike the tail loops of poses_kernel / twists_kernel, whose outputs
// ARE the per-body quantities.
//
// Parents are not read back from a row-major output row (there is none).  The pose (12), v (6) and a (6) of every body that has a child
// live in a lane-contiguous region [value][64] of the wavefront's share of the per-(device, stream) scratch slab -- the layout of the
// interpreter's global slots, every access one coalesced 256 / 512-byte row -- at the row CentroidalRows gives the body; leaves are
// consumed in registers and never stored.  LDS is not the home of this store: about 20 parent bodies x 24 values x 64 lanes x 4 B is
// 120 KiB, one wavefront per CU.  No per-lane array is indexed at run time.
//
// LEVEL selects what is computed: 0 positions only (qd is never touched), 1 positions and velocities, 2 accelerations as well.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

#include "devmath.h"

namespace {

// out = E^T x  (E: world -> body, row-major)
template <class T>
__device__ __forceinline__ void to_world(const T (&E)[9], T x0, T x1, T x2, T (&out)[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = E[i] * x0 + E[3 + i] * x1 + E[6 + i] * x2;
}
// acc += a x b
template <class T>
__device__ __forceinline__ void add_cross(const T (&a)[3], const T (&b)[3], T (&acc)[3])
{
    acc[0] += a[1] * b[2] - a[2] * b[1];
    acc[1] += a[2] * b[0] - a[0] * b[2];
    acc[2] += a[0] * b[1] - a[1] * b[0];
}

}  // namespace

template <class T, int LEVEL>
__global__ __launch_bounds__(kWave, 1) void centroidal_kernel(DevPlan<T> DP, int n_clusters, int n_span, const int32_t *__restrict__ rows_,
                                                              int n_rows, const T *__restrict__ q, const T *__restrict__ qd_span,
                                                              const T *__restrict__ qdd_span, T gx, T gy, T gz, T mass, CentroidalOut<T> O,
                                                              size_t B, T *__restrict__ scratch)
{
    cptr<ClusterRec> clusters = (cptr<ClusterRec>)DP.clusters;
    cptr<BodyRec> bodies = (cptr<BodyRec>)DP.bodies;
    cptr<T> consts = (cptr<T>)DP.consts;
    cptr<int32_t> rows = (cptr<int32_t>)rows_;
    const int lane = threadIdx.x, nq = DP.nq;
    T *slab = scratch + (size_t)blockIdx.x * (size_t)n_rows * kWave + lane;  // row k of this lane: slab[k * kWave]
    const size_t n_tiles = (B + kWave - 1) / kWave;
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t r = tile * kWave + lane;
        if (r >= B) continue;  // (no cross-lane operation below)
        const T *qr = q + r * (size_t)nq;
        const T *vs = LEVEL >= 1 ? qd_span + r * (size_t)n_span : nullptr;
        const T *as = LEVEL >= 2 ? qdd_span + r * (size_t)n_span : nullptr;
        T ke = 0, mc[3] = {0, 0, 0}, Pw[3] = {0, 0, 0}, hO[3] = {0, 0, 0}, Fw[3] = {0, 0, 0}, NO[3] = {0, 0, 0};
        int at = 0;
        for (int ci = 0; ci < n_clusters; ci++) {
            const ClusterRec c = load_rec(clusters + ci);
            for (int i = 0; i < c.k; i++) {
                const int gb = c.first_body + i;
                const BodyRec b = load_rec(bodies + gb);
                cptr<T> C = consts + b.cofs;
                const int own = rows[2 * gb], par = rows[2 * gb + 1];
                T E[9], rr[3], v[6], a[6];
                if (c.kind == CK_FREE) {  // S = 1: the rates are the base twist; a = X (-gravity) + ydd
                    T o[4];
                    const int nori = DP.ori_repr == 0 ? 4 : 3;
#pragma unroll
                    for (int j = 0; j < 4; j++) o[j] = j < nori ? qr[c.q_index + 3 + j] : T(0);
                    free_rotation(DP.ori_repr, o, E);
#pragma unroll
                    for (int j = 0; j < 3; j++) rr[j] = qr[c.q_index + j];
                    if constexpr (LEVEL >= 1) {
#pragma unroll
                        for (int j = 0; j < 6; j++) v[j] = vs[at + j];
                    }
                    if constexpr (LEVEL >= 2) {
#pragma unroll
                        for (int j = 0; j < 6; j++) a[j] = as[at + j];
#pragma unroll
                        for (int u = 0; u < 3; u++) {
                            a[u] += E[3 * u] * DP.a_root[0] + E[3 * u + 1] * DP.a_root[1] + E[3 * u + 2] * DP.a_root[2];
                            a[3 + u] += E[3 * u] * DP.a_root[3] + E[3 * u + 1] * DP.a_root[4] + E[3 * u + 2] * DP.a_root[5];
                        }
                    }
                } else {
                    T qi = 0;
                    if (c.kind == CK_LOOP) {
                        qi = qr[c.q_index + i];
                    } else {
                        for (int k2 = 0; k2 < c.n; k2++) qi += C[kBodyConstFixed + k2] * qr[c.q_index + k2];
                    }
                    T sn, cs, El[9], vp[6], ap[6];
                    sincos_t(qi, &sn, &cs);
                    build_E(b.axis, sn, cs, C, El);
                    if (par >= 0) {  // Xa = X Xa_parent: E = E_l E_p, r = r_p + E_p^T r_l
                        const T *Xp = slab + (size_t)par * kWave;
                        T Ep[9], rp[3];
#pragma unroll
                        for (int u = 0; u < 9; u++) Ep[u] = Xp[u * kWave];
#pragma unroll
                        for (int u = 0; u < 3; u++) rp[u] = Xp[(9 + u) * kWave];
#pragma unroll
                        for (int u = 0; u < 3; u++)
#pragma unroll
                            for (int w = 0; w < 3; w++) E[3 * u + w] = El[3 * u] * Ep[w] + El[3 * u + 1] * Ep[3 + w] + El[3 * u + 2] * Ep[6 + w];
#pragma unroll
                        for (int u = 0; u < 3; u++) rr[u] = rp[u] + Ep[u] * C[9] + Ep[3 + u] * C[10] + Ep[6 + u] * C[11];
                        if constexpr (LEVEL >= 1) {
#pragma unroll
                            for (int j = 0; j < 6; j++) vp[j] = Xp[(12 + j) * kWave];
                        }
                        if constexpr (LEVEL >= 2) {
#pragma unroll
                            for (int j = 0; j < 6; j++) ap[j] = Xp[(18 + j) * kWave];
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < 9; u++) E[u] = El[u];
#pragma unroll
                        for (int u = 0; u < 3; u++) rr[u] = C[9 + u];
#pragma unroll
                        for (int j = 0; j < 6; j++) {
                            vp[j] = 0;
                            ap[j] = DP.a_root[j];
                        }
                    }
                    if constexpr (LEVEL >= 1) {
                        const T qdi = vs[at + i];
                        xmotion(El, C + 9, vp, v);
                        add_axis(v, b.axis, qdi);
                        if constexpr (LEVEL >= 2) {
                            T cx[6];
                            xmotion(El, C + 9, ap, a);
                            vxaxis(b.axis, v, qdi, cx);  // v x (S qd)
#pragma unroll
                            for (int j = 0; j < 6; j++) a[j] += cx[j];
                            add_axis(a, b.axis, as[at + i]);
                        }
                    }
                }
                if (own >= 0) {  // a body with children: what they read
                    T *Xo = slab + (size_t)own * kWave;
#pragma unroll
                    for (int u = 0; u < 9; u++) Xo[u * kWave] = E[u];
#pragma unroll
                    for (int u = 0; u < 3; u++) Xo[(9 + u) * kWave] = rr[u];
                    if constexpr (LEVEL >= 1) {
#pragma unroll
                        for (int j = 0; j < 6; j++) Xo[(12 + j) * kWave] = v[j];
                    }
                    if constexpr (LEVEL >= 2) {
#pragma unroll
                        for (int j = 0; j < 6; j++) Xo[(18 + j) * kWave] = a[j];
                    }
                }
                // ---- the body's terms ----
                cptr<T> I = C + 12;
                const T m = I[sidx(3, 3)];
                T w3[3];
                to_world(E, -I[sidx(1, 5)], I[sidx(0, 5)], -I[sidx(0, 4)], w3);  // h = m c from the upper right block m c x
#pragma unroll
                for (int u = 0; u < 3; u++) mc[u] += m * rr[u] + w3[u];
                if constexpr (LEVEL >= 1) {
                    T l[6], pw[3];
                    symv_c(I, v, l);
                    T dot = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++) dot += v[j] * l[j];
                    ke += T(0.5) * dot;
                    to_world(E, l[3], l[4], l[5], pw);
                    to_world(E, l[0], l[1], l[2], w3);
#pragma unroll
                    for (int u = 0; u < 3; u++) {
                        Pw[u] += pw[u];
                        hO[u] += w3[u];
                    }
                    add_cross(rr, pw, hO);
                    if constexpr (LEVEL >= 2) {
                        T f[6], fx[6], fw[3];
                        symv_c(I, a, f);
                        crf(v, l, fx);
#pragma unroll
                        for (int j = 0; j < 6; j++) f[j] += fx[j];
                        to_world(E, f[3], f[4], f[5], fw);
                        to_world(E, f[0], f[1], f[2], w3);
#pragma unroll
                        for (int u = 0; u < 3; u++) {
                            Fw[u] += fw[u];
                            NO[u] += w3[u];
                        }
                        add_cross(rr, fw, NO);
                    }
                }
            }
            at += c.kind == CK_FREE ? 6 : c.k;
        }
        // ---- finish ----
        const T g[3] = {gx, gy, gz};
        const T cm[3] = {mc[0] / mass, mc[1] / mass, mc[2] / mass};
        if (O.potential) O.potential[r] = -(g[0] * mc[0] + g[1] * mc[1] + g[2] * mc[2]);
        if (O.com) {
#pragma unroll
            for (int u = 0; u < 3; u++) O.com[3 * r + u] = cm[u];
        }
        if constexpr (LEVEL >= 1) {
            if (O.kinetic) O.kinetic[r] = ke;
            if (O.com_vel) {
#pragma unroll
                for (int u = 0; u < 3; u++) O.com_vel[3 * r + u] = Pw[u] / mass;
            }
            if (O.h) {
                T hG[3] = {hO[0], hO[1], hO[2]};
                const T mP[3] = {-Pw[0], -Pw[1], -Pw[2]};
                add_cross(cm, mP, hG);  // h_O - c x P
                // rows of h: [r][6], or -- the momentum matrix, h_cols = nv rows of the expanded batch per state -- A[state][6][nv]
                const size_t st = O.h_cols ? r / (size_t)O.h_cols : r, col = O.h_cols ? r % (size_t)O.h_cols : 0;
                const size_t step = O.h_cols ? (size_t)O.h_cols : 1;
                T *ho = O.h + st * 6 * step + col;
#pragma unroll
                for (int u = 0; u < 3; u++) {
                    ho[(size_t)u * step] = hG[u];
                    ho[(size_t)(3 + u) * step] = Pw[u];
                }
            }
        }
        if constexpr (LEVEL >= 2) {
            if (O.hdot) {
                const T Pd[3] = {Fw[0] + mass * g[0], Fw[1] + mass * g[1], Fw[2] + mass * g[2]};
                const T mPd[3] = {-Pd[0], -Pd[1], -Pd[2]};
                T hd[3] = {NO[0], NO[1], NO[2]};
                add_cross(mc, g, hd);    // + mc_w x g
                add_cross(cm, mPd, hd);  // - c x P_dot
#pragma unroll
                for (int u = 0; u < 3; u++) {
                    O.hdot[6 * r + u] = hd[u];
                    O.hdot[6 * r + 3 + u] = Pd[u];
                }
            }
        }
    }
}

// The launch-decision record of the stage: the kernel variant, the grid and the scratch rows of one launch.  launch_centroidal (the one
// launch site) and capi.cpp's centroidal_stage (which sizes the scratch slab) both read it from here.
CentroidalLaunch centroidal_launch(bool velocities, bool rates, int n_parent_bodies, int n_cu, size_t nb)
{
    CentroidalLaunch L;
    L.level = rates ? 2 : velocities ? 1 : 0;
    // eight one-wavefront workgroups per CU, as poses_kernel / twists_kernel (registers hold two per SIMD in either precision), one per tile at most
    L.grid = std::min(static_cast<size_t>(n_cu) * 8, (nb + kWave - 1) / kWave);
    L.slab_rows = static_cast<size_t>(n_parent_bodies) * kCentroidalBodyRows;
    return L;
}

template <class T>
hipError_t launch_centroidal(const DevPlan<T> &P, int n_clusters, int n_span, const int32_t *rows, const CentroidalLaunch &L, const T *q,
                             const T *qd_span, const T *qdd_span, const T g[3], T mass, const CentroidalOut<T> &out, size_t nb, T *scratch,
                             hipStream_t stream)
{
    const dim3 grid(static_cast<unsigned>(L.grid)), block(kWave);
    const int n_rows = static_cast<int>(L.slab_rows);
    if (L.level == 2)
        hipLaunchKernelGGL((centroidal_kernel<T, 2>), grid, block, 0, stream, P, n_clusters, n_span, rows, n_rows, q, qd_span, qdd_span, g[0], g[1],
                           g[2], mass, out, nb, scratch);
    else if (L.level == 1)
        hipLaunchKernelGGL((centroidal_kernel<T, 1>), grid, block, 0, stream, P, n_clusters, n_span, rows, n_rows, q, qd_span, qdd_span, g[0], g[1],
                           g[2], mass, out, nb, scratch);
    else
        hipLaunchKernelGGL((centroidal_kernel<T, 0>), grid, block, 0, stream, P, n_clusters, n_span, rows, n_rows, q, qd_span, qdd_span, g[0], g[1],
                           g[2], mass, out, nb, scratch);
    return hipGetLastError();
}
template hipError_t launch_centroidal<float>(const DevPlan<float> &, int, int, const int32_t *, const CentroidalLaunch &, const float *, const float *,
                                             const float *, const float[3], float, const CentroidalOut<float> &, size_t, float *, hipStream_t);
template hipError_t launch_centroidal<double>(const DevPlan<double> &, int, int, const int32_t *, const CentroidalLaunch &, const double *,
                                              const double *, const double *, const double[3], double, const CentroidalOut<double> &, size_t,
                                              double *, hipStream_t);

}  // namespace grbda_hip
