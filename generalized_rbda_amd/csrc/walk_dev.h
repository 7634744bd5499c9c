// walk_dev.h -- the device side of an ancestor walk (walk.h), shared by the walk kernels (body_list_kernels.hip, frame_jacobian_kernels.hip, frame_product_kernels.hip):
// the saved values' LDS slots, the joint angle of a step and the pose step.  A step record is wave-uniform -- it sits in the kernel
// arguments and is read through the scalar unit -- so every branch on it is a scalar branch, and nothing here indexes a per-lane array at
// run time.  Included inside namespace grbda_hip, after devmath.h.
#pragma once

// LDS slot of 12 values, [slot][value][lane]: a lane reads what it wrote, lane == bank, no barrier
template <class T>
__device__ __forceinline__ void slot_put(int slot, int lane, const T (&x)[12])
{
    T *p = reinterpret_cast<T *>(grbda_smem) + slot * 12 * kWave + lane;
#pragma unroll
    for (int k = 0; k < 12; k++) p[k * kWave] = x[k];
}
template <class T>
__device__ __forceinline__ void slot_get(int slot, int lane, T (&x)[12])
{
    const T *p = reinterpret_cast<const T *>(grbda_smem) + slot * 12 * kWave + lane;
#pragma unroll
    for (int k = 0; k < 12; k++) x[k] = p[k * kWave];
}
// six values in the LDS rows [row, row + 6) of kWave lanes each (a slot of 12 is rows [12 slot, 12 slot + 12)): what the product walk
// (frame_product_kernels.hip) keeps next to the saved poses -- a branch point's running twist, a frame's world wrench
template <class T>
__device__ __forceinline__ void rows6_put(int row, int lane, const T (&x)[6])
{
    T *p = reinterpret_cast<T *>(grbda_smem) + row * kWave + lane;
#pragma unroll
    for (int k = 0; k < 6; k++) p[k * kWave] = x[k];
}
template <class T>
__device__ __forceinline__ void rows6_get(int row, int lane, T (&x)[6])
{
    const T *p = reinterpret_cast<const T *>(grbda_smem) + row * kWave + lane;
#pragma unroll
    for (int k = 0; k < 6; k++) x[k] = p[k * kWave];
}
// the spanning joint angle of the step's body: its G row times the cluster's n positions; n == 0: q[q_col] itself (BodyWalkStep::n)
template <class T, class Step>
__device__ __forceinline__ T joint_angle(const Step &st, cptr<T> C, const T *qr)
{
    if (st.n == 0) return qr[st.q_col];
    T qi = 0;
    for (int a = 0; a < st.n; a++) qi += C[kBodyConstFixed + a] * qr[st.q_col + a];
    return qi;
}
// One pose step of a walk (Step: BodyWalkStep or JacWalkStep).  X = [E 9 | r 3] of the step's body (TreeNode::Xa_) from the running value
// -- its parent's, restored from the step's slot where the walk branches -- and saved where later children start from it.  The formulas
// are those of poses_kernel (kernels.hip), term by term, in the plan's canonical body frames.
template <class T, class Step>
__device__ __forceinline__ void walk_pose_step(const Step &st, cptr<T> consts, int ori_repr, const T *qr, int lane, T (&X)[12])
{
    if (st.restore != kWalkNone) slot_get(st.restore, lane, X);
    T E[9], rr[3];
    if (st.free) {
        T o[4];
        const int nori = ori_repr == 0 ? 4 : 3;
        for (int j = 0; j < 4; j++) o[j] = j < nori ? qr[st.q_col + 3 + j] : T(0);
        free_rotation(ori_repr, o, E);
        for (int j = 0; j < 3; j++) rr[j] = qr[st.q_col + j];
    } else {
        cptr<T> C = consts + st.cofs;
        const T qi = joint_angle(st, C, qr);
        T sn, cs, El[9];
        sincos_t(qi, &sn, &cs);
        build_E((int)st.axis, sn, cs, C, El);
        if (!st.root) {  // Xa = X * Xa_parent: E = E_l E_p, r = r_p + E_p^T r_l
#pragma unroll
            for (int u = 0; u < 3; u++)
#pragma unroll
                for (int w = 0; w < 3; w++) E[3 * u + w] = El[3 * u] * X[w] + El[3 * u + 1] * X[3 + w] + El[3 * u + 2] * X[6 + w];
#pragma unroll
            for (int u = 0; u < 3; u++) rr[u] = X[9 + u] + X[u] * C[9] + X[3 + u] * C[10] + X[6 + u] * C[11];
        } else {
#pragma unroll
            for (int u = 0; u < 9; u++) E[u] = El[u];
#pragma unroll
            for (int u = 0; u < 3; u++) rr[u] = C[9 + u];
        }
    }
#pragma unroll
    for (int u = 0; u < 9; u++) X[u] = E[u];
#pragma unroll
    for (int u = 0; u < 3; u++) X[9 + u] = rr[u];
    if (st.save != kWalkNone) slot_put(st.save, lane, X);
}
