// vjp_kernels.hip -- the contraction of the vector-Jacobian products (include/grbda_hip_vjp.h): rows of two [nv][nv] matrices per state
// weighted by one [nv] vector,
//     out_q[b][j] = sign * sum_i w[b][i] Mq[b][i][j],   out_qd[b][j] = sign * sum_i w[b][i] Mqd[b][i][j],   w = w_add - w_sub.
// A pure stream of 2 nv^2 scalars per state against 2 nv written: everything here is for bandwidth.
//
// Lanes are COLUMNS j, so every row load of a wavefront is a run of consecutive addresses.  A unit of work is
//     nv <= 32        floor(64 / nv) consecutive states, lane = s * nv + j (their matrices are one contiguous block; lanes past the last
//                     state of the pack idle)
//     32 < nv <= 64   one state, lane = j
//     nv > 64         one block of 64 columns of one state, lane = j - 64 * block
// and one-wavefront workgroups walk the units in a grid-stride loop (vjp_contract_launch: the one launch rule).  The weights of a unit go to
// LDS once (the difference w_add - w_sub is formed there, and written to out_w by the unit of column block 0 when that is asked for); the
// row loop reads them back as broadcasts.  Rows are summed in ascending i, four at a time in flight per matrix: the order is fixed, so a
// replayed graph gives the eager call's bits.  Lanes past the last state or the last column neither load nor store.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

namespace {

template <class T>
__global__ void __launch_bounds__(kWave) vjp_contract_kernel(const T *__restrict__ Mq, const T *__restrict__ Mqd, const T *__restrict__ w_add,
                                                             const T *__restrict__ w_sub, T sign, int nv, size_t nb, size_t n_units,
                                                             T *__restrict__ out_q, T *__restrict__ out_qd, T *__restrict__ out_w)
{
    extern __shared__ __align__(16) unsigned char vjp_lds_raw[];
    T *wl = reinterpret_cast<T *>(vjp_lds_raw);  // [pack][nv]
    const int lane = static_cast<int>(threadIdx.x);
    const int pack = nv <= kWave / 2 ? kWave / nv : 1;  // states per unit
    const int n_blk = (nv + kWave - 1) / kWave;         // column blocks per state
    const int s = pack > 1 ? lane / nv : 0;             // this lane's state of the pack ...
    const int jl = pack > 1 ? lane - s * nv : lane;     // ... and its column of the block
    const size_t nn = static_cast<size_t>(nv) * static_cast<size_t>(nv);
    for (size_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const size_t sg = u / static_cast<size_t>(n_blk);
        const int blk = static_cast<int>(u - sg * static_cast<size_t>(n_blk));
        const size_t b0 = sg * static_cast<size_t>(pack);
        const int live_states = static_cast<int>(nb - b0 < static_cast<size_t>(pack) ? nb - b0 : static_cast<size_t>(pack));
        // the weights of the unit's states: contiguous in w, live_states * nv of them
        const size_t w0 = b0 * static_cast<size_t>(nv);
        const int n_w = live_states * nv;
        for (int k = lane; k < n_w; k += kWave) {
            T v = w_add[w0 + k];
            if (w_sub) v -= w_sub[w0 + k];
            wl[k] = v;
            if (out_w && blk == 0) out_w[w0 + k] = v;
        }
        __syncthreads();
        const int j = blk * kWave + jl;
        if (s < live_states && j < nv && (Mq || Mqd)) {
            const size_t m0 = (b0 + static_cast<size_t>(s)) * nn + static_cast<size_t>(j);
            const T *wr = wl + s * nv;
            const T *mq = Mq ? Mq + m0 : nullptr, *mqd = Mqd ? Mqd + m0 : nullptr;
            T aq = T(0), aqd = T(0);
            int i = 0;
            for (; i + 4 <= nv; i += 4) {
                const size_t r = static_cast<size_t>(i) * static_cast<size_t>(nv);
                T q0 = T(0), q1 = T(0), q2 = T(0), q3 = T(0), d0 = T(0), d1 = T(0), d2 = T(0), d3 = T(0);
                if (mq) {
                    q0 = mq[r];
                    q1 = mq[r + nv];
                    q2 = mq[r + 2 * static_cast<size_t>(nv)];
                    q3 = mq[r + 3 * static_cast<size_t>(nv)];
                }
                if (mqd) {
                    d0 = mqd[r];
                    d1 = mqd[r + nv];
                    d2 = mqd[r + 2 * static_cast<size_t>(nv)];
                    d3 = mqd[r + 3 * static_cast<size_t>(nv)];
                }
                const T w0r = wr[i], w1r = wr[i + 1], w2r = wr[i + 2], w3r = wr[i + 3];
                aq += w0r * q0;
                aq += w1r * q1;
                aq += w2r * q2;
                aq += w3r * q3;
                aqd += w0r * d0;
                aqd += w1r * d1;
                aqd += w2r * d2;
                aqd += w3r * d3;
            }
            for (; i < nv; i++) {
                const size_t r = static_cast<size_t>(i) * static_cast<size_t>(nv);
                const T wi = wr[i];
                if (mq) aq += wi * mq[r];
                if (mqd) aqd += wi * mqd[r];
            }
            const size_t o = (b0 + static_cast<size_t>(s)) * static_cast<size_t>(nv) + static_cast<size_t>(j);
            if (out_q) out_q[o] = sign * aq;
            if (out_qd) out_qd[o] = sign * aqd;
        }
        __syncthreads();  // (the next unit overwrites the weights)
    }
}

}  // namespace

// The launch rule of the contraction: units of work over nb states, a persistent grid of kVjpWavesPerCu one-wavefront workgroups per CU (a
// memory-bound stream: four wavefronts per SIMD, eight row loads in flight each) and at most one per unit, LDS for the weights of one unit.
VjpLaunch vjp_contract_launch(int nv, size_t elem, int n_cu, size_t nb)
{
    VjpLaunch L;
    const size_t pack = nv <= kWave / 2 ? static_cast<size_t>(kWave / nv) : 1;
    const size_t n_blk = (static_cast<size_t>(nv) + kWave - 1) / kWave;
    L.units = (nb + pack - 1) / pack * n_blk;
    L.grid = std::min(static_cast<size_t>(n_cu) * kVjpWavesPerCu, L.units);
    L.lds_bytes = (pack * static_cast<size_t>(nv) * elem + 15) / 16 * 16;
    return L;
}

template <class T>
hipError_t launch_vjp_contract(const VjpLaunch &L, const T *Mq, const T *Mqd, const T *w_add, const T *w_sub, T sign, int nv, size_t nb, T *out_q,
                               T *out_qd, T *out_w, hipStream_t stream)
{
    if (nb == 0 || L.grid == 0) return hipSuccess;
    hipLaunchKernelGGL((vjp_contract_kernel<T>), dim3(static_cast<unsigned>(L.grid)), dim3(kWave), L.lds_bytes, stream, Mq, Mqd, w_add, w_sub, sign, nv, nb,
                       L.units, out_q, out_qd, out_w);
    return hipGetLastError();
}
template hipError_t launch_vjp_contract<float>(const VjpLaunch &, const float *, const float *, const float *, const float *, float, int, size_t,
                                               float *, float *, float *, hipStream_t);
template hipError_t launch_vjp_contract<double>(const VjpLaunch &, const double *, const double *, const double *, const double *, double, int,
                                                size_t, double *, double *, double *, hipStream_t);

}  // namespace grbda_hip
