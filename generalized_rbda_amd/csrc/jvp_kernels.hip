// jvp_kernels.hip -- the contraction of the Jacobian-vector products (include/grbda_hip_jvp.h): two row-major [nv][nv] matrices per state
// summed ALONG their rows against one [nv] vector each,
//     out[b][i] = w_add[b][i] (or 0) + sign * ( sum_j Mq[b][i][j] uq[b][j] + sum_j Mqd[b][i][j] uqd[b][j] ).
// A pure stream of 2 nv^2 scalars per state against nv written, the budget of vjp_kernels.hip; the access problem is the other way round:
// the result of a lane is a sum over what a row load spreads across the lanes.
//
// Shape: a block of rows goes from global memory to LDS in loads that are runs of consecutive addresses, and is read back with
// lane = ROW along a padded row pitch.  One pass, no shuffle chain per row (lanes as columns would pay six cross-lane steps for every row
// of every matrix), and no lane ever strides through global memory by nv.  A unit of work follows the unit rule of the VJP kernel:
//     nv <= 32        floor(64 / nv) consecutive states, lane = s * nv + i: their matrices are one contiguous block of <= 64 rows
//     32 < nv <= 64   one state, lane = i
//     nv > 64         one block of 64 rows of one state, lane = i - 64 * block; the block sums over ALL columns, 64 at a time
// A tile is <= 64 rows by kt = min(nv, 64) columns.  Up to nv = 64 the tile is the unit's whole block of the matrix and the load index
// f = 64 k + lane runs through it contiguously (row f / kt, column f % kt: f itself is the offset); beyond, one load is one row's run of
// 64 columns (the last tile of a row: the columns that are left, the lanes past them idle).  The LDS image has pitch kt | 1 scalars: odd, so
// the 32 lanes of a half-wavefront that read one column of 32 rows hit 32 different banks (ds_read_b32), or 32 different bank pairs
// (ds_read_b64).  Eight loads are in flight per lane before the first LDS write.  The vectors uq, uqd of the unit sit in LDS too (read back
// as broadcasts within a state).  Sums run over Mq's columns in ascending j, then Mqd's, in one accumulator each: the order does not depend
// on the grid or on B, there are no atomics, and a replayed graph gives the eager call's bits.  Lanes past the last state, row or column
// neither load nor store.  One-wavefront workgroups walk the units in a grid-stride loop (jvp_contract_launch: the one launch rule).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devplan.h"

namespace grbda_hip {

namespace {

constexpr int kJvpLoads = 8;  // global loads in flight per lane

// the shape of a unit, one definition for the kernel and the launch rule
__host__ __device__ inline int jvp_pack(int nv) { return nv <= kWave / 2 ? kWave / nv : 1; }            // states per unit
__host__ __device__ inline int jvp_tile_cols(int nv) { return nv < kWave ? nv : kWave; }                 // kt
__host__ __device__ inline int jvp_pitch(int nv) { return jvp_tile_cols(nv) | 1; }                       // scalars per LDS row
__host__ __device__ inline int jvp_vec_len(int nv) { return nv <= kWave / 2 ? jvp_pack(nv) * nv : nv; }  // scalars of one staged vector

template <class T>
__global__ void __launch_bounds__(kWave) jvp_contract_kernel(const T *__restrict__ Mq, const T *__restrict__ Mqd, const T *__restrict__ uq,
                                                             const T *__restrict__ uqd, const T *__restrict__ w_add, T sign, int nv, size_t nb,
                                                             size_t n_units, T *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char jvp_lds_raw[];
    const int lane = static_cast<int>(threadIdx.x);
    const int pack = jvp_pack(nv), kt = jvp_tile_cols(nv), pitch = jvp_pitch(nv), n_vec = jvp_vec_len(nv);
    T *ul_q = reinterpret_cast<T *>(jvp_lds_raw);  // [n_vec]
    T *ul_qd = ul_q + n_vec;                       // [n_vec]
    T *tile = ul_qd + n_vec;                       // [kWave][pitch]
    const int n_blk = (nv + kWave - 1) / kWave;    // row blocks per state
    const int s = pack > 1 ? lane / nv : 0;        // this lane's state of the pack: its vector starts at s * nv
    const size_t nn = static_cast<size_t>(nv) * static_cast<size_t>(nv);
    const int lane_r = lane / kt, lane_c = lane - lane_r * kt, step_r = kWave / kt, step_c = kWave - step_r * kt;  // (no division per load)
    for (size_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const size_t sg = u / static_cast<size_t>(n_blk);
        const int blk = static_cast<int>(u - sg * static_cast<size_t>(n_blk));
        const size_t b0 = sg * static_cast<size_t>(pack);
        const int live_states = static_cast<int>(nb - b0 < static_cast<size_t>(pack) ? nb - b0 : static_cast<size_t>(pack));
        const int row0 = blk * kWave;                                                        // first row of the block within its state
        const int rows = pack > 1 ? live_states * nv : (nv - row0 < kWave ? nv - row0 : kWave);  // live rows of the unit: lanes 0 .. rows - 1
        // the vectors of the unit's states: contiguous in uq / uqd, live_states * nv of them
        const size_t v0 = b0 * static_cast<size_t>(nv);
        const int n_u = live_states * nv;
        for (int k = lane; k < n_u; k += kWave) {
            if (uq) ul_q[k] = uq[v0 + k];
            if (uqd) ul_qd[k] = uqd[v0 + k];
        }
        const size_t m0 = b0 * nn + static_cast<size_t>(row0) * static_cast<size_t>(nv);  // the unit's first row in either matrix
        T acc[2] = {T(0), T(0)};
        for (int m = 0; m < 2; m++) {
            const T *M = m == 0 ? Mq : Mqd;
            const T *ul = (m == 0 ? ul_q : ul_qd) + s * nv;
            if (!M) continue;  // (wave-uniform)
            for (int c0 = 0; c0 < nv; c0 += kt) {
                const int cols = nv - c0 < kt ? nv - c0 : kt;  // live columns of the tile
                const int n_f = rows * kt;                      // load indices of the tile: row f / kt, column f % kt
                __syncthreads();                                // (the previous tile has been read; the vectors are written)
                int r = lane_r, c = lane_c;  // of load index f = lane; a step of kWave indices is step_r rows and step_c columns on
                for (int f0 = 0; f0 < n_f; f0 += kJvpLoads * kWave) {
                    T v[kJvpLoads];
                    int at[kJvpLoads];  // where the value goes in the tile, -1: a lane past the last row or column
#pragma unroll
                    for (int k = 0; k < kJvpLoads; k++) {
                        const bool live = r < rows && c < cols;
                        at[k] = live ? r * pitch + c : -1;
                        v[k] = live ? M[m0 + static_cast<size_t>(r) * static_cast<size_t>(nv) + static_cast<size_t>(c0 + c)] : T(0);
                        r += step_r;
                        c += step_c;
                        if (c >= kt) {
                            c -= kt;
                            r++;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < kJvpLoads; k++)
                        if (at[k] >= 0) tile[at[k]] = v[k];
                }
                __syncthreads();
                if (lane < rows) {
                    const T *row = tile + lane * pitch;
                    T a = acc[m];
                    for (int j = 0; j < cols; j++) a += row[j] * ul[c0 + j];
                    acc[m] = a;
                }
            }
        }
        if (lane < rows) {
            const size_t o = v0 + static_cast<size_t>(row0 + lane);
            const T sum = sign * (acc[0] + acc[1]);
            out[o] = w_add ? w_add[o] + sum : sum;
        }
        __syncthreads();  // (the next unit overwrites the vectors and the tile)
    }
}

}  // namespace

// The launch rule of the contraction: units of work over nb states; LDS for two staged vectors and one tile; a persistent grid of at most
// kJvpWavesPerCu one-wavefront workgroups per CU, no more than the LDS of a CU holds at once, and at most one per unit.
JvpLaunch jvp_contract_launch(int nv, size_t elem, int n_cu, size_t nb)
{
    JvpLaunch L;
    const size_t pack = static_cast<size_t>(jvp_pack(nv));
    const size_t n_blk = (static_cast<size_t>(nv) + kWave - 1) / kWave;
    L.units = (nb + pack - 1) / pack * n_blk;
    L.lds_bytes = ((2 * static_cast<size_t>(jvp_vec_len(nv)) + static_cast<size_t>(kWave) * jvp_pitch(nv)) * elem + 15) / 16 * 16;
    const size_t per_cu = std::max<size_t>(1, std::min(kJvpWavesPerCu, lds_workgroups_per_cu(L.lds_bytes)));
    L.grid = std::min(static_cast<size_t>(n_cu) * per_cu, L.units);
    return L;
}

template <class T>
hipError_t launch_jvp_contract(const JvpLaunch &L, const T *Mq, const T *Mqd, const T *uq, const T *uqd, const T *w_add, T sign, int nv, size_t nb,
                               T *out, hipStream_t stream)
{
    if (nb == 0 || L.grid == 0) return hipSuccess;
    if (L.lds_bytes > kJvpMaxLdsBytes || !out) return hipErrorInvalidValue;
    // (a matrix without its vector, or a vector without its matrix, contributes nothing)
    hipLaunchKernelGGL((jvp_contract_kernel<T>), dim3(static_cast<unsigned>(L.grid)), dim3(kWave), L.lds_bytes, stream, uq ? Mq : nullptr, uqd ? Mqd : nullptr,
                       Mq ? uq : nullptr, Mqd ? uqd : nullptr, w_add, sign, nv, nb, L.units, out);
    return hipGetLastError();
}
template hipError_t launch_jvp_contract<float>(const JvpLaunch &, const float *, const float *, const float *, const float *, const float *, float, int,
                                               size_t, float *, hipStream_t);
template hipError_t launch_jvp_contract<double>(const JvpLaunch &, const double *, const double *, const double *, const double *, const double *, double,
                                                int, size_t, double *, hipStream_t);

}  // namespace grbda_hip
