// The two small sums that end a training step's backward - the decoder's dW partial rows and the per-ray loss partials - as
// __device__ functions of (workgroup index, thread index), so that they can run either as launches of their own
// (nerf_mlp_reduce_kernel, loss_sum_kernel) or as extra workgroups of a launch that is in the stream anyway (the hash-grid reduce
// launch, hashgrid.hip: "side jobs").  The arithmetic exists once, here: same summation order, same bits, whoever calls.
// Both expect a workgroup of STEP_TAIL_THREADS threads, all of which make the call (there are barriers inside).
#pragma once
#include "nerf_mlp_shape.h"

#define STEP_TAIL_THREADS 1024
#define STEP_TAIL_DW_LDS_FLOATS (16 * 64)
#define STEP_TAIL_LOSS_LDS_FLOATS 16

namespace wisp_tail {

constexpr int DW_COL_BLOCKS = (wisp_mlp::NPARAM + 63) / 64;

// grad_params[packed(j)] += sum over partial rows (rows are in canonical order, nerf_mlp_shape.h), for the 64 parameters
// [wg * 64, wg * 64 + 64); DW_COL_BLOCKS workgroups cover the vector.  Thread = column tx of row group ty (16 groups): per element the
// partial rows r = ty, ty + 16, ... are added in that order, then the 16 group sums in index order, then the element is added to
// grad_params.  `s`: STEP_TAIL_DW_LDS_FLOATS floats of LDS.
__device__ __forceinline__ void dw_reduce(const float* __restrict__ partials, int rows, int in_dim, float* __restrict__ grad_params,
                                          int wg, int tid, float* __restrict__ s) {
    using namespace wisp_mlp;
    const int tx = tid & 63, ty = tid >> 6;
    const int j = wg * 64 + tx;
    float a = 0.0f;
    if (j < NPARAM)
        for (int r = ty; r < rows; r += 16) a += partials[(int64_t)r * NPARAM_PAD + j];
    s[ty * 64 + tx] = a;
    __syncthreads();
    if (ty == 0 && j < NPARAM) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += s[k * 64 + tx];
        const int dst = packed_index(j, in_dim);
        if (dst >= 0) grad_params[dst] += t;
    }
}

// loss[0] = (sum of partial[0 .. n)) * inv_n, one workgroup: per-thread strided sums in blocks of 8 x 1024 (eight loads of a thread in
// flight at once), the 64-lane shuffle-down tree, then the 16 wave sums in index order.  `part`: STEP_TAIL_LOSS_LDS_FLOATS floats of LDS.
__device__ __forceinline__ void loss_sum(const float* __restrict__ partial, int n, float inv_n, float* __restrict__ loss, int tid,
                                         float* __restrict__ part) {
    float t = 0.0f;
    for (int base = 0; base < n; base += 8 * STEP_TAIL_THREADS) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int i = base + tid + k * STEP_TAIL_THREADS; v[k] = i < n ? partial[i] : 0.0f; }
#pragma unroll
        for (int k = 0; k < 8; ++k) t += v[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    if ((tid & 63) == 0) part[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < 16; ++w) s += part[w];
        loss[0] = s * inv_n;
    }
}

}  // namespace wisp_tail
