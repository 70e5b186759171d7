// The field-independent parts of one fused SDF training step (forward + loss + backward of the reference's SDFTrainer,
// wisp/trainers/sdf_trainer.py:65-124, only_last) over an arbitrary-position encoder, written once for hash_sdf_train.hip and
// triplane_sdf_train.hip:
//     pred = decoder([x, features(x)]) ;  loss = sum (pred - gt)^2 / B ;  backward
// Two launches:
//   the field's training kernel  16 lanes own a sample.  The forward is the field's point_inputs + sdf_decode (sdf_decoder_dev.h),
//                         the statements of the field's query kernel: the predicted distance is bit for bit what that kernel returns
//                         for the same parameters.  Then g = 2 (pred - gt) / B and the decoder backward: lane c keeps hidden units c,
//                         c + 16, ..., the gradient of the decoder's feature columns is a column sum over LDS (sdf_step_column_sum).
//                         The encoder's gradient is scattered right there by the field.  Nothing consumes d / d position: not
//                         computed.  Per workgroup the decoder's weight gradients and the squared error are summed by the thread
//                         that owns the entry, in sample order (sdf_step_owner_sum), and stored as one partial row - no atomics.
//   sdf_step_reduce_body  adds the partial rows up in workgroup order, ADDS the sums to the decoder's gradient tensors, writes the
//                         loss, and rounds the fp64 accumulators (SdfWide below) into the encoder's gradient.
// The sums over hidden units, samples and partial rows run in fp64 and are rounded to fp32 once each (products of two floats are
// exact in fp64): that keeps every gradient as close to the float64 result as the modular path's library GEMMs are.
// Determinism: the loss and the four decoder gradients have a fixed summation order and are bitwise repeatable.  What a field
// scatters goes through atomics, f32 or fp64: those sums depend on arrival order and are repeatable only where they are exact.
#pragma once
#include "wisp_common.h"
#include "sdf_decoder_dev.h"

#define SDF_STEP_BLOCK 256
#define SDF_STEP_GROUPS (SDF_STEP_BLOCK / SDF_GROUP)   // samples per workgroup pass
#define SDF_STEP_MAX_LDS (160 * 1024)                  // one workgroup may hold the whole LDS of a compute unit
#define SDF_STEP_WIDE_ENTRIES (1 << 16)                // a level or plane of at most this many entries is summed in fp64

// A small part of the encoder's parameters - where a batch puts many samples on one entry - does not take its gradient by f32
// atomics: an entry's sum of m terms would carry m roundings in arrival order.  It gets fp64 accumulators in scratch (zeroed by the
// step), the scatter adds exact fp64 products with fp64 atomic adds, and the reduce kernel rounds every accumulator once into its
// destination.  off[i] .. off[i + 1]: accumulators of the i-th such part, dst[i]: where its gradient goes, slot[k]: the position of
// part k (a level, a plane) in that list or -1.  The unused tail of off repeats the total.
template <int N> struct SdfWide {
    int64_t off[N + 1];
    float* dst[N];
    int32_t slot[N];
    int n;
};

constexpr int sdf_step_entries(int hidden, int cols) { return hidden * (3 + cols) + 2 * hidden + 2; }
constexpr int sdf_step_row_stride(int hidden, int cols) { return (sdf_step_entries(hidden, cols) + 15) / 16 * 16; }
static inline int sdf_step_grid(int64_t n) { return (int)min64(ceil_div64(n, SDF_STEP_GROUPS), 1024); }
// LDS of a workgroup: what sdf_decoder_stage lays out (weights, the groups' group_floats) | d loss / d pre-activation [groups][H] |
// d loss / d pred * relu output [groups][H] | d loss / d pred [groups] | squared error [groups] | d loss / d feature column
// [groups][cols] | the workgroup's partial row
constexpr size_t sdf_step_lds_bytes(int hidden, int cols, int group_floats) {
    return sdf_decoder_lds_bytes(hidden, cols, group_floats, SDF_STEP_GROUPS) +
           ((size_t)SDF_STEP_GROUPS * (2 * hidden + 2 + cols) + (size_t)sdf_step_entries(hidden, cols)) * sizeof(float);
}

// The training kernel itself stays with each field (hash_sdf_train.hip, triplane_sdf_train.hip: weight staging, LDS carve-up, the
// sample loop with the forward, the loss block and the field's scatter): written once over an encoder policy, the hash kernel came
// out 0.6 % slower at 2^16 coordinates although its sample loop compiled to the same instructions, and the cause was not found
// (profiles/sdf_shared_decoder_ab.txt).  Shared are the two sums in it that round.
//
// sdf_step_column_sum: the gradient of the decoder input, feature columns only (nothing consumes d / d position), of one sample into
// gdx[0 .. cols) - summed in fp64 (every product of two floats is exact there) and rounded once: a chain of up to 256 fp32 fma
// steps was up to three times as far from the float64 result as the modular path's GEMM.  ga: the group's d loss / d
// pre-activation.  All 16 lanes of the group, between two wave barriers of the caller.
static __device__ __forceinline__ void sdf_step_column_sum(const SdfDecoderLds& s, const float* ga, float* gdx, int c, int H, int cols) {
    for (int col = c; col < cols; col += SDF_GROUP) {
        double dx0 = 0.0, dx1 = 0.0;
        int hh = 0;
        for (; hh + 1 < H; hh += 2) {
            dx0 = __builtin_fma((double)ga[hh], (double)s.w1[hh * s.in_pad + 3 + col], dx0);
            dx1 = __builtin_fma((double)ga[hh + 1], (double)s.w1[(hh + 1) * s.in_pad + 3 + col], dx1);
        }
        if (hh < H) dx0 = __builtin_fma((double)ga[hh], (double)s.w1[hh * s.in_pad + 3 + col], dx0);
        gdx[col] = (float)(dx0 + dx1);
    }
}

// sdf_step_owner_sum: the weight gradients of one pass.  s_own holds the workgroup's partial row - d W1 [H][in_dim], d b1 [H],
// d w2 [H], d b2, loss, in that order; every entry has one owner - and the thread that owns an entry adds the pass's samples up in
// order, in fp64, rounded into the fp32 partial sum once per pass.  s_ga / s_gr: [groups][H], s_g / s_sq: [groups].  Every thread
// of the block, between two block barriers of the caller.
static __device__ __forceinline__ void sdf_step_owner_sum(const SdfDecoderLds& s, const float* s_ga, const float* s_gr, const float* s_g,
                                                          const float* s_sq, float* s_own, int H, int in_dim) {
    const int n_entries = H * in_dim + 2 * H + 2;
    for (int e = threadIdx.x; e < n_entries; e += blockDim.x) {
        double acc = 0.0;
        if (e < H * in_dim) {
            const int hh = e / in_dim, k = e - hh * in_dim;
            for (int q = 0; q < SDF_STEP_GROUPS; ++q) acc = __builtin_fma((double)s_ga[q * H + hh], (double)s.in[q * s.stride + k], acc);
        } else if (e < H * in_dim + H) {
            const int hh = e - H * in_dim;
            for (int q = 0; q < SDF_STEP_GROUPS; ++q) acc += (double)s_ga[q * H + hh];
        } else if (e < H * in_dim + 2 * H) {
            const int hh = e - H * in_dim - H;
            for (int q = 0; q < SDF_STEP_GROUPS; ++q) acc += (double)s_gr[q * H + hh];
        } else if (e == H * in_dim + 2 * H) {
            for (int q = 0; q < SDF_STEP_GROUPS; ++q) acc += (double)s_g[q];
        } else {
            for (int q = 0; q < SDF_STEP_GROUPS; ++q) acc += (double)s_sq[q];
        }
        s_own[e] = (float)((double)s_own[e] + acc);
    }
}

template <int N>
static __device__ __forceinline__ void sdf_step_reduce_body(const float* __restrict__ partials, int rows, int row_stride, int H, int in_dim,
                                                            float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2,
                                                            float* __restrict__ gb2, float* __restrict__ loss, float inv_batch,
                                                            const SdfWide<N>& wide, const double* __restrict__ wacc) {
#pragma clang fp contract(off)
    // 16 lanes per entry: lane r adds rows r, r + 16, ... in order, then a fixed butterfly over the 16 lanes - in fp64, rounded once
    const int n_entries = H * in_dim + 2 * H + 2;
    const int r0 = threadIdx.x & 15;
    for (int e = blockIdx.x * 16 + (threadIdx.x >> 4); e < n_entries + 15; e += gridDim.x * 16) {      // (whole groups stay together)
        const bool in = e < n_entries;
        double sum = 0.0;
        if (in)
            for (int r = r0; r < rows; r += 16) sum += (double)partials[(int64_t)r * row_stride + e];
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 16);
        if (!in || r0 != 0) continue;
        const float acc = (float)sum;
        if (e < H * in_dim) gw1[e] += acc;
        else if (e < H * in_dim + H) gb1[e - H * in_dim] += acc;
        else if (e < H * in_dim + 2 * H) gw2[e - H * in_dim - H] += acc;
        else if (e == H * in_dim + 2 * H) gb2[0] += acc;
        else loss[0] = acc * inv_batch;
    }
    // the fp64 sums, rounded once and ADDED to their destination (an untouched accumulator leaves its entry alone)
    const int64_t total = wide.off[wide.n];
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const double v = wacc[e];
        if (v == 0.0) continue;
        int i = 0;
        while (e >= wide.off[i + 1]) ++i;
        wide.dst[i][e - wide.off[i]] += (float)v;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
// scratch: the partial rows (a row is a multiple of 16 floats, so the fp64 accumulators behind them are aligned), then the accumulators
static inline int64_t sdf_step_partials_bytes(int64_t n, int hidden, int cols) {
    return (int64_t)sdf_step_grid(n) * sdf_step_row_stride(hidden, cols) * (int64_t)sizeof(float);
}

template <int N> static inline void sdf_wide_clear(SdfWide<N>& w) {
    w.n = 0;
    for (int i = 0; i <= N; ++i) w.off[i] = 0;
    for (int i = 0; i < N; ++i) { w.dst[i] = nullptr; w.slot[i] = -1; }
}
template <int N> static inline void sdf_wide_add(SdfWide<N>& w, int part, float* dst, int64_t entries) {
    w.slot[part] = w.n;
    w.dst[w.n] = dst;
    for (int i = w.n + 1; i <= N; ++i) w.off[i] = w.off[w.n] + entries;
    ++w.n;
}

// the memset of the accumulators (only when there are any) and the two launches.  Train(coords, gts, n, fld, inv_batch, target,
// partials, row_stride, wide, wacc) is the field's training kernel, Reduce(partials, rows, row_stride, H, in_dim, four gradients,
// loss, inv_batch, wide, wacc) its __global__ wrapper of sdf_step_reduce_body; target is what its scatter adds into with f32 atomics.
template <auto Train, auto Reduce, class Field, class Target, class Wide>
static inline int sdf_step_launch(const char* fn, const float* coords, const float* gts, int64_t n, const Field& fld, int group_floats,
                                  Target target, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, float* loss,
                                  void* scratch, const Wide& wide, hipStream_t s) {
    const int hidden = fld.dec.hidden, cols = fld.dec.cols;
    const size_t lds = sdf_step_lds_bytes(hidden, cols, group_floats);
    const int grid = sdf_step_grid(n), row_stride = sdf_step_row_stride(hidden, cols);
    float* partials = static_cast<float*>(scratch);
    double* wacc = reinterpret_cast<double*>(partials + (size_t)grid * row_stride);
    const float inv_batch = 1.0f / (float)n;
    if (const hipError_t e = WISP_ALLOW_LDS(Train, lds)) return wisp_fail(WISP_ERR_LAUNCH, fn, hipGetErrorString(e));
    if (wide.off[wide.n] > 0 && hipMemsetAsync(wacc, 0, (size_t)wide.off[wide.n] * sizeof(double), s) != hipSuccess)
        return wisp_fail(WISP_ERR_LAUNCH, fn, "hipMemsetAsync failed");
    hipLaunchKernelGGL(Train, dim3(grid), dim3(SDF_STEP_BLOCK), lds, s, coords, gts, n, fld, inv_batch, target, partials, row_stride, wide,
                       wacc);
    hipLaunchKernelGGL(Reduce, dim3((sdf_step_entries(hidden, cols) + 15) / 16), dim3(256), 0, s, partials, grid, row_stride, hidden,
                       3 + cols, grad_w1, grad_b1, grad_w2, grad_b2, loss, inv_batch, wide, wacc);
    if (const hipError_t e = hipGetLastError()) return wisp_fail(WISP_ERR_LAUNCH, fn, hipGetErrorString(e));
    return WISP_OK;
}
