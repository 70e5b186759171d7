// The density half of the exact-fp32 decoder - layer 1 (IN -> H, relu) and layer 2 (H -> 16) on v_mfma_f32_32x32x2_f32 - shared by
// nerf_mlp_kernel<float, ...> (nerf_mlp.hip) and the fused prune query (prune_query.hip).  One definition of the MFMA sequence, of
// the LDS strides and of the bias / relu epilogue, so that a density computed by either kernel from the same feature row and the
// same parameters is the same bits.
#pragma once
#include "wisp_common.h"
#include "nerf_mlp_shape.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace wisp_mlp {

// LDS strides of the fp32 tiles: row-major [row][K] with one pad element, so that the MFMA operand reads are bank-conflict free
constexpr int F32_PAD = 1;
constexpr int F32_LDI = IN + F32_PAD;     // [.][IN] tiles: W1, x0
constexpr int F32_LDH = H + F32_PAD;      // [.][H] tiles: W2 (32 rows, 16 real), h1

// D[i][n] += sum_k A[i][k] * B[n][k]   (A = 32 weight rows, B = the wave's 32 samples), K a multiple of 2; bit for bit an fmaf
// chain over k = 0 .. K - 1
template <int K>
static __device__ __forceinline__ void f32_mma_nt(const float* A, int lda, const float* B, int ldb, floatx16& acc, int lane) {
    const float* pa = A + (lane & 31) * lda + (lane >> 5);
    const float* pb = B + (lane & 31) * ldb + (lane >> 5);
#pragma unroll
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k], pb[k], acc, 0, 0, 0);
}

// row of accumulator register `reg` for this lane (C/D layout of the 32x32 MFMA shapes)
static __device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

static __device__ __forceinline__ floatx16 zero16() {
    floatx16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.0f;
    return z;
}

// W1 [H][F32_LDI], b1 [H], W2 [32][F32_LDH] (rows 16.. zero), b2 [32] from the caller's packed parameters into LDS images that
// the caller has ZEROED (padding rows / columns must be 0) and synchronised; the caller synchronises again afterwards.
static __device__ __forceinline__ void f32_stage_density_params(const float* __restrict__ params, int in_dim, float* w1, float* b1,
                                                                float* w2, float* b2, int tid, int nthreads) {
    for (int e = tid; e < H * IN; e += nthreads) w1[(e / IN) * F32_LDI + e % IN] = packed_param(params, OW1 + e, in_dim);
    for (int e = tid; e < 16 * H; e += nthreads) w2[(e / H) * F32_LDH + e % H] = packed_param(params, OW2 + e, in_dim);
    for (int e = tid; e < H; e += nthreads) b1[e] = packed_param(params, OB1 + e, in_dim);
    if (tid < 16) b2[tid] = packed_param(params, OB2 + tid, in_dim);
}

}  // namespace wisp_mlp

// The two stages are statement macros, not functions: nerf_mlp_kernel's backward instantiations sit at the 512-register limit and
// the register allocator spilled as soon as these loops reached it through a call (even a force-inlined one), while the same
// statements expanded in place compile to the code they were before they moved here.  Names in scope: SW / SB = the LDS weight /
// bias images (float*), OW.. / OB.. = offsets of the layer inside them, N = lane & 31 (the sample), LANE.
// L1: H1[N][0..H) = relu(W1 X0[N] + b1); X0 [32][F32_LDI], H1 [32][F32_LDH]
#define WISP_F32_LAYER1(SW, OW1_, SB, OB1_, X0, H1, N, LANE)                                                            \
    _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_) {                                                                  \
        floatx16 acc_ = wisp_mlp::zero16();                                                                             \
        wisp_mlp::f32_mma_nt<wisp_mlp::IN>((SW) + (OW1_) + t_ * 32 * wisp_mlp::F32_LDI, wisp_mlp::F32_LDI, X0,          \
                                           wisp_mlp::F32_LDI, acc_, LANE);                                              \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                             \
            const int row_ = t_ * 32 + wisp_mlp::acc_row(r_, LANE);                                                     \
            (H1)[(N) * wisp_mlp::F32_LDH + row_] = fmaxf(acc_[r_] + (SB)[(OB1_) + row_], 0.0f);                         \
        }                                                                                                               \
    }
// L2: y = W2 H1[N] + b2; Y0 (a float lvalue) = y[0], the density logit - it lands in the lanes below 32 (row 0 is register 0 of
// those); GEO (a constant): the geometry features y[1..15] go to X2[N][0..14] (row stride F32_LDH), the colour network's input
#define WISP_F32_LAYER2(SW, OW2_, SB, OB2_, H1, N, LANE, Y0, GEO, X2)                                                   \
    {                                                                                                                   \
        floatx16 acc_ = wisp_mlp::zero16();                                                                             \
        wisp_mlp::f32_mma_nt<wisp_mlp::H>((SW) + (OW2_), wisp_mlp::F32_LDH, H1, wisp_mlp::F32_LDH, acc_, LANE);         \
        _Pragma("unroll") for (int r_ = 0; r_ < 8; ++r_) {      /* rows 0..15 live in regs 0..7 (rows 16.. are padding) */ \
            const int row_ = wisp_mlp::acc_row(r_, LANE);                                                               \
            const float y_ = acc_[r_] + (SB)[(OB2_) + row_];                                                            \
            if (row_ == 0) Y0 = y_; else if (GEO) (X2)[(N) * wisp_mlp::F32_LDH + row_ - 1] = y_;                        \
        }                                                                                                               \
    }
