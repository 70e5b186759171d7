// The exact-fp32 decoder's stages on v_mfma_f32_32x32x2_f32 - layer 1 (IN -> H, relu), layer 2 (H -> 16), the view encoding, layers
// 3 - 5 and the sigmoid - shared by nerf_mlp_kernel<float, ...> (nerf_mlp.hip), the fused prune query (prune_query.hip, the density
// half) and the fused field query (nerf_query.hip, all of it).  One definition of the MFMA sequence, of the LDS strides and of the
// bias / relu / sigmoid epilogues, so that a value computed by any of these kernels from the same feature row, the same view
// direction and the same parameters is the same bits.
#pragma once
#include "wisp_common.h"
#include "nerf_mlp_shape.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace wisp_mlp {

// LDS strides of the fp32 tiles: row-major [row][K] with one pad element, so that the MFMA operand reads are bank-conflict free
constexpr int F32_PAD = 1;
constexpr int F32_LDI = IN + F32_PAD;     // [.][IN] tiles: W1, x0
constexpr int F32_LDH = H + F32_PAD;      // [.][H] tiles: W2 (32 rows, 16 real), h1
constexpr int F32_K3 = 48;                // X2 = 42 colour inputs padded to the MFMA K granularity

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

// the colour network the same way: W3 [H][F32_LDH] (columns X2.. zero), W4 [H][F32_LDH], W5 [32][F32_LDH] (rows 3.. zero), b3 / b4 [H],
// b5 [32]
static __device__ __forceinline__ void f32_stage_color_params(const float* __restrict__ params, int in_dim, float* w3, float* b3,
                                                              float* w4, float* b4, float* w5, float* b5, int tid, int nthreads) {
    for (int e = tid; e < H * X2; e += nthreads) w3[(e / X2) * F32_LDH + e % X2] = packed_param(params, OW3 + e, in_dim);
    for (int e = tid; e < H * H; e += nthreads) w4[(e / H) * F32_LDH + e % H] = packed_param(params, OW4 + e, in_dim);
    for (int e = tid; e < 3 * H; e += nthreads) w5[(e / H) * F32_LDH + e % H] = packed_param(params, OW5 + e, in_dim);
    for (int e = tid; e < H; e += nthreads) { b3[e] = packed_param(params, OB3 + e, in_dim); b4[e] = packed_param(params, OB4 + e, in_dim); }
    if (tid < 3) b5[tid] = packed_param(params, OB5 + tid, in_dim);
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

// ---- the colour half: view encoding, layers 3 - 5, sigmoid - shared by nerf_mlp_kernel<float, ...> and the fused field query
// (nerf_query.hip), statement macros for the reason given above.  HALF = LANE >> 5.
// Positional encoding of the view direction D (float[3], zeros for a dead sample) -> X2[N][15..41], and zeros in the K padding
// X2[N][42..63].  Layout [d ; sin(2^k d) k-major ; cos(2^k d) k-major] (positional_embedder.py:61-65).  The two half-waves split
// the work: half 0 writes d and the sines, half 1 the cosines and the padding; one accurate sinf / cosf per band (bit-compatible
// with torch.sin / torch.cos to ~1 ulp).  XV = the x2 tile, [32][F32_LDH]
#define WISP_F32_VIEW_ENCODE(XV, N, HALF, D)                                                                            \
    {                                                                                                                   \
        float* row_ = (XV) + (N) * wisp_mlp::F32_LDH + 15;                                                              \
        if ((HALF) == 0) {                                                                                              \
            _Pragma("unroll") for (int a_ = 0; a_ < 3; ++a_) row_[a_] = (D)[a_];                                        \
        } else {                                                                                                        \
            _Pragma("unroll") for (int k_ = wisp_mlp::X2; k_ < 64; ++k_) (XV)[(N) * wisp_mlp::F32_LDH + k_] = 0.0f;     \
        }                                                                                                               \
        _Pragma("unroll") for (int a_ = 0; a_ < 3; ++a_) {                                                              \
            _Pragma("unroll") for (int k_ = 0; k_ < wisp_mlp::NF; ++k_) {                                               \
                const float arg_ = (float)(1 << k_) * (D)[a_];                                                          \
                const float val_ = (HALF) == 0 ? sinf(arg_) : cosf(arg_);                                               \
                row_[3 + (HALF) * 3 * wisp_mlp::NF + k_ * 3 + a_] = val_;                                               \
            }                                                                                                           \
        }                                                                                                               \
    }
// L3 (KDIM = F32_K3: X2 padded to the MFMA K granularity) and L4 (KDIM = H): HOUT[N][0..H) = relu(W XIN[N] + b); W [H][F32_LDH],
// XIN, HOUT [32][F32_LDH]
#define WISP_F32_LAYER_HIDDEN(SW, OW_, SB, OB_, KDIM, XIN, HOUT, N, LANE)                                               \
    _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_) {                                                                  \
        floatx16 acc_ = wisp_mlp::zero16();                                                                             \
        wisp_mlp::f32_mma_nt<KDIM>((SW) + (OW_) + t_ * 32 * wisp_mlp::F32_LDH, wisp_mlp::F32_LDH, XIN, wisp_mlp::F32_LDH, \
                                   acc_, LANE);                                                                         \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                             \
            const int row_ = t_ * 32 + wisp_mlp::acc_row(r_, LANE);                                                     \
            (HOUT)[(N) * wisp_mlp::F32_LDH + row_] = fmaxf(acc_[r_] + (SB)[(OB_) + row_], 0.0f);                        \
        }                                                                                                               \
    }
// L5 and its epilogue: SG[c] (a float[3]) = sigmoid(W5 H3[N] + b5)[c]; rows 0..2 are registers 0..2 of the lanes below 32
#define WISP_F32_LAYER5(SW, OW5_, SB, OB5_, H3, LANE, SG)                                                               \
    {                                                                                                                   \
        floatx16 acc_ = wisp_mlp::zero16();                                                                             \
        wisp_mlp::f32_mma_nt<wisp_mlp::H>((SW) + (OW5_), wisp_mlp::F32_LDH, H3, wisp_mlp::F32_LDH, acc_, LANE);         \
        _Pragma("unroll") for (int c_ = 0; c_ < 3; ++c_) (SG)[c_] = 1.0f / (1.0f + expf(-(acc_[c_] + (SB)[(OB5_) + c_]))); \
    }
