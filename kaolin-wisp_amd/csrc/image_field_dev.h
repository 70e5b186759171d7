// Per-pixel forward of ImageNeuralField.rgb, shared by the whole-image render (image_field.hip) and the fused training step
// (image_field_train.hip): the level blend with its last-row pin, the embedding layout, the decoder's accumulation steps and the
// sigmoid expression.  One definition each, so a colour is the same bits whichever kernel computes it:
//   unit j   = b1[j], then one image_fma per input in column order (feature columns, then the 14 embedding values);
//   output k = b2[k], then one image_fma per hidden unit, ascending, on image_relu of the unit;
//   colour   = image_sigmoid(output).
#pragma once
#include "wisp_common.h"
#include "hashgrid_dev.h"

#define IF_MAX_LODS 16
#define IF_EMBED 14                               // x, y, sin / cos of (x, y) * (1, 2, 4)
#define IF_IN (IF_MAX_LODS * 2 + IF_EMBED)        // rows of the packed first layer: 32 feature rows (absent levels: zero), 14 embedding
#define IF_PIECE 32                               // hidden units per pass of the render kernel
#define IF_MAX_HIDDEN 128

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Corner rows (relative to the level's first row) and blend factors of one level: corner_setup of hashgrid_dev.h and, as
// hashgrid_fwd_kernel does for dense levels from resolution 258 on, the read pinned to the table's last row.
// level_first: the level's first row in the table, table_rows: rows of the whole table.
static __device__ __forceinline__ void image_level_corners(const float* __restrict__ c, int32_t res, float hi, float hr, bool dense,
                                                           uint32_t tsize, bool tsize_pow2, int64_t level_first, int64_t table_rows,
                                                           CornerSetup<2>& cs) {
    corner_setup<2>(c, res, hi, hr, dense, tsize, tsize_pow2, cs);
    if (dense && res >= 258) {
        const int64_t last = table_rows - 1 - level_first;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((int64_t)(uint32_t)cs.idx[j] > last) cs.idx[j] = (int32_t)last;
    }
}

// The blend of hashgrid_fwd_kernel's plain path: `acc[k] += table[idx[j]][k] * coef[j]`, corners in index order.
// table: the level's first row ([rows][2] f32).
static __device__ __forceinline__ void image_level_blend(const float* __restrict__ table, const CornerSetup<2>& cs,
                                                         float* __restrict__ acc) {
    float2 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float2*>(table + (int64_t)cs.idx[j] * 2);
    // One fused multiply-add per corner, from zero - what the compiler's contraction made of `acc += v * coef` in the render
    // kernel.  Spelled out: left to the optimizer, whether a product fuses into its sum depends on how the surrounding code
    // was vectorized, and the two kernels that inline this function would round differently.
    acc[0] = 0.0f; acc[1] = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { acc[0] = __builtin_fmaf(v[j].x, cs.coef[j], acc[0]); acc[1] = __builtin_fmaf(v[j].y, cs.coef[j], acc[1]); }
}

// PositionalEmbedder's layout: [x, y | sin(1x) sin(1y) sin(2x) sin(2y) sin(4x) sin(4y) | cos(same)].  Entry pair r = 2 f + a
// (octave f, axis a) of the sine block and of the cosine block: e[2 + r] = s, e[8 + r] = co.
static __device__ __forceinline__ void image_embed_pair(const float* __restrict__ c, int r, float& s, float& co) {
    const float t = c[r & 1] * (float)(1 << (r >> 1));                     // exact: a power of two
    s = sinf(t);
    co = cosf(t);
}
static __device__ __forceinline__ void image_embed(const float* __restrict__ c, float* __restrict__ e) {
    e[0] = c[0]; e[1] = c[1];
#pragma unroll
    for (int r = 0; r < 6; ++r) image_embed_pair(c, r, e[2 + r], e[8 + r]);
}

static __device__ __forceinline__ float image_fma(float x, float w, float acc) { return __builtin_fmaf(x, w, acc); }
static __device__ __forceinline__ float image_relu(float a) { return fmaxf(a, 0.0f); }
static __device__ __forceinline__ float image_sigmoid(float o) { return 1.0f / (1.0f + expf(-o)); }

// The decoder over wisp_image_field_render's packed weights, 32 hidden units at a time; every weight is a scalar operand.
// weights: [IF_IN][hp] first layer, transposed | b1 [hp] | W2 [3][hp] | b2 [3]  ->  the three pre-sigmoid outputs
static __device__ __forceinline__ void image_decode_packed(const float* __restrict__ x, const float* __restrict__ weights, int hp,
                                                           float* __restrict__ o) {
    const float* __restrict__ b1 = weights + (size_t)IF_IN * hp;
    const float* __restrict__ w2 = b1 + hp;
    const float* __restrict__ b2 = w2 + 3 * (size_t)hp;
    float o0 = b2[0], o1 = b2[1], o2 = b2[2];
    for (int piece = 0; piece < hp; piece += IF_PIECE) {
        float hacc[IF_PIECE];
        {
            const f32x16 ba = *reinterpret_cast<const f32x16*>(b1 + piece), bb = *reinterpret_cast<const f32x16*>(b1 + piece + 16);
#pragma unroll
            for (int j = 0; j < 16; ++j) { hacc[j] = ba[j]; hacc[16 + j] = bb[j]; }
        }
#pragma unroll
        for (int k = 0; k < IF_IN; ++k) {
            const float* __restrict__ wr = weights + (size_t)k * hp + piece;
            const f32x16 wa = *reinterpret_cast<const f32x16*>(wr), wb = *reinterpret_cast<const f32x16*>(wr + 16);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                hacc[j] = image_fma(x[k], wa[j], hacc[j]);
                hacc[16 + j] = image_fma(x[k], wb[j], hacc[16 + j]);
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const f32x16 u0 = *reinterpret_cast<const f32x16*>(w2 + piece + half * 16);
            const f32x16 u1 = *reinterpret_cast<const f32x16*>(w2 + hp + piece + half * 16);
            const f32x16 u2 = *reinterpret_cast<const f32x16*>(w2 + 2 * hp + piece + half * 16);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float a = image_relu(hacc[half * 16 + j]);
                o0 = image_fma(a, u0[j], o0); o1 = image_fma(a, u1[j], o1); o2 = image_fma(a, u2[j], o2);
            }
        }
    }
    o[0] = o0; o[1] = o1; o[2] = o2;
}
