// The one decoder of the fused SDF fields over an arbitrary-position encoder (hash grid: hash_sdf_eval_dev.h, triplanar grid:
// triplane_sdf_eval_dev.h): [position, features] -> Linear(3 + cols, hidden) -> relu -> Linear(hidden, 1), 16 lanes a point.  The
// hidden layer is split over the lanes (weights in LDS, odd row stride), every unit is an fp32 fma chain in input order, the output
// dot product is reduced with four shuffles of width 16, b2 is added last.  Every rounding is spelled out - explicit fmaf, the
// compiler's own contraction switched off - for the reason recorded at sdf_eval_coeffs (sdf_eval_dev.h): inlined copies of one
// function were scheduled differently and returned different bits.  Written once, so that a value the gradient kernel differences,
// a distance the marching kernel steps by and a prediction a training step takes its loss from are bit for bit what the query
// kernel returns for the same position, for every field of this family.
#pragma once
#include "wisp_common.h"

#define SDF_GROUP 16                                   // lanes per point
#define SDF_MAX_HIDDEN 256

struct SdfDecoder {
    int cols, hidden;                                  // cols = decoder feature columns K
    const float *w1, *b1, *w2, *b2;                    // [hidden, 3 + cols], [hidden], [hidden], [1]
};

// LDS of a block: W1 [hidden][in_pad], b1 [hidden], w2 [hidden] | per group `stride` floats: the 3 + cols decoder inputs, then
// whatever the encoder keeps behind them
struct SdfDecoderLds { float *w1, *b1, *w2, *in; int in_pad, stride; };

constexpr int sdf_decoder_in_pad(int cols) { return (3 + cols) | 1; }            // odd row stride: the lanes of a group read different rows
constexpr size_t sdf_decoder_lds_bytes(int hidden, int cols, int group_floats, int groups) {
    return ((size_t)hidden * sdf_decoder_in_pad(cols) + 2 * (size_t)hidden + (size_t)groups * group_floats) * sizeof(float);
}

// every thread of the block; ends with the block barrier
static __device__ __forceinline__ SdfDecoderLds sdf_decoder_stage(float* base, const SdfDecoder& dec, int group_floats) {
    SdfDecoderLds s;
    const int in_dim = 3 + dec.cols;
    s.in_pad = in_dim | 1;
    s.stride = group_floats;
    s.w1 = base;
    s.b1 = s.w1 + dec.hidden * s.in_pad;
    s.w2 = s.b1 + dec.hidden;
    s.in = s.w2 + dec.hidden;
    for (int e = threadIdx.x; e < dec.hidden * in_dim; e += blockDim.x) s.w1[(e / in_dim) * s.in_pad + e % in_dim] = dec.w1[e];
    for (int e = threadIdx.x; e < dec.hidden; e += blockDim.x) { s.b1[e] = dec.b1[e]; s.w2[e] = dec.w2[e]; }
    __syncthreads();
    return s;
}

// The decoder over gin = the group's [position, features]; returns the raw output with the bias added.  All 16 lanes of a group
// call it together (the shuffles stay inside the group); c = lane within the group.  KEEP (the training step): lane c also
// leaves, for its hidden units hh = c, c + 16, ..., w2[hh] where the unit is active (0 elsewhere) in ga[hh] and the unit's relu
// output in gr[hh] - stores only, the arithmetic is the same statements.
template <bool KEEP>
static __device__ __forceinline__ float sdf_decode(const SdfDecoder& dec, const SdfDecoderLds& s, const float* gin, int c, float* ga,
                                                   float* gr) {
#pragma clang fp contract(off)
    const int in_dim = 3 + dec.cols;
    float o = 0.0f;
    for (int hh = c; hh < dec.hidden; hh += SDF_GROUP) {
        const float* wr = s.w1 + hh * s.in_pad;
        float a = s.b1[hh];
        for (int i = 0; i < in_dim; ++i) a = __builtin_fmaf(wr[i], gin[i], a);
        o = __builtin_fmaf(s.w2[hh], fmaxf(a, 0.0f), o);
        if (KEEP) {
            ga[hh] = a > 0.0f ? s.w2[hh] : 0.0f;
            gr[hh] = fmaxf(a, 0.0f);
        }
    }
#pragma unroll
    for (int d = SDF_GROUP / 2; d >= 1; d >>= 1) o += __shfl_xor(o, d, SDF_GROUP);
    return o + dec.b2[0];
}
