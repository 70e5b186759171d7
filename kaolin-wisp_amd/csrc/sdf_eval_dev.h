// Field evaluation of the nglod shape as one __device__ function: NeuralSDF / NeuralSDFTex over an OctreeGrid
// (wisp/models/nefs/neural_sdf.py:120-155, neural_sdf_tex.py:85-123: OctreeGrid.interpolate 'sum' over the active levels ->
// [position, features] -> Linear -> relu -> Linear).  The only evaluator of this shape outside training: the query, gradient
// and marching kernels of sdf_eval.hip all call it, so that a value the gradient kernel differences, or a distance the march
// advances by, is bit for bit the value the query kernel returns for the same position.
//
// 16 lanes own one point.  They walk the octree once (the voxel on every active level; a point outside [-1,1]^3 or in an
// unoccupied cell gets zero features and the decoder still runs, as grid.interpolate + decoder do); lane c gathers feature
// channel c of the 8 corners per level: one contiguous 64-byte row per corner and group; the hidden layer is split over the
// lanes (weights in LDS), the ROWS output dot products are reduced over the group with four shuffles each.  Walk, trilinear
// weights and level sum follow spc_query_kernel (csrc/spc.hip) / spc_trilinear_multi_fwd_kernel (csrc/spc_interp.hip), so
// cells and features are those of the modular path; the decoder is an fp32 fma chain in input order, which differs from the
// library GEMM of the modular path by summation order only.
#pragma once
#include "wisp_common.h"

#define SDFE_GROUP 16
#define SDFE_CHANNELS 16
#define SDFE_IN (3 + SDFE_CHANNELS)
#define SDFE_IN_PAD (SDFE_IN | 1)            // odd row stride: the lanes of a group read different rows
#define SDFE_MAX_HIDDEN 256
#define SDFE_MAX_LODS 16

struct SdfEvalField {
    const void* feats[SDFE_MAX_LODS];
    int32_t level[SDFE_MAX_LODS];
    int num_lods, half_round, hidden, max_level;
    const float *w1, *b1, *w2, *b2;           // [hidden, 19], [hidden], [ROWS, hidden], [ROWS]
    const uint8_t* octree;
    const int32_t* exsum;
    const int16_t* points;
    const int32_t* trinkets;
};

// LDS of a block: W1 [hidden][SDFE_IN_PAD], b1 [hidden], W2 [rows][hidden] | per group: the 19 decoder inputs
struct SdfEvalLds { float *w1, *b1, *w2, *in; };

static inline size_t sdf_eval_lds_bytes(int hidden, int rows, int groups) {
    return ((size_t)hidden * SDFE_IN_PAD + (size_t)hidden + (size_t)rows * hidden + (size_t)groups * SDFE_IN) * sizeof(float);
}

// every thread of the block; ends with the block barrier
static __device__ __forceinline__ SdfEvalLds sdf_eval_stage(float* base, const SdfEvalField& fld, int rows) {
    SdfEvalLds s;
    s.w1 = base;
    s.b1 = s.w1 + fld.hidden * SDFE_IN_PAD;
    s.w2 = s.b1 + fld.hidden;
    s.in = s.w2 + rows * fld.hidden;
    for (int e = threadIdx.x; e < fld.hidden * SDFE_IN; e += blockDim.x) s.w1[(e / SDFE_IN) * SDFE_IN_PAD + e % SDFE_IN] = fld.w1[e];
    for (int e = threadIdx.x; e < fld.hidden; e += blockDim.x) s.b1[e] = fld.b1[e];
    for (int e = threadIdx.x; e < rows * fld.hidden; e += blockDim.x) s.w2[e] = fld.w2[e];
    __syncthreads();
    return s;
}

// Every rounding below is spelled out (explicit fmaf, the compiler's own contraction switched off).  Left to the compiler, the
// two inlined copies of this function in the gradient kernel and the copy in the query kernel were scheduled differently and
// returned values that differed in rare points by one fp16 ulp behind half_round (a blend one fp32 ulp apart rounds to the
// other fp16 neighbour): seen on an MI355X as central differences thousands of ulps away from the query's own values.  The
// spelling is what contraction makes of the statements of trilinear_coeffs / spc_trilinear_multi_fwd_kernel
// (csrc/spc_interp.hip): x = fma(2^l, fma(0.5, c, 0.5), -pt), weight products left to right, blend = fma chain over the corners
// in corner order.  Against the modular path the outputs then differ by summation order of the decoder at most (measured:
// DESIGN.md section 4).
static __device__ __forceinline__ void sdf_eval_coeffs(const float (&c)[3], const int16_t* __restrict__ pt, int level, float (&w)[8]) {
#pragma clang fp contract(off)
    const float res = (float)(1 << level);
    float f[3], g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        f[a] = __builtin_fmaf(res, __builtin_fmaf(0.5f, c[a], 0.5f), -(float)pt[a]);
        g[a] = 1.0f - f[a];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (((j & 4) ? f[0] : g[0]) * ((j & 2) ? f[1] : g[1])) * ((j & 1) ? f[2] : g[2]);
}

// All 16 lanes of a group call this together, with the same position: the reduction shuffles have width 16 and the barriers
// order one group's LDS traffic, so the wave's other groups need not be here (a marching kernel's group leaves early as a
// whole).  c = lane within the group, gin = the group's 19 floats of LDS.  On return every lane holds the ROWS raw decoder
// outputs (bias added) in the order the module produces them.
template <typename T, int ROWS>
static __device__ __forceinline__ void sdf_eval_point(const SdfEvalField& fld, const SdfEvalLds& s, float* gin, int c,
                                                      float px, float py, float pz, float (&out)[ROWS]) {
#pragma clang fp contract(off)
    const int L = fld.max_level;
    const bool inside = (fabsf(px) <= 1.0f) && (fabsf(py) <= 1.0f) && (fabsf(pz) <= 1.0f);
    const float res = (float)(1 << L);
    const int top = (1 << L) - 1;
    // (the cell only of a point inside the cube: far-outside or NaN coordinates never reach the float -> int conversion)
    const int qx = inside ? min((int)floorf(res * __builtin_fmaf(0.5f, px, 0.5f)), top) : 0;
    const int qy = inside ? min((int)floorf(res * __builtin_fmaf(0.5f, py, 0.5f)), top) : 0;
    const int qz = inside ? min((int)floorf(res * __builtin_fmaf(0.5f, pz, 0.5f)), top) : 0;
    const float pos[3] = {px, py, pz};
    float feat = 0.0f;                                   // channel c, summed over the levels
    int64_t node = inside ? 0 : -1;
    int li = 0;
    for (int l = 0; l <= L && li < fld.num_lods; ++l) {
        if (l == fld.level[li]) {
            float acc = 0.0f;
            if (node >= 0) {
                float w[8];
                sdf_eval_coeffs(pos, fld.points + node * 3, l, w);
                const int32_t* tr = fld.trinkets + node * 8;
                const T* f = reinterpret_cast<const T*>(fld.feats[li]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float fv = Cvt<T>::to_f(f[(int64_t)tr[j] * SDFE_CHANNELS + c]);
                    if (fld.half_round) fv = __half2float(__float2half_rn(fv));
                    acc = __builtin_fmaf(fv, w[j], acc);
                }
                if (fld.half_round) acc = __half2float(__float2half_rn(acc));
            }
            feat += acc;
            ++li;
        }
        if (l < L && node >= 0) {
            const int sh = L - 1 - l;
            const int cs = (((qx >> sh) & 1) << 2) | (((qy >> sh) & 1) << 1) | ((qz >> sh) & 1);
            const uint32_t bits = fld.octree[node];
            node = ((bits >> cs) & 1u) ? (int64_t)fld.exsum[node] + __popc(bits & ((2u << cs) - 1u)) : -1;
        }
    }
    // ---- decoder: in = [position, features]
    __builtin_amdgcn_wave_barrier();                     // the previous evaluation's reads of gin are done
    if (c < 3) gin[c] = pos[c];
    gin[3 + c] = feat;
    __builtin_amdgcn_wave_barrier();                     // the group's lanes are in one wave: LDS order suffices
    float o[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) o[r] = 0.0f;
    for (int hh = c; hh < fld.hidden; hh += SDFE_GROUP) {
        const float* wr = s.w1 + hh * SDFE_IN_PAD;
        float a = s.b1[hh];
#pragma unroll
        for (int i = 0; i < SDFE_IN; ++i) a = __builtin_fmaf(wr[i], gin[i], a);
        const float h = fmaxf(a, 0.0f);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) o[r] = __builtin_fmaf(s.w2[r * fld.hidden + hh], h, o[r]);
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        float v = o[r];
#pragma unroll
        for (int d = SDFE_GROUP / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, SDFE_GROUP);
        out[r] = v + fld.b2[r];
    }
}
