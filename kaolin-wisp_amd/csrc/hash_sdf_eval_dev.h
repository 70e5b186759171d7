// Field evaluation of the nglod_hash shape as one __device__ function: NeuralSDF over a HashGrid
// (wisp/models/nefs/neural_sdf.py:120-155 over wisp/models/grids/hash_grid.py:205-233: HashGrid.interpolate 'cat' with the
// columns from lod_idx * feature_dim on zeroed, or 'sum' over the levels -> [position, features] -> Linear -> relu -> Linear).
// This file is the ENCODER half, hash_sdf_point_inputs; the decoder is sdf_decoder_dev.h's, and the two are put together by the
// kernel bodies of sdf_point_kernels_dev.h (hash_sdf_eval.hip) and sdf_step_dev.h (hash_sdf_train.hip).
//
// 16 lanes own one point.  The level columns l * F + k are handed out in adjacent PAIRS (F is even, so a pair lies in one
// level and in one table row): lane c blends pairs c, c + 16, ... - one corner_setup (hashgrid_dev.h: the cell, the eight
// indices and the blend factors are the bits hashgrid_fwd_kernel computes) and eight 8- or 4-byte gathers per pair.  At the
// nglod_hash shape (4 levels x 8 features) every lane has exactly one pair.  There is no occupancy test: a hash grid answers
// everywhere, a coordinate outside the cube is clamped by corner_setup.  The blend is the forward kernel's: fp32 fma chain
// over the corners in corner order, rounded through the table dtype as its store does.  'cat' puts the columns behind the
// position; 'sum' adds the (rounded) levels in level order in fp32 and rounds through the table dtype once, as
// Tensor.sum(-2) does on a half tensor.
//
// The end of the file is HOST code: hash_sdf_fill, the shape and pointer checks that fill a HashSdfField.  It lives here, next to the
// struct it fills, because every entry point over such a field (hash_sdf_eval.hip, hash_sdf_train.hip) runs the same checks.
#pragma once
#include "wisp_common.h"
#include "hashgrid_dev.h"
#include "sdf_decoder_dev.h"

#define HSDF_MAX_COLS 32
#define HSDF_MAX_LODS 16

struct HashSdfField {
    HashLevels lv;
    int64_t begin[HSDF_MAX_LODS + 1];         // first table row of every level, and the number of rows of the whole table
    const void* codebook;                     // MultiTable.feats: [begin[num_lods], feature_dim] of the table dtype
    uint32_t tsize;                           // 2^codebook_bitwidth
    int num_lods, feature_dim, sum, zero_from_col;
    SdfDecoder dec;
};

// floats of LDS per group: the 3 + cols decoder inputs, then ('sum' only) the num_lods * feature_dim level blends
constexpr int hash_sdf_group_floats(int cols, int num_lods, int feature_dim, int sum) {
    return 3 + cols + (sum ? num_lods * feature_dim : 0);
}

// two adjacent features of one table row (the pair is 2 * sizeof(T) aligned: even column of a row of an even number of features)
template <typename T> static __device__ __forceinline__ void hash_sdf_load_pair(const T* p, float& a, float& b);
template <> __device__ __forceinline__ void hash_sdf_load_pair<float>(const float* p, float& a, float& b) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    a = v.x; b = v.y;
}
template <> __device__ __forceinline__ void hash_sdf_load_pair<__half>(const __half* p, float& a, float& b) {
    const __half2 v = *reinterpret_cast<const __half2*>(p);
    a = __half2float(__low2half(v)); b = __half2float(__high2half(v));
}
template <> __device__ __forceinline__ void hash_sdf_load_pair<__hip_bfloat16>(const __hip_bfloat16* p, float& a, float& b) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
    a = __uint_as_float(v << 16); b = __uint_as_float(v & 0xffff0000u);
}

// hash_sdf_point_inputs: the decoder inputs [position, features] of one position into gin[0 .. 3 + cols) (and, for 'sum', the level
// blends behind them).  All 16 lanes of a group call it together, with the same position; c = lane within the group, gin = the
// group's floats of LDS.  Ends with the wave barrier that makes them visible to the group.  Every rounding is spelled out, as in
// sdf_decode: here the bits at stake lie behind the rounding through a half table dtype.
template <typename T>
static __device__ __forceinline__ void hash_sdf_point_inputs(const HashSdfField& fld, float* gin, int c, float px, float py, float pz) {
#pragma clang fp contract(off)
    const float pos[3] = {px, py, pz};
    const int F = fld.feature_dim;
    const int level_cols = fld.num_lods * F;
    float* lev = fld.sum ? gin + 3 + fld.dec.cols : gin + 3;        // 'cat': the level columns ARE the decoder's feature columns
    const T* __restrict__ table = reinterpret_cast<const T*>(fld.codebook);
    __builtin_amdgcn_wave_barrier();                           // the previous evaluation's reads of gin are done
    for (int q = c; 2 * q < level_cols; q += SDF_GROUP) {
        const int col = 2 * q;
        const int l = col / F, k = col - l * F;
        float a0 = 0.0f, a1 = 0.0f;
        if (col < fld.zero_from_col) {                         // (a zeroed column is not gathered)
            CornerSetup<3> cs;
            const bool dense = fld.lv.dense[l] != 0;
            corner_setup<3>(pos, fld.lv.res[l], fld.lv.hi[l], fld.lv.hr[l], dense, fld.tsize, true, cs);
            const int64_t first = fld.begin[l];
            if (dense) {
                // hashgrid_fwd_kernel's pin (its comment: at res >= 258 the fp32 clamp bound rounds up and a corner index can
                // leave the level; below that no index reaches the pin, so it is applied to every dense level here)
                const int64_t last = fld.begin[fld.num_lods] - 1 - first;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if ((int64_t)(uint32_t)cs.idx[j] > last) cs.idx[j] = (int32_t)last;
            }
            float v0[8], v1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) hash_sdf_load_pair<T>(table + (first + (int64_t)(uint32_t)cs.idx[j]) * F + k, v0[j], v1[j]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a0 = __builtin_fmaf(v0[j], cs.coef[j], a0);
                a1 = __builtin_fmaf(v1[j], cs.coef[j], a1);
            }
            a0 = Cvt<T>::to_f(Cvt<T>::from_f(a0));
            a1 = (col + 1 < fld.zero_from_col) ? Cvt<T>::to_f(Cvt<T>::from_f(a1)) : 0.0f;
        }
        lev[col] = a0;
        lev[col + 1] = a1;
    }
    if (c < 3) gin[c] = pos[c];
    __builtin_amdgcn_wave_barrier();                           // the group's lanes are in one wave: LDS order suffices
    if (fld.sum) {
        if (c < F) {
            float acc = 0.0f;
            for (int l = 0; l < fld.num_lods; ++l) acc += lev[l * F + c];
            gin[3 + c] = Cvt<T>::to_f(Cvt<T>::from_f(acc));
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// the encoder policy of the shared kernel bodies (sdf_point_kernels_dev.h, sdf_step_dev.h)
template <typename T> struct HashSdfEnc {
    using Field = HashSdfField;
    static __host__ __device__ int group_floats(const Field& f) { return hash_sdf_group_floats(f.dec.cols, f.num_lods, f.feature_dim, f.sum); }
    static __device__ __forceinline__ void point_inputs(const Field& f, float* gin, int c, float px, float py, float pz) {
        hash_sdf_point_inputs<T>(f, gin, c, px, py, pz);
    }
};

// ---------------------------------------------------------------------------------------------------- host side
// The shape and pointer checks of a hash field, shared by every entry point over it (hash_sdf_eval.hip, hash_sdf_train.hip):
// nothing is dereferenced but the two HOST arrays, and nothing is launched.
static inline int hash_sdf_fill(HashSdfField& fld, const char* fn, const void* codebook, int dtype, const int64_t* begin_idxes,
                         const int32_t* resolutions, int num_lods, int feature_dim, int codebook_bitwidth, int multiscale,
                         int zero_from_col, const float* w1, const float* b1, const float* w2, const float* b2, int hidden) {
#define HSDF_REQUIRE(cond, what) do { if (!(cond)) return wisp_fail(WISP_ERR_INVALID, fn, what); } while (0)
    HSDF_REQUIRE(num_lods >= 1 && num_lods <= HSDF_MAX_LODS, "num_lods out of range (1..16)");
    HSDF_REQUIRE(feature_dim == 2 || feature_dim == 4 || feature_dim == 8, "feature_dim must be 2, 4 or 8");
    HSDF_REQUIRE(multiscale == 0 || multiscale == 1, "multiscale must be 0 ('cat') or 1 ('sum')");
    const int cols = multiscale ? feature_dim : num_lods * feature_dim;
    HSDF_REQUIRE(cols <= HSDF_MAX_COLS, "more than 32 feature columns");
    HSDF_REQUIRE(hidden >= 1 && hidden <= SDF_MAX_HIDDEN, "hidden width out of range");
    HSDF_REQUIRE(codebook_bitwidth >= 1 && codebook_bitwidth <= 30, "codebook_bitwidth out of range");
    HSDF_REQUIRE(zero_from_col >= 0, "zero_from_col is negative");
    HSDF_REQUIRE(dtype == WISP_F32 || dtype == WISP_F16 || dtype == WISP_BF16, "bad dtype");
    HSDF_REQUIRE(codebook && begin_idxes && resolutions && w1 && b1 && w2 && b2, "null pointer");
    const int64_t tsize = (int64_t)1 << codebook_bitwidth;
    HSDF_REQUIRE(fill_levels(resolutions, num_lods, 3, tsize, fld.lv) == 0, "bad resolution");
    // every row a kernel can read lies inside the table: a hashed index is below 2^bitwidth, a dense one is pinned to the last row
    HSDF_REQUIRE(begin_idxes[0] >= 0, "bad begin_idxes");
    for (int l = 0; l < num_lods; ++l) {
        const int64_t rows = begin_idxes[l + 1] - begin_idxes[l];
        HSDF_REQUIRE(rows >= 1 && (fld.lv.dense[l] || rows >= tsize), "a level has fewer rows than its indices reach");
    }
#undef HSDF_REQUIRE
    for (int l = 0; l <= HSDF_MAX_LODS; ++l) fld.begin[l] = begin_idxes[l <= num_lods ? l : num_lods];
    fld.codebook = codebook; fld.tsize = (uint32_t)tsize;
    fld.num_lods = num_lods; fld.feature_dim = feature_dim; fld.sum = multiscale; fld.zero_from_col = zero_from_col;
    fld.dec = SdfDecoder{cols, hidden, w1, b1, w2, b2};
    return WISP_OK;
}
