// Field evaluation of the nglod_triplanar shape as one __device__ function: NeuralSDF over a TriplanarGrid
// (wisp/models/nefs/neural_sdf.py:120-155 over wisp/models/grids/triplanar_grid.py:97-146 and :205-233: per level three bilinear
// F.grid_sample lookups with align_corners=True and reflection padding - plane x with (y, z), plane y with (x, z), plane z with
// (x, y) - stacked as [x | y | z], the levels 'cat'-ed behind one another or 'sum'-med -> [position, features] -> Linear -> relu
// -> Linear).  This file is the ENCODER half, tri_sdf_point_inputs; the decoder is sdf_decoder_dev.h's, and the two
// are put together by the kernel bodies of sdf_point_kernels_dev.h (triplane_sdf_eval.hip) and sdf_step_dev.h
// (triplane_sdf_train.hip).
//
// 16 lanes own one point.  Lane c blends the feature columns c, c + 16, ... (at most three: K <= 48).  A column is one (plane,
// channel) of one level ('cat') or of every level ('sum': the lane adds its column's levels itself in level order in fp32, so
// no level blend is staged in LDS).  The source coordinates are wisp_reflect_source_index's (grid_sample_dev.h), the function
// wisp_triplane_fwd runs; x0 = floor(ix), tx = ix - x0, the four weights (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty as rounded
// products; a corner with x0 + 1 >= size or y0 + 1 >= size is left out; the corners are accumulated 00, 01, 10, 11 as an fma
// chain that starts from the rounded product of corner 00.  The planes are gathered from global memory (the whole pyramid of the
// shipped shape is 52 KB: L2-resident).  Every rounding is spelled out - explicit fmaf, the compiler's own contraction switched off - for the reason recorded at
// sdf_eval_coeffs (sdf_eval_dev.h).  triplane_kernel (spc_interp.hip) leaves its contraction to the compiler, so the two agree
// to rounding, not bit for bit.
//
// The end of the file is HOST code: tri_sdf_fill, the shape and pointer checks that fill a TriSdfField, shared by the entry points
// of both files.
#pragma once
#include "wisp_common.h"
#include "grid_sample_dev.h"
#include "sdf_decoder_dev.h"

#define TSDF_MAX_COLS 48
#define TSDF_MAX_LODS 16

struct TriSdfField {
    const float* planes[TSDF_MAX_LODS * 3];   // x, y, z of level 0, then level 1, ...: each [feature_dim, size, size]
    int32_t size[TSDF_MAX_LODS];
    int num_lods, feature_dim, sum;           // feature_dim per plane
    SdfDecoder dec;
};

// The integer corner and the four weights of one bilinear lookup: channel ch of a [feature_dim, R, R] plane at grid_sample
// coordinates (gx -> width, gy -> height).  Written once for the forward (tri_sdf_blend) and the training step's scatter
// (triplane_sdf_train.hip), so the same bits.  off: the offset of texel (y0, x0) of channel ch inside the plane.
struct TriSdfCorner { int64_t off; float w00, w01, w10, w11; bool vx1, vy1; };
static __device__ __forceinline__ TriSdfCorner tri_sdf_corner(int R, int ch, float gx, float gy) {
#pragma clang fp contract(off)
    const float ix = wisp_reflect_source_index(gx, R), iy = wisp_reflect_source_index(gy, R);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;                      // in [0, R - 1] for every input (grid_sample_dev.h)
    const float tx = ix - fx, ty = iy - fy;
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    TriSdfCorner k;
    k.w00 = ux * uy; k.w01 = tx * uy; k.w10 = ux * ty; k.w11 = tx * ty;
    k.vx1 = x0 + 1 < R; k.vy1 = y0 + 1 < R;
    k.off = (int64_t)ch * R * R + (int64_t)y0 * R + x0;
    return k;
}

// the lookup itself: a corner with x0 + 1 >= R or y0 + 1 >= R is left out
static __device__ __forceinline__ float tri_sdf_blend(const float* __restrict__ plane, int R, int ch, float gx, float gy) {
#pragma clang fp contract(off)
    const TriSdfCorner k = tri_sdf_corner(R, ch, gx, gy);
    const float* fm = plane + k.off;
    const float f00 = fm[0];
    const float f01 = k.vx1 ? fm[1] : 0.0f;
    const float f10 = k.vy1 ? fm[R] : 0.0f;
    const float f11 = (k.vx1 && k.vy1) ? fm[(int64_t)R + 1] : 0.0f;
    float v = f00 * k.w00;
    if (k.vx1) v = __builtin_fmaf(f01, k.w01, v);
    if (k.vy1) v = __builtin_fmaf(f10, k.w10, v);
    if (k.vx1 && k.vy1) v = __builtin_fmaf(f11, k.w11, v);
    return v;
}

// tri_sdf_point_inputs: the decoder inputs [position, features] of one position into gin[0 .. 3 + cols).  All 16 lanes of a group
// call it together, with the same position; c = lane within the group.  Ends with the wave barrier that makes them visible to the
// group.
static __device__ __forceinline__ void tri_sdf_point_inputs(const TriSdfField& fld, float* gin, int c, float px, float py, float pz) {
#pragma clang fp contract(off)
    const int F = fld.feature_dim, F3 = 3 * F;
    __builtin_amdgcn_wave_barrier();                           // the previous evaluation's reads of gin are done
    for (int j = c; j < fld.dec.cols; j += SDF_GROUP) {
        const int l0 = fld.sum ? 0 : j / F3, l1 = fld.sum ? fld.num_lods : l0 + 1;
        const int rem = j - (fld.sum ? 0 : l0 * F3);
        const int p = rem / F, ch = rem - p * F;
        const float gx = p == 0 ? py : px;                     // grid[..., 0] -> width:  x-plane y, y-plane x, z-plane x
        const float gy = p == 2 ? py : pz;                     // grid[..., 1] -> height: x-plane z, y-plane z, z-plane y
        float acc = 0.0f;
        for (int l = l0; l < l1; ++l) acc += tri_sdf_blend(fld.planes[l * 3 + p], fld.size[l], ch, gx, gy);
        gin[3 + j] = acc;
    }
    if (c < 3) gin[c] = c == 0 ? px : c == 1 ? py : pz;
    __builtin_amdgcn_wave_barrier();                           // the group's lanes are in one wave: LDS order suffices
}

// the encoder policy of the shared kernel bodies (sdf_point_kernels_dev.h, sdf_step_dev.h); a group's LDS holds the decoder
// inputs only
struct TriSdfEnc {
    using Field = TriSdfField;
    static __host__ __device__ int group_floats(const Field& f) { return 3 + f.dec.cols; }
    static __device__ __forceinline__ void point_inputs(const Field& f, float* gin, int c, float px, float py, float pz) {
        tri_sdf_point_inputs(f, gin, c, px, py, pz);
    }
};

// ---------------------------------------------------------------------------------------------------- host side
// The shape and pointer checks of a triplanar field, shared by the three entry points: nothing is dereferenced but the two HOST
// arrays, and nothing is launched.  `groups`: points per block (the LDS budget is part of the shape).
static inline int tri_sdf_fill(TriSdfField& fld, const char* fn, const float* const* planes, const int32_t* sizes, int num_lods,
                               int feature_dim, int multiscale, const float* w1, const float* b1, const float* w2, const float* b2,
                               int hidden, int groups) {
#define TSDF_REQUIRE(cond, what) do { if (!(cond)) return wisp_fail(WISP_ERR_INVALID, fn, what); } while (0)
    TSDF_REQUIRE(num_lods >= 1 && num_lods <= TSDF_MAX_LODS, "num_lods out of range (1..16)");
    TSDF_REQUIRE(feature_dim >= 1, "feature_dim must be at least 1");
    TSDF_REQUIRE(multiscale == 0 || multiscale == 1, "multiscale must be 0 ('cat') or 1 ('sum')");
    const int64_t cols = (int64_t)(multiscale ? 1 : num_lods) * 3 * feature_dim;
    TSDF_REQUIRE(cols <= TSDF_MAX_COLS, "more than 48 feature columns");
    TSDF_REQUIRE(hidden >= 1 && hidden <= SDF_MAX_HIDDEN, "hidden width out of range");
    TSDF_REQUIRE(planes && sizes && w1 && b1 && w2 && b2, "null pointer");
    for (int l = 0; l < num_lods; ++l) {
        TSDF_REQUIRE(sizes[l] >= 1, "bad plane size");
        for (int p = 0; p < 3; ++p) TSDF_REQUIRE(planes[l * 3 + p], "null plane pointer");
    }
    TSDF_REQUIRE(sdf_decoder_lds_bytes(hidden, (int)cols, 3 + (int)cols, groups) <= 64 * 1024, "LDS budget exceeded");
#undef TSDF_REQUIRE
    for (int k = 0; k < TSDF_MAX_LODS * 3; ++k) fld.planes[k] = k < num_lods * 3 ? planes[k] : nullptr;
    for (int l = 0; l < TSDF_MAX_LODS; ++l) fld.size[l] = l < num_lods ? sizes[l] : 1;
    fld.num_lods = num_lods; fld.feature_dim = feature_dim; fld.sum = multiscale;
    fld.dec = SdfDecoder{(int)cols, hidden, w1, b1, w2, b2};
    return WISP_OK;
}
