// Field evaluation of the nglod_triplanar shape as one __device__ function: NeuralSDF over a TriplanarGrid
// (wisp/models/nefs/neural_sdf.py:120-155 over wisp/models/grids/triplanar_grid.py:97-146 and :205-233: per level three bilinear
// F.grid_sample lookups with align_corners=True and reflection padding - plane x with (y, z), plane y with (x, z), plane z with
// (x, y) - stacked as [x | y | z], the levels 'cat'-ed behind one another or 'sum'-med -> [position, features] -> Linear -> relu
// -> Linear).  The triplanar twin of hash_sdf_eval_point (hash_sdf_eval_dev.h); shared by the three kernels of
// triplane_sdf_eval.hip and the training step of triplane_sdf_train.hip, so that a value the gradient kernel differences, a
// distance the marching kernel steps by and a prediction the training step takes its loss from are bit for bit what the query
// kernel returns for the same position.
//
// 16 lanes own one point.  Lane c blends the feature columns c, c + 16, ... (at most three: K <= 48).  A column is one (plane,
// channel) of one level ('cat') or of every level ('sum': the lane adds its column's levels itself in level order in fp32, so
// no level blend is staged in LDS).  The source coordinates are wisp_reflect_source_index's (grid_sample_dev.h), the function
// wisp_triplane_fwd runs; x0 = floor(ix), tx = ix - x0, the four weights (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty as rounded
// products; a corner with x0 + 1 >= size or y0 + 1 >= size is left out; the corners are accumulated 00, 01, 10, 11 as an fma
// chain that starts from the rounded product of corner 00.  The planes are gathered from global memory (the whole pyramid of the
// shipped shape is 52 KB: L2-resident).  The decoder is that of hash_sdf_decode: hidden layer split over the lanes (weights in
// LDS, odd row stride), fp32 fma chain in input order, the output dot product reduced with four shuffles of width 16, b2 last.
// Every rounding is spelled out - explicit fmaf, the compiler's own contraction switched off - for the reason recorded at
// sdf_eval_coeffs (sdf_eval_dev.h).  triplane_kernel (spc_interp.hip) leaves its contraction to the compiler, so the two agree
// to rounding, not bit for bit.
//
// The end of the file is HOST code: tri_sdf_fill, the shape and pointer checks that fill a TriSdfField, shared by the entry points
// of both files.
#pragma once
#include "wisp_common.h"
#include "grid_sample_dev.h"

#define TSDF_GROUP 16
#define TSDF_MAX_COLS 48
#define TSDF_MAX_HIDDEN 256
#define TSDF_MAX_LODS 16

struct TriSdfField {
    const float* planes[TSDF_MAX_LODS * 3];   // x, y, z of level 0, then level 1, ...: each [feature_dim, size, size]
    int32_t size[TSDF_MAX_LODS];
    int num_lods, feature_dim, sum, cols, hidden;                     // feature_dim per plane; cols = decoder feature columns K
    const float *w1, *b1, *w2, *b2;           // [hidden, 3 + cols], [hidden], [hidden], [1]
};

// LDS of a block: W1 [hidden][in_pad], b1 [hidden], w2 [hidden] | per group: the 3 + cols decoder inputs
struct TriSdfLds { float *w1, *b1, *w2, *in; int in_pad, stride; };

static inline int tri_sdf_in_pad(int cols) { return (3 + cols) | 1; }            // odd row stride: the lanes of a group read different rows
static inline size_t tri_sdf_lds_bytes(int hidden, int cols, int groups) {
    return ((size_t)hidden * tri_sdf_in_pad(cols) + 2 * (size_t)hidden + (size_t)groups * (3 + cols)) * sizeof(float);
}

// every thread of the block; ends with the block barrier
static __device__ __forceinline__ TriSdfLds tri_sdf_stage(float* base, const TriSdfField& fld) {
    TriSdfLds s;
    const int in_dim = 3 + fld.cols;
    s.in_pad = in_dim | 1;
    s.stride = in_dim;
    s.w1 = base;
    s.b1 = s.w1 + fld.hidden * s.in_pad;
    s.w2 = s.b1 + fld.hidden;
    s.in = s.w2 + fld.hidden;
    for (int e = threadIdx.x; e < fld.hidden * in_dim; e += blockDim.x) s.w1[(e / in_dim) * s.in_pad + e % in_dim] = fld.w1[e];
    for (int e = threadIdx.x; e < fld.hidden; e += blockDim.x) { s.b1[e] = fld.b1[e]; s.w2[e] = fld.w2[e]; }
    __syncthreads();
    return s;
}

// one bilinear lookup: channel ch of a [feature_dim, R, R] plane at grid_sample coordinates (gx -> width, gy -> height)
static __device__ __forceinline__ float tri_sdf_blend(const float* __restrict__ plane, int R, int ch, float gx, float gy) {
#pragma clang fp contract(off)
    const float ix = wisp_reflect_source_index(gx, R), iy = wisp_reflect_source_index(gy, R);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;                      // in [0, R - 1] for every input (grid_sample_dev.h)
    const float tx = ix - fx, ty = iy - fy;
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    const float w00 = ux * uy, w01 = tx * uy, w10 = ux * ty, w11 = tx * ty;
    const bool vx1 = x0 + 1 < R, vy1 = y0 + 1 < R;
    const float* fm = plane + (int64_t)ch * R * R + (int64_t)y0 * R + x0;
    const float f00 = fm[0];
    const float f01 = vx1 ? fm[1] : 0.0f;
    const float f10 = vy1 ? fm[R] : 0.0f;
    const float f11 = (vx1 && vy1) ? fm[(int64_t)R + 1] : 0.0f;
    float v = f00 * w00;
    if (vx1) v = __builtin_fmaf(f01, w01, v);
    if (vy1) v = __builtin_fmaf(f10, w10, v);
    if (vx1 && vy1) v = __builtin_fmaf(f11, w11, v);
    return v;
}

// The integer corner and the four weights of that lookup, for the training step's scatter (triplane_sdf_train.hip): the statements
// of tri_sdf_blend, so the same bits.  off: the offset of texel (y0, x0) of channel ch inside the plane.
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

// tri_sdf_point_inputs: the decoder inputs [position, features] of one position into gin[0 .. 3 + cols).  All 16 lanes of a group
// call it together, with the same position; c = lane within the group.  Ends with the wave barrier that makes them visible to the
// group.
static __device__ __forceinline__ void tri_sdf_point_inputs(const TriSdfField& fld, float* gin, int c, float px, float py, float pz) {
#pragma clang fp contract(off)
    const int F = fld.feature_dim, F3 = 3 * F;
    __builtin_amdgcn_wave_barrier();                           // the previous evaluation's reads of gin are done
    for (int j = c; j < fld.cols; j += TSDF_GROUP) {
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

// tri_sdf_decode: the decoder over gin, in = [position, features]; returns the raw output with the bias added (hash_sdf_decode's
// statements).  KEEP (the training step): lane c also leaves, for its hidden units hh = c, c + 16, ..., w2[hh] where the unit is
// active (0 elsewhere) in ga[hh] and the unit's relu output in gr[hh] - stores only, the arithmetic is the same statements.
template <bool KEEP = false>
static __device__ __forceinline__ float tri_sdf_decode(const TriSdfField& fld, const TriSdfLds& s, const float* gin, int c,
                                                       float* ga = nullptr, float* gr = nullptr) {
#pragma clang fp contract(off)
    const int in_dim = 3 + fld.cols;
    float o = 0.0f;
    for (int hh = c; hh < fld.hidden; hh += TSDF_GROUP) {
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
    for (int d = TSDF_GROUP / 2; d >= 1; d >>= 1) o += __shfl_xor(o, d, TSDF_GROUP);
    return o + fld.b2[0];
}

// A group either runs the whole function or none of it (the shuffles stay inside the group).
static __device__ __forceinline__ float tri_sdf_eval_point(const TriSdfField& fld, const TriSdfLds& s, float* gin, int c,
                                                           float px, float py, float pz) {
    tri_sdf_point_inputs(fld, gin, c, px, py, pz);
    return tri_sdf_decode(fld, s, gin, c);
}

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
    TSDF_REQUIRE(hidden >= 1 && hidden <= TSDF_MAX_HIDDEN, "hidden width out of range");
    TSDF_REQUIRE(planes && sizes && w1 && b1 && w2 && b2, "null pointer");
    for (int l = 0; l < num_lods; ++l) {
        TSDF_REQUIRE(sizes[l] >= 1, "bad plane size");
        for (int p = 0; p < 3; ++p) TSDF_REQUIRE(planes[l * 3 + p], "null plane pointer");
    }
    TSDF_REQUIRE(tri_sdf_lds_bytes(hidden, (int)cols, groups) <= 64 * 1024, "LDS budget exceeded");
#undef TSDF_REQUIRE
    for (int k = 0; k < TSDF_MAX_LODS * 3; ++k) fld.planes[k] = k < num_lods * 3 ? planes[k] : nullptr;
    for (int l = 0; l < TSDF_MAX_LODS; ++l) fld.size[l] = l < num_lods ? sizes[l] : 1;
    fld.num_lods = num_lods; fld.feature_dim = feature_dim; fld.sum = multiscale; fld.cols = (int)cols; fld.hidden = hidden;
    fld.w1 = w1; fld.b1 = b1; fld.w2 = w2; fld.b2 = b2;
    return WISP_OK;
}
