// Level arithmetic of the multi-resolution hash / dense grid, shared by every kernel that looks a coordinate up: the forward,
// backward and diagnostic kernels of hashgrid.hip and the fused image render of image_field.hip.  One definition, so the cell, the
// corner indices and the blend factors of a coordinate are the same bits wherever they are computed.
#pragma once
#include "wisp_common.h"

#define HG_MAX_LODS 32

struct HashLevels {
    int32_t res[HG_MAX_LODS];
    int32_t dense[HG_MAX_LODS];
    // per level, computed once on the host (the same IEEE operations the kernels used to repeat per wave and level, three of
    // them in fp64): the float32 clamp bound of hashgrid_interpolate_cuda.cu:40 and res / 2
    float hi[HG_MAX_LODS];
    float hr[HG_MAX_LODS];
};

template <int DIM>
struct CornerSetup {
    int32_t idx[1 << DIM];
    float coef[1 << DIM];
    int32_t cell[DIM];          // integer coordinates of corner 0
    float frac[DIM];            // position inside the cell (read by the diagnostic wisp_hashgrid_cells only)
};

// Position / coefficient / index computation shared by forward and backward.
template <int DIM>
static __device__ __forceinline__ void corner_setup(const float* __restrict__ c, int32_t res, float hi, float hr, bool dense,
                                                    uint32_t tsize, bool tsize_pow2, CornerSetup<DIM>& cs) {
    // hi = (float)((double)(res - 1) - 1e-5): hashgrid_interpolate_cuda.cu:40, clamp bound;  hr = 0.5f * res (exact: res < 2^24)
    int32_t pos[DIM];
    float f[DIM], g[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        // reference (hash_utils.cuh:108-112): float x = res * (c * 0.5 + 0.5) evaluated in double, rounded once to float.
        // res/2 * c + res/2 is exact in double whenever |c| >= 2^-18 (<= 52 significant bits), so ONE fp32 fma - exact
        // product and sum, one rounding - returns the same float; for smaller |c| the two could only differ if the exact
        // value sat within 2^-53 relative of a float rounding midpoint.  Saves four fp64 instructions per axis and level.
        float x = __builtin_fmaf(hr, c[a], hr);
        x = fmaxf(0.0f, fminf(hi, x));
        float p = floorf(x);
        pos[a] = (int32_t)p;
        cs.cell[a] = pos[a];
        f[a] = x - p;
        cs.frac[a] = f[a];
        g[a] = 1.0f - f[a];
    }
    // Per-axis partial terms, shared by the corners: index terms for (pos, pos + 1) - (p + 1) * k == p * k + k in uint32
    // arithmetic, so one multiply per axis serves both - and the blend factors (g, f).
    uint32_t term[DIM][2];
    if (dense) {                                                  // hash_utils.cuh:27-32: x + y * res + z * res * res
        uint32_t mul = 1u;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            term[a][0] = (uint32_t)pos[a] * mul;
            term[a][1] = term[a][0] + mul;
            mul *= (uint32_t)res;
        }
    } else {                                                      // hash_utils.cuh:34-36 (uint32 wrap-around)
        const uint32_t primes[3] = {1u, 2654435761u, 805459861u};
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            term[a][0] = (uint32_t)pos[a] * primes[a];
            term[a][1] = term[a][0] + primes[a];
        }
    }
    if constexpr (DIM == 3) {
        // left-to-right products (.cu:49-56) two at a time: v_pk_mul_f32 does the (x y) pairs and then (xy z0, xy z1) =
        // coefficients j, j + 1 - six packed multiplies instead of twelve scalar ones, same roundings
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 X = {g[0], f[0]}, Z = {g[2], f[2]};
        const f32x2 xy0 = X * g[1], xy1 = X * f[1];              // (bx, by = 0), (bx, by = 1)
        const f32x2 c00 = Z * xy0[0], c01 = Z * xy1[0], c10 = Z * xy0[1], c11 = Z * xy1[1];
        cs.coef[0] = c00[0]; cs.coef[1] = c00[1]; cs.coef[2] = c01[0]; cs.coef[3] = c01[1];
        cs.coef[4] = c10[0]; cs.coef[5] = c10[1]; cs.coef[6] = c11[0]; cs.coef[7] = c11[1];
    } else {
#pragma unroll
        for (int j = 0; j < (1 << DIM); ++j) {
            float w = 1.0f;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const float t = ((j >> (DIM - 1 - a)) & 1) ? f[a] : g[a];
                w = (a == 0) ? t : w * t;                         // left-to-right product, .cu:49-56
            }
            cs.coef[j] = w;
        }
    }
    // the index flavour is uniform for the whole wave: branch once, not per corner
#define HG_CORNER_TERMS(OP)                                                                               \
    _Pragma("unroll") for (int j = 0; j < (1 << DIM); ++j) {                                              \
        uint32_t h = term[0][(j >> (DIM - 1)) & 1];                                                       \
        _Pragma("unroll") for (int a = 1; a < DIM; ++a) h = h OP term[a][(j >> (DIM - 1 - a)) & 1];       \
        hh[j] = h;                                                                                        \
    }
    uint32_t hh[1 << DIM];
    if (dense) {
        HG_CORNER_TERMS(+)
#pragma unroll
        for (int j = 0; j < (1 << DIM); ++j) cs.idx[j] = (int32_t)hh[j];
    } else {
        HG_CORNER_TERMS(^)
        if (tsize_pow2) {
#pragma unroll
            for (int j = 0; j < (1 << DIM); ++j) cs.idx[j] = (int32_t)(hh[j] & (tsize - 1u));
        } else {
#pragma unroll
            for (int j = 0; j < (1 << DIM); ++j) cs.idx[j] = (int32_t)(hh[j] % tsize);
        }
    }
#undef HG_CORNER_TERMS
}

// One level of the lookup on an fp32 table of two features per row (the master table of nerf_hash.yaml), for kernels that fuse the
// lookup with what consumes it (prune_query.hip) - in three steps, so that a caller can have the gathers of several levels in
// flight before it blends the first.
// Dense level with res >= 258: the fp32 clamp bound rounds up to res - 1, so a corner can be `res` and its index can
// leave the level; the reference then reads the next level's rows, and past the allocation on the last level, which is the one
// case refused: the read is pinned to the table's last row (`last` = rows from the level's first row to the table's last one).
template <int DIM>
static __device__ __forceinline__ void corner_pin(CornerSetup<DIM>& cs, int64_t last) {
#pragma unroll
    for (int j = 0; j < (1 << DIM); ++j)
        if ((int64_t)(uint32_t)cs.idx[j] > last) cs.idx[j] = (int32_t)last;
}
template <int DIM>
static __device__ __forceinline__ void corner_gather_f32x2(const float* __restrict__ table, const CornerSetup<DIM>& cs,
                                                           float2 (&v)[1 << DIM]) {
#pragma unroll
    for (int j = 0; j < (1 << DIM); ++j) v[j] = *reinterpret_cast<const float2*>(table + (int64_t)(uint32_t)cs.idx[j] * 2);
}
// the blend, in hashgrid_fwd_kernel's order: acc = fmaf(v_j, coef_j, acc), j = 0 .. 2^DIM - 1, from 0
template <int DIM>
static __device__ __forceinline__ void corner_blend_f32x2(const float2 (&v)[1 << DIM], const CornerSetup<DIM>& cs, float& a0, float& a1) {
    a0 = 0.0f; a1 = 0.0f;
#pragma unroll
    for (int j = 0; j < (1 << DIM); ++j) {
        a0 = __builtin_fmaf(v[j].x, cs.coef[j], a0);
        a1 = __builtin_fmaf(v[j].y, cs.coef[j], a1);
    }
}

// Per-level constants, computed once on the host.
static inline int fill_levels(const int32_t* resolutions, int num_lods, int coord_dim, int64_t tsize, HashLevels& lv) {
    for (int l = 0; l < num_lods; ++l) {
        const int32_t r = resolutions[l];
        if (r < 1) return -1;
        lv.res[l] = r;
        lv.hi[l] = (float)((double)(r - 1) - 1e-5);
        lv.hr[l] = 0.5f * (float)r;
        // hash_utils.cuh:27-29 / :75-76 -- strict '<' on int32 products (wrap-around preserved)
        const int32_t ts = (int32_t)tsize;
        const int32_t r2 = (int32_t)((uint32_t)r * (uint32_t)r);
        const int32_t r3 = (int32_t)((uint32_t)r2 * (uint32_t)r);
        bool dense = (r < ts) && (r2 < ts);
        if (coord_dim == 3) dense = dense && (r3 < ts);
        lv.dense[l] = dense ? 1 : 0;
    }
    for (int l = num_lods; l < HG_MAX_LODS; ++l) { lv.res[l] = 1; lv.dense[l] = 1; lv.hi[l] = 0.0f; lv.hr[l] = 0.5f; }
    return 0;
}
