// The encoder of an octree-backed radiance field (OctreeGrid.interpolate, wisp/models/grids/octree_grid.py:165-219) for one
// sample and one lane: the walk from the root to the finest listed level, the trilinear blend of the eight corner rows on every
// listed level, and the 'sum' or 'cat' decoder input written into the lane's row of an LDS tile.  No chain tensor, no feature
// tensor.
//
// Cells are those of spc_query_kernel (csrc/spc.hip), the weights are sdf_eval_coeffs (sdf_eval_dev.h, the spelling of
// trilinear_coeffs under contraction), the blend is the fmaf chain over corners 0..7 and the level sum runs in ascending level
// order from 0.0f: the bits of spc_trilinear_multi_fwd.  A position outside [-1,1]^3 (or NaN), or one in an unoccupied cell,
// contributes zeros from there on.
#pragma once
#include "wisp_common.h"
#include "sdf_eval_dev.h"

#define ONE_MAX_LODS 16
#define ONE_MAX_FEATURES 16
#define ONE_CHUNK 4                              // channels blended together: 8 x 4 gathers in flight per lane

struct OctreeNerfField {
    const void* feats[ONE_MAX_LODS];
    int32_t level[ONE_MAX_LODS];
    int num_lods, feature_dim, half_round, sum;
    const uint8_t* octree;
    const int32_t* exsum;
    const int16_t* points;
    const int32_t* trinkets;
};

// row: the lane's `width` floats of LDS (the decoder's padded input row); every entry is written.  live = false: a lane past the
// last sample, it writes zeros and reads nothing.
template <typename T>
static __device__ __forceinline__ void octree_nerf_encode(const OctreeNerfField& fld, bool live, float px, float py, float pz,
                                                          float* row, int width) {
#pragma clang fp contract(off)
    for (int k = 0; k < width; ++k) row[k] = 0.0f;
    const int L = fld.level[fld.num_lods - 1];
    const int F = fld.feature_dim;
    const bool inside = live && (fabsf(px) <= 1.0f) && (fabsf(py) <= 1.0f) && (fabsf(pz) <= 1.0f);
    const float res = (float)(1 << L);
    const int top = (1 << L) - 1;
    // (the cell only of a point inside the cube: far-outside or NaN coordinates never reach the float -> int conversion)
    const int qx = inside ? min((int)floorf(res * __builtin_fmaf(0.5f, px, 0.5f)), top) : 0;
    const int qy = inside ? min((int)floorf(res * __builtin_fmaf(0.5f, py, 0.5f)), top) : 0;
    const int qz = inside ? min((int)floorf(res * __builtin_fmaf(0.5f, pz, 0.5f)), top) : 0;
    const float pos[3] = {px, py, pz};
    int64_t node = inside ? 0 : -1;
    int li = 0;
    for (int l = 0; l <= L; ++l) {
        if (l == fld.level[li]) {
            float w[8];
            int32_t tr[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { w[j] = 0.0f; tr[j] = 0; }
            if (node >= 0) {
                sdf_eval_coeffs(pos, fld.points + node * 3, l, w);
                const int4* t4 = reinterpret_cast<const int4*>(fld.trinkets + node * 8);      // 32-byte rows of an aligned tensor
                const int4 ta = t4[0], tb = t4[1];
                tr[0] = ta.x; tr[1] = ta.y; tr[2] = ta.z; tr[3] = ta.w; tr[4] = tb.x; tr[5] = tb.y; tr[6] = tb.z; tr[7] = tb.w;
            }
            const T* f = reinterpret_cast<const T*>(fld.feats[li]);
            float* dst = fld.sum ? row : row + li * F;
            for (int c0 = 0; c0 < F; c0 += ONE_CHUNK) {
                float acc[ONE_CHUNK];
#pragma unroll
                for (int c = 0; c < ONE_CHUNK; ++c) acc[c] = 0.0f;
                if (node >= 0) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const T* r = f + (int64_t)tr[j] * F + c0;
#pragma unroll
                        for (int c = 0; c < ONE_CHUNK; ++c) {
                            if (c0 + c < F) {
                                float fv = Cvt<T>::to_f(r[c]);
                                if (fld.half_round) fv = __half2float(__float2half_rn(fv));
                                acc[c] = __builtin_fmaf(fv, w[j], acc[c]);
                            }
                        }
                    }
                    if (fld.half_round) {
#pragma unroll
                        for (int c = 0; c < ONE_CHUNK; ++c) acc[c] = wisp_round_through_f16(acc[c]);
                    }
                }
#pragma unroll
                for (int c = 0; c < ONE_CHUNK; ++c) {
                    if (c0 + c < F) {
                        if (fld.sum) dst[c0 + c] = dst[c0 + c] + acc[c]; else dst[c0 + c] = acc[c];
                    }
                }
            }
            ++li;
        }
        if (l < L && node >= 0) {
            const int sh = L - 1 - l;
            const int cs = (((qx >> sh) & 1) << 2) | (((qy >> sh) & 1) << 1) | ((qz >> sh) & 1);
            const uint32_t bits = fld.octree[node];
            node = ((bits >> cs) & 1u) ? (int64_t)fld.exsum[node] + __popc(bits & ((2u << cs) - 1u)) : -1;
        }
    }
}
