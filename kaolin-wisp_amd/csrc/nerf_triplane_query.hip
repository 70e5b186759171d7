// The inference query of a triplanar radiance field - nerf_triplanar.yaml (NeuralRadianceField over a TriplanarGrid) - as ONE
// launch: NeuralRadianceField.rgba (wisp/models/nefs/nerf.py:219-264) over TriplanarGrid.interpolate
// (wisp/models/grids/triplanar_grid.py:97-146 and :205-233).
//
// The modular path runs, per chunk of samples: an index_select of the ray directions, wisp_triplane_fwd (one thread per sample
// that, for 'sum', read-modify-writes its output row in global memory once per level) into a feature tensor, and the exact-fp32
// decoder.  Here a wave takes 64 samples (the kernel of nerf_field_query_dev.h): every lane blends the three planes of every level
// for its own sample straight into the decoder's input tile in the wave's LDS slice, and the tile's two halves of 32 samples run
// all five layers on the matrix cores.  The encoder arithmetic is tri_sdf_blend's (triplane_sdf_eval_dev.h), every rounding
// spelled out and the compiler's contraction off, so a feature row is the bits the triplanar SDF kernels produce for the same
// planes and position; triplane_kernel (spc_interp.hip) leaves its contraction to the compiler, so the modular lookup agrees to
// rounding.  The decoder is the shared MFMA sequence: the bits of wisp_nerf_mlp_fwd with WISP_F32 compute on the same rows.
#include "wisp_common.h"
#include "triplane_sdf_eval_dev.h"
#include "nerf_field_query_dev.h"

namespace {

constexpr int TNQ_CHUNK = 4;              // channels of one (level, plane) blended together: their 16 loads are independent

struct TriNerfField {
    const float* planes[TSDF_MAX_LODS * 3];   // x, y, z of level 0, then level 1, ...: each [feature_dim, size, size]
    int32_t size[TSDF_MAX_LODS];
    int num_lods, feature_dim, sum;           // feature_dim per plane
};

// One lane per sample.  Column p * F + ch ('sum') or l * 3 F + p * F + ch ('cat') is plane p (x: (y, z), y: (x, z), z: (x, y);
// grid[..., 0] indexes the width), channel ch; 'sum' adds a column's levels in level order in fp32 starting from +0.0f, as
// tri_sdf_point_inputs does.  The source coordinates and the four weights of a (level, plane) do not depend on the channel: the
// TNQ_CHUNK calls of tri_sdf_blend in the unrolled loop share them.  wisp_reflect_source_index returns a coordinate inside the
// plane for every input, NaN and +-inf included, so no position reads out of bounds.
struct TriNerfEnc {
    using Field = TriNerfField;
    static __device__ __forceinline__ void encode(const Field& fld, bool live, float px, float py, float pz, float* row, int width) {
#pragma clang fp contract(off)
        for (int k = 0; k < width; ++k) row[k] = 0.0f;
        if (!live) return;
        const int F = fld.feature_dim, L = fld.num_lods;
        for (int p = 0; p < 3; ++p) {
            const float gx = p == 0 ? py : px;                 // grid[..., 0] -> width:  x-plane y, y-plane x, z-plane x
            const float gy = p == 2 ? py : pz;                 // grid[..., 1] -> height: x-plane z, y-plane z, z-plane y
            for (int c0 = 0; c0 < F; c0 += TNQ_CHUNK) {
                float acc[TNQ_CHUNK];
#pragma unroll
                for (int c = 0; c < TNQ_CHUNK; ++c) acc[c] = 0.0f;
                for (int l = 0; l < L; ++l) {
                    const float* plane = fld.planes[l * 3 + p];
                    const int R = fld.size[l];
#pragma unroll
                    for (int c = 0; c < TNQ_CHUNK; ++c)
                        if (c0 + c < F) acc[c] += tri_sdf_blend(plane, R, c0 + c, gx, gy);
                    if (!fld.sum || l == L - 1) {
                        float* dst = row + (fld.sum ? 0 : l * 3 * F) + p * F + c0;
#pragma unroll
                        for (int c = 0; c < TNQ_CHUNK; ++c) {
                            if (c0 + c < F) dst[c] = acc[c];
                            acc[c] = 0.0f;
                        }
                    }
                }
            }
        }
    }
};

}  // namespace

extern "C" int wisp_nerf_triplane_query(const float* coords, const float* dirs, const int64_t* ridx, int64_t num_rays, int64_t n,
                                        const float* const* planes, const int32_t* sizes, int num_lods, int feature_dim, int sum,
                                        const float* params, int dtype_params, int in_dim, int hidden, float* rgb, float* density,
                                        float* feats_out, wisp_stream_t stream) {
    using namespace wisp_nfq;
    WISP_REQUIRE(n >= 0, "negative sample count");
    bool shape_ok = num_lods >= 1 && num_lods <= TSDF_MAX_LODS && feature_dim >= 1 && feature_dim <= IN && hidden == H &&
                    dtype_params == WISP_F32 && in_dim <= IN &&
                    (int64_t)in_dim == (int64_t)(sum ? 1 : num_lods) * 3 * feature_dim;
    if (shape_ok && sizes)
        for (int l = 0; l < num_lods; ++l) shape_ok = shape_ok && sizes[l] >= 1;
    if (!shape_ok)
        return wisp_fail(WISP_ERR_UNSUPPORTED, "nerf_triplane_query",
                         "this build supports 1..16 levels of f32 planes of size >= 1, feature_dim >= 1 per plane, hidden 64, in_dim = "
                         "3 * feature_dim ('sum') or levels * 3 * feature_dim ('cat') <= 32 and fp32 parameters");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && planes && sizes && params && (rgb || density), "null pointer");
    WISP_REQUIRE(!rgb || dirs, "null pointer");                                   // the colour needs a view direction
    WISP_REQUIRE(!ridx || (dirs && num_rays >= 1), "ridx needs ray_dirs with at least one ray");
    TriNerfField fld;
    for (int k = 0; k < TSDF_MAX_LODS * 3; ++k) fld.planes[k] = nullptr;
    for (int l = 0; l < TSDF_MAX_LODS; ++l) fld.size[l] = 1;
    for (int l = 0; l < num_lods; ++l) {
        fld.size[l] = sizes[l];
        for (int p = 0; p < 3; ++p) {
            WISP_REQUIRE(planes[l * 3 + p], "null plane pointer");
            fld.planes[l * 3 + p] = planes[l * 3 + p];
        }
    }
    fld.num_lods = num_lods; fld.feature_dim = feature_dim; fld.sum = sum ? 1 : 0;
    return nerf_field_query_launch<TriNerfEnc>("nerf_triplane_query", coords, dirs, ridx, num_rays, n, fld, in_dim, params, rgb, density,
                                               feats_out, (hipStream_t)stream);
}
