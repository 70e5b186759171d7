// Evaluation and sphere tracing of a triplanar SDF field (nglod_triplanar.yaml: NeuralSDF over a TriplanarGrid, 'sum', one level
// of three 4 x 33 x 33 planes, raw position in front, one hidden relu layer) for gfx950: the signed distance at arbitrary points
// with the intersection-over-union counters of a validation batch, central-difference normals, and one marching iteration of
// PackedSDFTracer including the field query - one launch each.  The modular path is a wisp_triplane_fwd launch, a cat and a
// decoder launch per query, six queries per normal, and a boolean-mask gather, a scatter and two read-backs per marching
// iteration.  The encoder: triplane_sdf_eval_dev.h; the decoder: sdf_decoder_dev.h; the kernel bodies: sdf_point_kernels_dev.h.
#include "wisp_common.h"
#include "triplane_sdf_eval_dev.h"
#include "sdf_point_kernels_dev.h"

// The bodies are sdf_point_kernels_dev.h's over the triplanar encoder.
__global__ void __launch_bounds__(SDF_POINT_BLOCK)
tri_sdf_point_query_kernel(const float* __restrict__ coords, int64_t n, TriSdfField fld, float* __restrict__ out,
                           const float* __restrict__ gts, unsigned long long* __restrict__ counts) {
    sdf_point_query_body<TriSdfEnc>(coords, n, fld, out, gts, counts);
}

__global__ void __launch_bounds__(SDF_POINT_BLOCK)
tri_sdf_point_gradient_kernel(const float* __restrict__ coords, int64_t n, TriSdfField fld, float eps, float* __restrict__ grad) {
    sdf_point_gradient_body<TriSdfEnc>(coords, n, fld, eps, grad);
}

__global__ void __launch_bounds__(SDF_POINT_BLOCK)
tri_sdf_march_kernel(SphereTraceState st, int first, TriSdfField fld, float scale, int32_t* __restrict__ any_active) {
    sdf_march_body<TriSdfEnc>(st, first, fld, scale, any_active);
}

// ---------------------------------------------------------------------------------------------------- host side
static_assert(sdf_decoder_lds_bytes(SDF_MAX_HIDDEN, TSDF_MAX_COLS, 3 + TSDF_MAX_COLS, SDF_POINT_GROUPS) <= 64 * 1024,
              "the largest shape (hidden 256, 48 columns) must fit the default dynamic LDS limit");

extern "C" int wisp_triplane_sdf_query(const float* coords, int64_t n, const float* const* planes, const int32_t* sizes,
                                       int num_lods, int feature_dim, int multiscale, const float* w1, const float* b1,
                                       const float* w2, const float* b2, int hidden, float* out, const float* gts,
                                       int64_t* counts, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "bad sizes");
    TriSdfField fld;
    if (const int rc = tri_sdf_fill(fld, __func__, planes, sizes, num_lods, feature_dim, multiscale, w1, b1, w2, b2, hidden,
                                    SDF_POINT_GROUPS)) return rc;
    WISP_REQUIRE(!counts || gts, "counts given without gts");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && (out || counts), "null pointer");
    hipLaunchKernelGGL(tri_sdf_point_query_kernel, dim3(sdf_point_grid(n)), dim3(SDF_POINT_BLOCK), sdf_point_lds<TriSdfEnc>(fld), (hipStream_t)stream,
                       coords, n, fld, out, counts ? gts : nullptr, reinterpret_cast<unsigned long long*>(counts));
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_triplane_sdf_fd_gradient(const float* coords, int64_t n, const float* const* planes, const int32_t* sizes,
                                             int num_lods, int feature_dim, int multiscale, const float* w1, const float* b1,
                                             const float* w2, const float* b2, int hidden, float eps, float* grad,
                                             wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "bad sizes");
    TriSdfField fld;
    if (const int rc = tri_sdf_fill(fld, __func__, planes, sizes, num_lods, feature_dim, multiscale, w1, b1, w2, b2, hidden,
                                    SDF_POINT_GROUPS)) return rc;
    WISP_REQUIRE(eps > 0.0f, "eps must be positive");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && grad, "null pointer");
    hipLaunchKernelGGL(tri_sdf_point_gradient_kernel, dim3(sdf_point_grid(n)), dim3(SDF_POINT_BLOCK), sdf_point_lds<TriSdfEnc>(fld),
                       (hipStream_t)stream, coords, n, fld, eps, grad);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_triplane_sdf_trace_step_fused(int64_t num_packs, int first, const float* nug_o, const float* nug_d,
                                                  const float* nug_depth, const int32_t* nug_pidx, float dist_max,
                                                  float thr_close, float thr_avg, float* t, float* dist, float* dist_prev,
                                                  uint8_t* mask, uint8_t* hit, const int32_t* curr_in, int32_t* curr_out,
                                                  int64_t* curr_pidx, float* x, const float* const* planes, const int32_t* sizes,
                                                  int num_lods, int feature_dim, int multiscale, const float* w1, const float* b1,
                                                  const float* w2, const float* b2, int hidden, float scale, int32_t* any_active,
                                                  wisp_stream_t stream) {
    WISP_REQUIRE(num_packs >= 0 && num_packs <= 0x7fffffff, "bad sizes");
    TriSdfField fld;
    if (const int rc = tri_sdf_fill(fld, __func__, planes, sizes, num_lods, feature_dim, multiscale, w1, b1, w2, b2, hidden,
                                    SDF_POINT_GROUPS)) return rc;
    if (num_packs == 0) return WISP_OK;
    const SphereTraceState st{num_packs, nug_o, nug_d, nug_depth, nug_pidx, dist_max, thr_close, thr_avg, t, dist, dist_prev,
                              mask, hit, curr_in, curr_out, curr_pidx, x};
    WISP_REQUIRE(sphere_trace_state_complete(st), "null pointer");
    hipLaunchKernelGGL(tri_sdf_march_kernel, dim3((unsigned)ceil_div64(num_packs, SDF_POINT_GROUPS)), dim3(SDF_POINT_BLOCK), sdf_point_lds<TriSdfEnc>(fld),
                       (hipStream_t)stream, st, first, fld, scale, any_active);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
