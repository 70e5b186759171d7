// Evaluation and sphere tracing of a hash-grid SDF field (nglod_hash.yaml: NeuralSDF over HashGrid.from_geometric, 'cat',
// 4 levels x 8 features, raw position in front, one hidden relu layer) for gfx950: the signed distance at arbitrary points with
// the intersection-over-union counters of a validation batch, central-difference normals, and one marching iteration of
// PackedSDFTracer including the field query - one launch each.  The modular path is a boolean-mask gather, a hashgrid launch,
// two library GEMMs, a scatter and a read-back per marching iteration, and six field queries per normal.  The encoder:
// hash_sdf_eval_dev.h; the decoder: sdf_decoder_dev.h; the kernel bodies: sdf_point_kernels_dev.h.
#include "wisp_common.h"
#include "hash_sdf_eval_dev.h"
#include "sdf_point_kernels_dev.h"

// The bodies are sdf_point_kernels_dev.h's over the hash encoder; T is the table dtype.
template <typename T>
__global__ void __launch_bounds__(SDF_POINT_BLOCK)
hash_sdf_point_query_kernel(const float* __restrict__ coords, int64_t n, HashSdfField fld, float* __restrict__ out,
                      const float* __restrict__ gts, unsigned long long* __restrict__ counts) {
    sdf_point_query_body<HashSdfEnc<T>>(coords, n, fld, out, gts, counts);
}

template <typename T>
__global__ void __launch_bounds__(SDF_POINT_BLOCK)
hash_sdf_point_gradient_kernel(const float* __restrict__ coords, int64_t n, HashSdfField fld, float eps, float* __restrict__ grad) {
    sdf_point_gradient_body<HashSdfEnc<T>>(coords, n, fld, eps, grad);
}

template <typename T>
__global__ void __launch_bounds__(SDF_POINT_BLOCK)
hash_sdf_march_kernel(SphereTraceState st, int first, HashSdfField fld, float scale, int32_t* __restrict__ any_active) {
    sdf_march_body<HashSdfEnc<T>>(st, first, fld, scale, any_active);
}

// ---------------------------------------------------------------------------------------------------- host side
// (the LDS of a launch does not depend on the table dtype: the entry points size it through HashSdfEnc<float> for all three)
static_assert(sdf_decoder_lds_bytes(SDF_MAX_HIDDEN, HSDF_MAX_COLS, hash_sdf_group_floats(HSDF_MAX_COLS, HSDF_MAX_LODS, 8, 1),
                                    SDF_POINT_GROUPS) <= 64 * 1024,
              "the largest shape (hidden 256, 32 columns, 'sum' of 16 levels x 8) must fit the default dynamic LDS limit");
static_assert(HSDF_MAX_LODS <= HG_MAX_LODS, "HashLevels holds the levels");

#define HSDF_DISPATCH(LAUNCH)                                                                                                        \
    do { if (feats_dtype == WISP_F32) LAUNCH(float); else if (feats_dtype == WISP_F16) LAUNCH(__half); else LAUNCH(__hip_bfloat16); } while (0)

extern "C" int wisp_hash_sdf_query(const float* coords, int64_t n, const void* codebook, int feats_dtype, const int64_t* begin_idxes,
                                   const int32_t* resolutions, int num_lods, int feature_dim, int codebook_bitwidth,
                                   int multiscale, int zero_from_col, const float* w1, const float* b1, const float* w2,
                                   const float* b2, int hidden, float* out, const float* gts, int64_t* counts,
                                   wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "bad sizes");
    HashSdfField fld;
    if (const int rc = hash_sdf_fill(fld, __func__, codebook, feats_dtype, begin_idxes, resolutions, num_lods, feature_dim,
                                     codebook_bitwidth, multiscale, zero_from_col, w1, b1, w2, b2, hidden)) return rc;
    WISP_REQUIRE(!counts || gts, "counts given without gts");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && (out || counts), "null pointer");
    const size_t lds = sdf_point_lds<HashSdfEnc<float>>(fld);
    WISP_REQUIRE(lds <= 64 * 1024, "LDS budget exceeded");
    const dim3 grid(sdf_point_grid(n)), block(SDF_POINT_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
#define HSDF_Q(T) hipLaunchKernelGGL((hash_sdf_point_query_kernel<T>), grid, block, lds, s, coords, n, fld, out, counts ? gts : nullptr, cnt)
    HSDF_DISPATCH(HSDF_Q);
#undef HSDF_Q
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_hash_sdf_fd_gradient(const float* coords, int64_t n, const void* codebook, int feats_dtype,
                                         const int64_t* begin_idxes, const int32_t* resolutions, int num_lods, int feature_dim,
                                         int codebook_bitwidth, int multiscale, int zero_from_col, const float* w1,
                                         const float* b1, const float* w2, const float* b2, int hidden, float eps, float* grad,
                                         wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "bad sizes");
    HashSdfField fld;
    if (const int rc = hash_sdf_fill(fld, __func__, codebook, feats_dtype, begin_idxes, resolutions, num_lods, feature_dim,
                                     codebook_bitwidth, multiscale, zero_from_col, w1, b1, w2, b2, hidden)) return rc;
    WISP_REQUIRE(eps > 0.0f, "eps must be positive");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && grad, "null pointer");
    const size_t lds = sdf_point_lds<HashSdfEnc<float>>(fld);
    WISP_REQUIRE(lds <= 64 * 1024, "LDS budget exceeded");
    const dim3 grid(sdf_point_grid(n)), block(SDF_POINT_BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define HSDF_G(T) hipLaunchKernelGGL((hash_sdf_point_gradient_kernel<T>), grid, block, lds, s, coords, n, fld, eps, grad)
    HSDF_DISPATCH(HSDF_G);
#undef HSDF_G
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_hash_sdf_trace_step_fused(int64_t num_packs, int first, const float* nug_o, const float* nug_d,
                                              const float* nug_depth, const int32_t* nug_pidx, float dist_max, float thr_close,
                                              float thr_avg, float* t, float* dist, float* dist_prev, uint8_t* mask, uint8_t* hit,
                                              const int32_t* curr_in, int32_t* curr_out, int64_t* curr_pidx, float* x,
                                              const void* codebook, int feats_dtype, const int64_t* begin_idxes,
                                              const int32_t* resolutions, int num_lods, int feature_dim, int codebook_bitwidth,
                                              int multiscale, int zero_from_col, const float* w1, const float* b1, const float* w2,
                                              const float* b2, int hidden, float scale, int32_t* any_active, wisp_stream_t stream) {
    WISP_REQUIRE(num_packs >= 0 && num_packs <= 0x7fffffff, "bad sizes");
    HashSdfField fld;
    if (const int rc = hash_sdf_fill(fld, __func__, codebook, feats_dtype, begin_idxes, resolutions, num_lods, feature_dim,
                                     codebook_bitwidth, multiscale, zero_from_col, w1, b1, w2, b2, hidden)) return rc;
    if (num_packs == 0) return WISP_OK;
    const SphereTraceState st{num_packs, nug_o, nug_d, nug_depth, nug_pidx, dist_max, thr_close, thr_avg, t, dist, dist_prev,
                              mask, hit, curr_in, curr_out, curr_pidx, x};
    WISP_REQUIRE(sphere_trace_state_complete(st), "null pointer");
    const size_t lds = sdf_point_lds<HashSdfEnc<float>>(fld);
    WISP_REQUIRE(lds <= 64 * 1024, "LDS budget exceeded");
    const dim3 grid((unsigned)ceil_div64(num_packs, SDF_POINT_GROUPS)), block(SDF_POINT_BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define HSDF_T(T) hipLaunchKernelGGL((hash_sdf_march_kernel<T>), grid, block, lds, s, st, first, fld, scale, any_active)
    HSDF_DISPATCH(HSDF_T);
#undef HSDF_T
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
