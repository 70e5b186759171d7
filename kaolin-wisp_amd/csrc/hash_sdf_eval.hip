// Evaluation and sphere tracing of a hash-grid SDF field (nglod_hash.yaml: NeuralSDF over HashGrid.from_geometric, 'cat',
// 4 levels x 8 features, raw position in front, one hidden relu layer) for gfx950: the signed distance at arbitrary points with
// the intersection-over-union counters of a validation batch, central-difference normals, and one marching iteration of
// PackedSDFTracer including the field query - one launch each.  The modular path is a boolean-mask gather, a hashgrid launch,
// two library GEMMs, a scatter and a read-back per marching iteration, and six field queries per normal.  Field evaluation:
// hash_sdf_eval_dev.h.
#include "wisp_common.h"
#include "hash_sdf_eval_dev.h"
#include "sphere_trace_dev.h"

#define HSDF_BLOCK 256
#define HSDF_GROUPS (HSDF_BLOCK / HSDF_GROUP)

// out [n, 1] (optional), counts {intersection, union} of (pred < 0) and (gt < 0) (optional).  Grid-stride over rounds of 16
// points: the block stages the weights once.
template <typename T>
__global__ void __launch_bounds__(HSDF_BLOCK)
hash_sdf_point_query_kernel(const float* __restrict__ coords, int64_t n, HashSdfField fld, float* __restrict__ out,
                      const float* __restrict__ gts, unsigned long long* __restrict__ counts) {
    extern __shared__ float s_hsdf[];
    const HashSdfLds s = hash_sdf_stage(s_hsdf, fld);
    const int c = threadIdx.x & (HSDF_GROUP - 1), grp = threadIdx.x / HSDF_GROUP;
    float* gin = s.in + grp * s.stride;
    const int64_t rounds = (n + HSDF_GROUPS - 1) / HSDF_GROUPS;
    unsigned int both = 0, either = 0;                   // wave-uniform; a wave sees 4 points a round: no overflow below 2^30 rounds
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * HSDF_GROUPS + grp;
        const bool live = i < n;                         // dead groups evaluate the origin: every lane stays in the ballots
        const float px = live ? coords[i * 3] : 0.0f, py = live ? coords[i * 3 + 1] : 0.0f, pz = live ? coords[i * 3 + 2] : 0.0f;
        const float o = hash_sdf_eval_point<T>(fld, s, gin, c, px, py, pz);
        if (out && live && c == 0) out[i] = o;
        if (counts) {
            const bool mine = live && c == 0;
            const bool pin = mine && o < 0.0f;
            const bool gt_in = mine && gts[i] < 0.0f;
            both += __popcll(__ballot(pin && gt_in));
            either += __popcll(__ballot(pin || gt_in));
        }
    }
    if (counts && (threadIdx.x & (WISP_WAVE - 1)) == 0) {      // one lane per wave, one add per counter
        if (both) atomicAdd(counts, (unsigned long long)both);
        if (either) atomicAdd(counts + 1, (unsigned long long)either);
    }
}

// grad[i, a] = (f(x + eps e_a) - f(x - eps e_a)) / (2 eps): finitediff_gradient in one launch.  The six positions are formed in
// fp32 as torch forms x + offs[a] / x - offs[a]; every value comes from hash_sdf_eval_point.
template <typename T>
__global__ void __launch_bounds__(HSDF_BLOCK)
hash_sdf_point_gradient_kernel(const float* __restrict__ coords, int64_t n, HashSdfField fld, float eps, float* __restrict__ grad) {
    extern __shared__ float s_hsdf[];
    const HashSdfLds s = hash_sdf_stage(s_hsdf, fld);
    const int c = threadIdx.x & (HSDF_GROUP - 1), grp = threadIdx.x / HSDF_GROUP;
    float* gin = s.in + grp * s.stride;
    const int64_t rounds = (n + HSDF_GROUPS - 1) / HSDF_GROUPS;
    const float two_eps = 2.0f * eps;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * HSDF_GROUPS + grp;
        const bool live = i < n;
        const float x0 = live ? coords[i * 3] : 0.0f, x1 = live ? coords[i * 3 + 1] : 0.0f, x2 = live ? coords[i * 3 + 2] : 0.0f;
        float mine = 0.0f;
#pragma unroll 1
        for (int a = 0; a < 3; ++a) {
            const float ep = (a == 0 ? x0 : a == 1 ? x1 : x2) + eps, em = (a == 0 ? x0 : a == 1 ? x1 : x2) - eps;
            const float fp = hash_sdf_eval_point<T>(fld, s, gin, c, a == 0 ? ep : x0, a == 1 ? ep : x1, a == 2 ? ep : x2);
            const float fm = hash_sdf_eval_point<T>(fld, s, gin, c, a == 0 ? em : x0, a == 1 ? em : x1, a == 2 ? em : x2);
            const float g = (fp - fm) / two_eps;
            if (c == a) mine = g;
        }
        if (live && c < 3) grad[i * 3 + c] = mine;
    }
}

// One marching iteration of PackedSDFTracer.trace (wisp/tracers/packed_sdf_tracer.py:118-146) including the field query
// nef(coords=x, channels="sdf") of a NeuralSDF over a HashGrid.  16 lanes own one pack: all 16 run the (pack-uniform)
// bookkeeping of sphere_trace_step (sphere_trace_dev.h), lane 0 stores the state, and the packs still marching evaluate the
// field at the new position.  A group leaves as a whole, so nothing below the exits is wave-wide.
template <typename T>
__global__ void __launch_bounds__(HSDF_BLOCK)
hash_sdf_march_kernel(SphereTraceState st, int first, HashSdfField fld, float scale, int32_t* __restrict__ any_active) {
    extern __shared__ float s_hsdf[];
    const HashSdfLds s = hash_sdf_stage(s_hsdf, fld);
    const int c = threadIdx.x & (HSDF_GROUP - 1), grp = threadIdx.x / HSDF_GROUP;
    const int64_t p = (int64_t)blockIdx.x * HSDF_GROUPS + grp;
    if (p >= st.num_packs) return;
    float px, py, pz;
    bool m;
    if (first) {
        m = st.mask[p] != 0;
        px = st.x[p * 3]; py = st.x[p * 3 + 1]; pz = st.x[p * 3 + 2];
    } else {
        m = sphere_trace_step(st, p, c == 0, px, py, pz);
    }
    if (!m) return;
    if (c == 0 && any_active) atomicAdd(any_active, 1);
    const float o = hash_sdf_eval_point<T>(fld, s, s.in + grp * s.stride, c, px, py, pz);
    if (c == 0) {
#pragma clang fp contract(off)
        st.dist[p] = o * scale;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static_assert(((size_t)HSDF_MAX_HIDDEN * ((3 + HSDF_MAX_COLS) | 1) + 2 * HSDF_MAX_HIDDEN +
               (size_t)HSDF_GROUPS * (3 + HSDF_MAX_COLS + HSDF_MAX_LODS * 8)) * sizeof(float) <= 64 * 1024,
              "the largest shape (hidden 256, 32 columns, 'sum' of 16 levels x 8) must fit the default dynamic LDS limit");
static_assert(HSDF_MAX_LODS <= HG_MAX_LODS, "HashLevels holds the levels");

static inline size_t hash_sdf_lds(const HashSdfField& fld) {
    return hash_sdf_lds_bytes(fld.hidden, fld.cols, fld.num_lods, fld.feature_dim, fld.sum, HSDF_GROUPS);
}

// enough blocks to fill the chip several times over, few enough that staging the weights (<= 37 KB) stays a small share
static inline unsigned hash_sdf_grid(int64_t n) { return (unsigned)min64(ceil_div64(n, HSDF_GROUPS), 2048); }

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
    const size_t lds = hash_sdf_lds(fld);
    WISP_REQUIRE(lds <= 64 * 1024, "LDS budget exceeded");
    const dim3 grid(hash_sdf_grid(n)), block(HSDF_BLOCK);
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
    const size_t lds = hash_sdf_lds(fld);
    WISP_REQUIRE(lds <= 64 * 1024, "LDS budget exceeded");
    const dim3 grid(hash_sdf_grid(n)), block(HSDF_BLOCK);
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
    const size_t lds = hash_sdf_lds(fld);
    WISP_REQUIRE(lds <= 64 * 1024, "LDS budget exceeded");
    const dim3 grid((unsigned)ceil_div64(num_packs, HSDF_GROUPS)), block(HSDF_BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define HSDF_T(T) hipLaunchKernelGGL((hash_sdf_march_kernel<T>), grid, block, lds, s, st, first, fld, scale, any_active)
    HSDF_DISPATCH(HSDF_T);
#undef HSDF_T
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
