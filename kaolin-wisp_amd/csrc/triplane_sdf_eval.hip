// Evaluation and sphere tracing of a triplanar SDF field (nglod_triplanar.yaml: NeuralSDF over a TriplanarGrid, 'sum', one level
// of three 4 x 33 x 33 planes, raw position in front, one hidden relu layer) for gfx950: the signed distance at arbitrary points
// with the intersection-over-union counters of a validation batch, central-difference normals, and one marching iteration of
// PackedSDFTracer including the field query - one launch each.  The modular path is a wisp_triplane_fwd launch, a cat and a
// decoder launch per query, six queries per normal, and a boolean-mask gather, a scatter and two read-backs per marching
// iteration.  Field evaluation: triplane_sdf_eval_dev.h.
#include "wisp_common.h"
#include "triplane_sdf_eval_dev.h"
#include "sphere_trace_dev.h"

#define TSDF_BLOCK 256
#define TSDF_GROUPS (TSDF_BLOCK / TSDF_GROUP)

// out [n, 1] (optional), counts {intersection, union} of (pred < 0) and (gt < 0) (optional).  Grid-stride over rounds of 16
// points: the block stages the weights once.
__global__ void __launch_bounds__(TSDF_BLOCK)
tri_sdf_point_query_kernel(const float* __restrict__ coords, int64_t n, TriSdfField fld, float* __restrict__ out,
                           const float* __restrict__ gts, unsigned long long* __restrict__ counts) {
    extern __shared__ float s_tsdf[];
    const TriSdfLds s = tri_sdf_stage(s_tsdf, fld);
    const int c = threadIdx.x & (TSDF_GROUP - 1), grp = threadIdx.x / TSDF_GROUP;
    float* gin = s.in + grp * s.stride;
    const int64_t rounds = (n + TSDF_GROUPS - 1) / TSDF_GROUPS;
    unsigned int both = 0, either = 0;                   // wave-uniform; a wave sees 4 points a round: no overflow below 2^30 rounds
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * TSDF_GROUPS + grp;
        const bool live = i < n;                         // dead groups evaluate the origin: every lane stays in the ballots
        const float px = live ? coords[i * 3] : 0.0f, py = live ? coords[i * 3 + 1] : 0.0f, pz = live ? coords[i * 3 + 2] : 0.0f;
        const float o = tri_sdf_eval_point(fld, s, gin, c, px, py, pz);
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
// fp32 as torch forms x + offs[a] / x - offs[a]; every value comes from tri_sdf_eval_point.
__global__ void __launch_bounds__(TSDF_BLOCK)
tri_sdf_point_gradient_kernel(const float* __restrict__ coords, int64_t n, TriSdfField fld, float eps, float* __restrict__ grad) {
    extern __shared__ float s_tsdf[];
    const TriSdfLds s = tri_sdf_stage(s_tsdf, fld);
    const int c = threadIdx.x & (TSDF_GROUP - 1), grp = threadIdx.x / TSDF_GROUP;
    float* gin = s.in + grp * s.stride;
    const int64_t rounds = (n + TSDF_GROUPS - 1) / TSDF_GROUPS;
    const float two_eps = 2.0f * eps;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * TSDF_GROUPS + grp;
        const bool live = i < n;
        const float x0 = live ? coords[i * 3] : 0.0f, x1 = live ? coords[i * 3 + 1] : 0.0f, x2 = live ? coords[i * 3 + 2] : 0.0f;
        float mine = 0.0f;
#pragma unroll 1
        for (int a = 0; a < 3; ++a) {
            const float ep = (a == 0 ? x0 : a == 1 ? x1 : x2) + eps, em = (a == 0 ? x0 : a == 1 ? x1 : x2) - eps;
            const float fp = tri_sdf_eval_point(fld, s, gin, c, a == 0 ? ep : x0, a == 1 ? ep : x1, a == 2 ? ep : x2);
            const float fm = tri_sdf_eval_point(fld, s, gin, c, a == 0 ? em : x0, a == 1 ? em : x1, a == 2 ? em : x2);
            const float g = (fp - fm) / two_eps;
            if (c == a) mine = g;
        }
        if (live && c < 3) grad[i * 3 + c] = mine;
    }
}

// One marching iteration of PackedSDFTracer.trace (wisp/tracers/packed_sdf_tracer.py:118-146) including the field query
// nef(coords=x, channels="sdf") of a NeuralSDF over a TriplanarGrid.  16 lanes own one pack: all 16 run the (pack-uniform)
// bookkeeping of sphere_trace_step (sphere_trace_dev.h), lane 0 stores the state, and the packs still marching evaluate the
// field at the new position.  A group leaves as a whole, so nothing below the exits is wave-wide.
__global__ void __launch_bounds__(TSDF_BLOCK)
tri_sdf_march_kernel(SphereTraceState st, int first, TriSdfField fld, float scale, int32_t* __restrict__ any_active) {
    extern __shared__ float s_tsdf[];
    const TriSdfLds s = tri_sdf_stage(s_tsdf, fld);
    const int c = threadIdx.x & (TSDF_GROUP - 1), grp = threadIdx.x / TSDF_GROUP;
    const int64_t p = (int64_t)blockIdx.x * TSDF_GROUPS + grp;
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
    const float o = tri_sdf_eval_point(fld, s, s.in + grp * s.stride, c, px, py, pz);
    if (c == 0) {
#pragma clang fp contract(off)
        st.dist[p] = o * scale;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static_assert(((size_t)TSDF_MAX_HIDDEN * ((3 + TSDF_MAX_COLS) | 1) + 2 * TSDF_MAX_HIDDEN + (size_t)TSDF_GROUPS * (3 + TSDF_MAX_COLS)) *
                  sizeof(float) <= 64 * 1024,
              "the largest shape (hidden 256, 48 columns) must fit the default dynamic LDS limit");

static inline size_t tri_sdf_lds(const TriSdfField& fld) { return tri_sdf_lds_bytes(fld.hidden, fld.cols, TSDF_GROUPS); }

// enough blocks to fill the chip several times over, few enough that staging the weights (<= 53 KB) stays a small share
static inline unsigned tri_sdf_grid(int64_t n) { return (unsigned)min64(ceil_div64(n, TSDF_GROUPS), 2048); }

extern "C" int wisp_triplane_sdf_query(const float* coords, int64_t n, const float* const* planes, const int32_t* sizes,
                                       int num_lods, int feature_dim, int multiscale, const float* w1, const float* b1,
                                       const float* w2, const float* b2, int hidden, float* out, const float* gts,
                                       int64_t* counts, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "bad sizes");
    TriSdfField fld;
    if (const int rc = tri_sdf_fill(fld, __func__, planes, sizes, num_lods, feature_dim, multiscale, w1, b1, w2, b2, hidden,
                                    TSDF_GROUPS)) return rc;
    WISP_REQUIRE(!counts || gts, "counts given without gts");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && (out || counts), "null pointer");
    hipLaunchKernelGGL(tri_sdf_point_query_kernel, dim3(tri_sdf_grid(n)), dim3(TSDF_BLOCK), tri_sdf_lds(fld), (hipStream_t)stream,
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
                                    TSDF_GROUPS)) return rc;
    WISP_REQUIRE(eps > 0.0f, "eps must be positive");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && grad, "null pointer");
    hipLaunchKernelGGL(tri_sdf_point_gradient_kernel, dim3(tri_sdf_grid(n)), dim3(TSDF_BLOCK), tri_sdf_lds(fld),
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
                                    TSDF_GROUPS)) return rc;
    if (num_packs == 0) return WISP_OK;
    const SphereTraceState st{num_packs, nug_o, nug_d, nug_depth, nug_pidx, dist_max, thr_close, thr_avg, t, dist, dist_prev,
                              mask, hit, curr_in, curr_out, curr_pidx, x};
    WISP_REQUIRE(sphere_trace_state_complete(st), "null pointer");
    hipLaunchKernelGGL(tri_sdf_march_kernel, dim3((unsigned)ceil_div64(num_packs, TSDF_GROUPS)), dim3(TSDF_BLOCK), tri_sdf_lds(fld),
                       (hipStream_t)stream, st, first, fld, scale, any_active);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
