// Evaluation of an nglod field outside training, for gfx950: the signed distance (or NeuralSDFTex's four raw outputs) at
// arbitrary points, the intersection-over-union counters of a validation batch, central-difference normals, and one marching
// iteration of PackedSDFTracer including the field query - one launch each.  The modular path is an octree query, a multi-level
// trilinear launch and two library GEMMs per call - six times over for a normal, once more with ~25 masked tensor ops, a
// scatter and a `mask.any()` read-back per marching iteration - and one host read-back per 512-point validation batch.
// Field evaluation: sdf_eval_dev.h.  Marching bookkeeping: sphere_trace_dev.h.
#include "wisp_common.h"
#include "sdf_eval_dev.h"
#include "sphere_trace_dev.h"

#define SDFE_BLOCK 256
#define SDFE_GROUPS (SDFE_BLOCK / SDFE_GROUP)

// out [n, ROWS] (optional), counts {intersection, union} of (pred < 0) and (gt < 0) on the last output row (optional).
// Grid-stride over rounds of 16 points: the block stages the weights once.
template <typename T, int ROWS>
__global__ void __launch_bounds__(SDFE_BLOCK)
sdf_query_kernel(const float* __restrict__ coords, int64_t n, SdfEvalField fld, float* __restrict__ out,
                 const float* __restrict__ gts, unsigned long long* __restrict__ counts) {
    extern __shared__ float s_sdfe[];
    const SdfEvalLds s = sdf_eval_stage(s_sdfe, fld, ROWS);
    const int c = threadIdx.x & (SDFE_GROUP - 1), grp = threadIdx.x / SDFE_GROUP;
    float* gin = s.in + grp * SDFE_IN;
    const int64_t rounds = (n + SDFE_GROUPS - 1) / SDFE_GROUPS;
    unsigned int both = 0, either = 0;                   // wave-uniform; a wave sees 4 points a round: no overflow below 2^30 rounds
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * SDFE_GROUPS + grp;
        const bool live = i < n;                         // dead groups evaluate the origin: every lane stays in the shuffles
        const float px = live ? coords[i * 3] : 0.0f, py = live ? coords[i * 3 + 1] : 0.0f, pz = live ? coords[i * 3 + 2] : 0.0f;
        float o[ROWS];
        sdf_eval_point<T, ROWS>(fld, s, gin, c, px, py, pz, o);
        if (out && live && c < ROWS) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
                if (c == r) out[i * ROWS + r] = o[r];
        }
        if (counts) {
            const bool mine = live && c == 0;
            const bool pin = mine && o[ROWS - 1] < 0.0f;
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

// grad[i, a] = (f(x + eps e_a) - f(x - eps e_a)) / (2 eps) on the distance row: finitediff_gradient in one launch.  The six
// positions are formed in fp32 as torch forms x + offs[a] / x - offs[a]; every value comes from sdf_eval_point.
template <typename T, int ROWS>
__global__ void __launch_bounds__(SDFE_BLOCK)
sdf_fd_gradient_kernel(const float* __restrict__ coords, int64_t n, SdfEvalField fld, float eps, float* __restrict__ grad) {
    extern __shared__ float s_sdfe[];
    const SdfEvalLds s = sdf_eval_stage(s_sdfe, fld, ROWS);
    const int c = threadIdx.x & (SDFE_GROUP - 1), grp = threadIdx.x / SDFE_GROUP;
    float* gin = s.in + grp * SDFE_IN;
    const int64_t rounds = (n + SDFE_GROUPS - 1) / SDFE_GROUPS;
    const float two_eps = 2.0f * eps;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * SDFE_GROUPS + grp;
        const bool live = i < n;
        const float x0 = live ? coords[i * 3] : 0.0f, x1 = live ? coords[i * 3 + 1] : 0.0f, x2 = live ? coords[i * 3 + 2] : 0.0f;
        float mine = 0.0f;
#pragma unroll 1
        for (int a = 0; a < 3; ++a) {
            const float ep = (a == 0 ? x0 : a == 1 ? x1 : x2) + eps, em = (a == 0 ? x0 : a == 1 ? x1 : x2) - eps;
            float fp[ROWS], fm[ROWS];
            sdf_eval_point<T, ROWS>(fld, s, gin, c, a == 0 ? ep : x0, a == 1 ? ep : x1, a == 2 ? ep : x2, fp);
            sdf_eval_point<T, ROWS>(fld, s, gin, c, a == 0 ? em : x0, a == 1 ? em : x1, a == 2 ? em : x2, fm);
            const float g = (fp[ROWS - 1] - fm[ROWS - 1]) / two_eps;
            if (c == a) mine = g;
        }
        if (live && c < 3) grad[i * 3 + c] = mine;
    }
}

// One marching iteration of PackedSDFTracer.trace (wisp/tracers/packed_sdf_tracer.py:118-146) including the field query
// nef(coords=x, channels="sdf") of a NeuralSDF over an OctreeGrid (or the distance row of a NeuralSDFTex).  16 lanes own one
// pack (= one ray that hit the octree): all 16 run the (pack-uniform) bookkeeping of sphere_trace_step (sphere_trace_dev.h),
// lane 0 stores the state, and the packs still marching evaluate the field at the new position - the values wisp_sdf_query
// returns there, bit for bit.  A group leaves as a whole, so nothing below the exits is wave-wide.
template <typename T>
__global__ void __launch_bounds__(SDFE_BLOCK)
sdf_trace_fused_kernel(SphereTraceState st, int first, SdfEvalField fld, float scale, int32_t* __restrict__ any_active) {
    extern __shared__ float s_sdfe[];
    const SdfEvalLds s = sdf_eval_stage(s_sdfe, fld, 1);
    const int c = threadIdx.x & (SDFE_GROUP - 1), grp = threadIdx.x / SDFE_GROUP;
    const int64_t p = (int64_t)blockIdx.x * SDFE_GROUPS + grp;
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
    float o[1];
    sdf_eval_point<T, 1>(fld, s, s.in + grp * SDFE_IN, c, px, py, pz, o);
    if (c == 0) {
#pragma clang fp contract(off)
        st.dist[p] = o[0] * scale;
    }
}

static int sdf_eval_fill(SdfEvalField& fld, const char* fn, const uint8_t* octree, const int32_t* exsum, const int16_t* points,
                         const int32_t* trinkets, const void* const* feats, int dtype, const int32_t* levels, int num_lods,
                         int channels, int half_round, const float* w1, const float* b1, const float* w2, const float* b2,
                         int hidden, int out_rows) {
#define SDFE_REQUIRE(cond, what) do { if (!(cond)) return wisp_fail(WISP_ERR_INVALID, fn, what); } while (0)
    SDFE_REQUIRE(num_lods >= 1 && num_lods <= SDFE_MAX_LODS, "bad sizes");
    SDFE_REQUIRE(channels == SDFE_CHANNELS, "the fused field query is built for 16 feature channels (nglod_octree.yaml)");
    SDFE_REQUIRE(hidden >= 1 && hidden <= SDFE_MAX_HIDDEN, "hidden width out of range");
    SDFE_REQUIRE(out_rows == 1 || out_rows == 4, "out_rows must be 1 (NeuralSDF) or 4 (NeuralSDFTex)");
    SDFE_REQUIRE(dtype == WISP_F32 || dtype == WISP_F16 || dtype == WISP_BF16, "bad dtype");
    SDFE_REQUIRE(octree && exsum && points && trinkets && feats && levels && w1 && b1 && w2 && b2, "null pointer");
    for (int l = 0; l < num_lods; ++l) {
        SDFE_REQUIRE(feats[l] && levels[l] >= 0 && levels[l] <= 15 && (l == 0 || levels[l] > levels[l - 1]), "bad level list");
        fld.feats[l] = feats[l]; fld.level[l] = levels[l];
    }
#undef SDFE_REQUIRE
    for (int l = num_lods; l < SDFE_MAX_LODS; ++l) { fld.feats[l] = nullptr; fld.level[l] = 0; }
    fld.num_lods = num_lods; fld.half_round = half_round; fld.hidden = hidden; fld.max_level = levels[num_lods - 1];
    fld.w1 = w1; fld.b1 = b1; fld.w2 = w2; fld.b2 = b2;
    fld.octree = octree; fld.exsum = exsum; fld.points = points; fld.trinkets = trinkets;
    return WISP_OK;
}

// enough blocks to fill the chip several times over, few enough that staging the weights (<= 25.8 KB: hidden 256, four rows) stays a small share
static inline unsigned sdf_eval_grid(int64_t n) { return (unsigned)min64(ceil_div64(n, SDFE_GROUPS), 2048); }

extern "C" int wisp_sdf_query(const float* coords, int64_t n, const uint8_t* octree, const int32_t* exsum, const int16_t* points,
                              const int32_t* trinkets, const void* const* feats, int feats_dtype, const int32_t* levels,
                              int num_lods, int channels, int half_round, const float* w1, const float* b1, const float* w2,
                              const float* b2, int hidden, int out_rows, float* out, const float* gts, int64_t* counts,
                              wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "bad sizes");
    SdfEvalField fld;
    if (const int rc = sdf_eval_fill(fld, __func__, octree, exsum, points, trinkets, feats, feats_dtype, levels, num_lods, channels,
                                     half_round, w1, b1, w2, b2, hidden, out_rows)) return rc;
    WISP_REQUIRE(!counts || gts, "counts given without gts");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && (out || counts), "null pointer");
    const size_t lds = sdf_eval_lds_bytes(hidden, out_rows, SDFE_GROUPS);
    const dim3 grid(sdf_eval_grid(n)), block(SDFE_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
#define SDFE_Q(T, R) hipLaunchKernelGGL((sdf_query_kernel<T, R>), grid, block, lds, s, coords, n, fld, out, counts ? gts : nullptr, cnt)
#define SDFE_QT(T) do { if (out_rows == 1) SDFE_Q(T, 1); else SDFE_Q(T, 4); } while (0)
    if (feats_dtype == WISP_F32) SDFE_QT(float); else if (feats_dtype == WISP_F16) SDFE_QT(__half); else SDFE_QT(__hip_bfloat16);
#undef SDFE_QT
#undef SDFE_Q
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_sdf_fd_gradient(const float* coords, int64_t n, const uint8_t* octree, const int32_t* exsum,
                                    const int16_t* points, const int32_t* trinkets, const void* const* feats, int feats_dtype,
                                    const int32_t* levels, int num_lods, int channels, int half_round, const float* w1,
                                    const float* b1, const float* w2, const float* b2, int hidden, int out_rows, float eps,
                                    float* grad, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "bad sizes");
    SdfEvalField fld;
    if (const int rc = sdf_eval_fill(fld, __func__, octree, exsum, points, trinkets, feats, feats_dtype, levels, num_lods, channels,
                                     half_round, w1, b1, w2, b2, hidden, out_rows)) return rc;
    WISP_REQUIRE(eps > 0.0f, "eps must be positive");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && grad, "null pointer");
    const size_t lds = sdf_eval_lds_bytes(hidden, out_rows, SDFE_GROUPS);
    const dim3 grid(sdf_eval_grid(n)), block(SDFE_BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define SDFE_G(T, R) hipLaunchKernelGGL((sdf_fd_gradient_kernel<T, R>), grid, block, lds, s, coords, n, fld, eps, grad)
#define SDFE_GT(T) do { if (out_rows == 1) SDFE_G(T, 1); else SDFE_G(T, 4); } while (0)
    if (feats_dtype == WISP_F32) SDFE_GT(float); else if (feats_dtype == WISP_F16) SDFE_GT(__half); else SDFE_GT(__hip_bfloat16);
#undef SDFE_GT
#undef SDFE_G
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_sdf_trace_step_fused(int64_t num_packs, int first, const float* nug_o, const float* nug_d, const float* nug_depth,
                                         const int32_t* nug_pidx, float dist_max, float thr_close, float thr_avg, float* t,
                                         float* dist, float* dist_prev, uint8_t* mask, uint8_t* hit, const int32_t* curr_in,
                                         int32_t* curr_out, int64_t* curr_pidx, float* x, const uint8_t* octree,
                                         const int32_t* exsum, const int16_t* points, const int32_t* trinkets,
                                         const void* const* feats, int feats_dtype, const int32_t* levels, int num_lods,
                                         int channels, int half_round, const float* w1, const float* b1, const float* w2,
                                         const float* b2, int hidden, float scale, int32_t* any_active, wisp_stream_t stream) {
    WISP_REQUIRE(num_packs >= 0, "bad sizes");
    SdfEvalField fld;
    if (const int rc = sdf_eval_fill(fld, __func__, octree, exsum, points, trinkets, feats, feats_dtype, levels, num_lods, channels,
                                     half_round, w1, b1, w2, b2, hidden, 1)) return rc;
    if (num_packs == 0) return WISP_OK;
    const SphereTraceState st{num_packs, nug_o, nug_d, nug_depth, nug_pidx, dist_max, thr_close, thr_avg, t, dist, dist_prev,
                              mask, hit, curr_in, curr_out, curr_pidx, x};
    WISP_REQUIRE(sphere_trace_state_complete(st), "null pointer");
    const size_t lds = sdf_eval_lds_bytes(hidden, 1, SDFE_GROUPS);
    const dim3 grid((unsigned)ceil_div64(num_packs, SDFE_GROUPS)), block(SDFE_BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define SDFE_T(T) hipLaunchKernelGGL((sdf_trace_fused_kernel<T>), grid, block, lds, s, st, first, fld, scale, any_active)
    if (feats_dtype == WISP_F32) SDFE_T(float); else if (feats_dtype == WISP_F16) SDFE_T(__half); else SDFE_T(__hip_bfloat16);
#undef SDFE_T
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
