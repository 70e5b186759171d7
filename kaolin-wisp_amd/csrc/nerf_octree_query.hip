// The inference query of an octree-backed radiance field - nerf_octree.yaml (OctreeGrid) and, over decoded dictionary rows,
// nerf_codebook.yaml (CodebookOctreeGrid in eval mode) - as ONE launch: NeuralRadianceField.rgba (wisp/models/nefs/nerf.py:219-264)
// over OctreeGrid.interpolate (wisp/models/grids/octree_grid.py:165-219).
//
// The modular path runs, per chunk of samples: an index_select of the ray directions, the octree query that writes an
// [S, num_lods] int64 chain, the multi-level trilinear lookup into a feature tensor (for a codebook grid one lookup per level,
// then cat / reshape / sum) and the exact-fp32 decoder.  Here a wave takes 64 samples, as in nerf_query.hip: every lane walks the
// octree for its own sample and blends the corner rows of every listed level (octree_nerf_eval_dev.h) straight into the
// decoder's input tile in the wave's LDS slice, and the tile's two halves of 32 samples run all five layers on the matrix cores
// through the stage macros of nerf_mlp_f32_dev.h - the sequence nerf_query_kernel expands, stage for stage.  (It is expanded here a
// second time rather than moved: nerf_query.hip stays byte for byte what its tests pin.)  Every value is the bits the modular
// path computes: the lookup is spc_trilinear_multi_fwd's arithmetic, the decoder is the shared MFMA sequence.
#include "wisp_common.h"
#include "octree_nerf_eval_dev.h"
#include "nerf_mlp_f32_dev.h"

namespace {

using namespace wisp_mlp;

// one workgroup per CU (LDS), one wave per SIMD, as nerf_query.hip found necessary for the same tiles
constexpr int NOQ_WAVES = 4;
constexpr int NOQ_TILE = 64;              // samples per wave tile: one per lane in the lookup, two MFMA tiles of TS = 32
// LDS (floats), the layout of nerf_query.hip: biases b1 [H], b2 [32], b3 [H], b4 [H], b5 [32]; W1 [H][LDI], W2 [32][LDH],
// W3 [H][LDH], W4 [H][LDH], W5 [32][LDH]; per wave x0 [64][LDI] and two [32][LDH] tiles A and B whose tenants do not overlap:
//   A = h1 (written by L1, dead after L2), then h2 (written by L3, read by L4)
//   B = x2 (view code before L1, geometry features from L2, dead after L3), then h3 (written by L4, read by L5)
constexpr int NOQ_B1 = 0, NOQ_B2 = H, NOQ_B3 = H + 32, NOQ_B4 = 2 * H + 32, NOQ_B5 = 3 * H + 32, NOQ_NBIAS = 3 * H + 64;
constexpr int NOQ_W1 = NOQ_NBIAS, NOQ_W2 = NOQ_W1 + H * F32_LDI, NOQ_W3 = NOQ_W2 + 32 * F32_LDH, NOQ_W4 = NOQ_W3 + H * F32_LDH,
              NOQ_W5 = NOQ_W4 + H * F32_LDH, NOQ_ACT = NOQ_W5 + 32 * F32_LDH;
constexpr int NOQ_X0 = 0, NOQ_A = NOQ_TILE * F32_LDI, NOQ_B = NOQ_A + TS * F32_LDH, NOQ_ACT_WAVE = NOQ_B + TS * F32_LDH;
constexpr size_t NOQ_LDS_BYTES = (size_t)(NOQ_ACT + NOQ_WAVES * NOQ_ACT_WAVE) * 4;
static_assert(NOQ_LDS_BYTES <= 160 * 1024, "one workgroup must fit the CU's LDS");
static_assert(ONE_MAX_FEATURES <= IN, "a level's features must fit the decoder's input row");

// RGB = false: the density alone, the kernel stops after layer 2 (no view direction is read)
template <typename T, bool RGB>
__global__ void __launch_bounds__(NOQ_WAVES * 64, 1)
nerf_octree_query_kernel(const float* __restrict__ coords, const float* __restrict__ dirs, const int64_t* __restrict__ ridx,
                         int64_t num_rays, int64_t n_samples, OctreeNerfField fld, int in_dim, const float* __restrict__ params,
                         float* __restrict__ out_rgb, float* __restrict__ out_density) {
    extern __shared__ __attribute__((aligned(16))) float noq_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* x0 = noq_smem + NOQ_ACT + wave * NOQ_ACT_WAVE + NOQ_X0;
    float* ta = noq_smem + NOQ_ACT + wave * NOQ_ACT_WAVE + NOQ_A;
    float* tb = noq_smem + NOQ_ACT + wave * NOQ_ACT_WAVE + NOQ_B;

    // ---- stage the parameters: zero everything (padding rows / columns must be 0), then the real entries
    for (int e = threadIdx.x; e < NOQ_ACT; e += NOQ_WAVES * 64) noq_smem[e] = 0.0f;
    __syncthreads();
    f32_stage_density_params(params, in_dim, noq_smem + NOQ_W1, noq_smem + NOQ_B1, noq_smem + NOQ_W2, noq_smem + NOQ_B2, threadIdx.x,
                             NOQ_WAVES * 64);
    if (RGB)
        f32_stage_color_params(params, in_dim, noq_smem + NOQ_W3, noq_smem + NOQ_B3, noq_smem + NOQ_W4, noq_smem + NOQ_B4,
                               noq_smem + NOQ_W5, noq_smem + NOQ_B5, threadIdx.x, NOQ_WAVES * 64);
    __syncthreads();

    const int64_t ntiles = (n_samples + NOQ_TILE - 1) / NOQ_TILE;
    for (int64_t tile = (int64_t)blockIdx.x * NOQ_WAVES + wave; tile < ntiles; tile += (int64_t)gridDim.x * NOQ_WAVES) {
        const int64_t i = tile * NOQ_TILE + lane;
        const bool live = i < n_samples;
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (live) { c[0] = coords[i * 3]; c[1] = coords[i * 3 + 1]; c[2] = coords[i * 3 + 2]; }
        // ---- lookup: walk + blend of every listed level, the 'sum' / 'cat' row (zero padded up to IN) into the input tile
        octree_nerf_encode<T>(fld, live, c[0], c[1], c[2], x0 + lane * F32_LDI, IN);
        __builtin_amdgcn_wave_barrier();
        // ---- decoder for the tile's two halves of 32 samples; lane (n, half) works on sample `s`
#pragma unroll 1
        for (int part = 0; part < 2; ++part) {
            const float* xp = x0 + part * TS * F32_LDI;
            const int n = lane & 31, half = lane >> 5;
            const int64_t s = tile * NOQ_TILE + part * TS + n;
            const bool alive = s < n_samples;
            if (RGB) {
                // the view direction: per sample, or the sample's ray's (rays.dirs.index_select(0, ridx) of the tracer, same bits);
                // a ray index outside [0, num_rays) is clamped, so nothing is read out of bounds
                float d[3] = {0.f, 0.f, 0.f};
                if (alive) {
                    int64_t r = s;
                    if (ridx) { r = ridx[s]; r = r < 0 ? 0 : (r >= num_rays ? num_rays - 1 : r); }
                    d[0] = dirs[r * 3]; d[1] = dirs[r * 3 + 1]; d[2] = dirs[r * 3 + 2];
                }
                WISP_F32_VIEW_ENCODE(tb, n, half, d)
            }
            // L1: h1 = relu(W1 x0 + b1) -> A;  L2: y = W2 h1 + b2, density = relu(y0), geometry features y[1..15] -> B[:, 0..14]
            WISP_F32_LAYER1(noq_smem, NOQ_W1, noq_smem, NOQ_B1, xp, ta, n, lane)
            __builtin_amdgcn_wave_barrier();
            float y0 = 0.0f;
            WISP_F32_LAYER2(noq_smem, NOQ_W2, noq_smem, NOQ_B2, ta, n, lane, y0, RGB, tb)
            if (half == 0 && alive && out_density) out_density[s] = fmaxf(y0, 0.0f);
            __builtin_amdgcn_wave_barrier();
            if (RGB) {
                // L3: h2 = relu(W3 x2 + b3), B -> A;  L4: h3 = relu(W4 h2 + b4), A -> B;  L5: rgb = sigmoid(W5 h3 + b5)
                WISP_F32_LAYER_HIDDEN(noq_smem, NOQ_W3, noq_smem, NOQ_B3, F32_K3, tb, ta, n, lane)
                __builtin_amdgcn_wave_barrier();
                WISP_F32_LAYER_HIDDEN(noq_smem, NOQ_W4, noq_smem, NOQ_B4, H, ta, tb, n, lane)
                __builtin_amdgcn_wave_barrier();
                float sg[3] = {0.f, 0.f, 0.f};
                WISP_F32_LAYER5(noq_smem, NOQ_W5, noq_smem, NOQ_B5, tb, lane, sg)
                if (half == 0 && alive) { out_rgb[s * 3] = sg[0]; out_rgb[s * 3 + 1] = sg[1]; out_rgb[s * 3 + 2] = sg[2]; }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

int noq_cu_count() {
    static int n = [] { int d = 0, c = 0; (void)hipGetDevice(&d); (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d); return c > 0 ? c : 256; }();
    return n;
}

template <typename T>
int noq_launch(const float* coords, const float* dirs, const int64_t* ridx, int64_t num_rays, int64_t n, const OctreeNerfField& fld,
               int in_dim, const float* params, float* rgb, float* density, hipStream_t stream) {
    auto kern = rgb ? nerf_octree_query_kernel<T, true> : nerf_octree_query_kernel<T, false>;
    const hipError_t e = rgb ? WISP_ALLOW_LDS((nerf_octree_query_kernel<T, true>), NOQ_LDS_BYTES)
                             : WISP_ALLOW_LDS((nerf_octree_query_kernel<T, false>), NOQ_LDS_BYTES);
    if (e != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, "nerf_octree_query", hipGetErrorString(e));
    const int64_t ntiles = ceil_div64(n, NOQ_TILE);
    const int grid = (int)min64(ceil_div64(ntiles, NOQ_WAVES), noq_cu_count());
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NOQ_WAVES * 64), NOQ_LDS_BYTES, stream, coords, dirs, ridx, num_rays, n, fld, in_dim,
                       params, rgb, density);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

}  // namespace

extern "C" int wisp_nerf_octree_query(const float* coords, const float* dirs, const int64_t* ridx, int64_t num_rays, int64_t n,
                                      const uint8_t* octree, const int32_t* exsum, const int16_t* points, const int32_t* trinkets,
                                      int max_level, const void* const* feats, int dtype_feats, const int32_t* levels, int num_lods,
                                      int feature_dim, int half_round, int sum, const float* params, int dtype_params, int in_dim,
                                      int hidden, float* rgb, float* density, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "negative sample count");
    if (feature_dim < 1 || feature_dim > ONE_MAX_FEATURES || num_lods < 1 || num_lods > ONE_MAX_LODS || hidden != H ||
        in_dim != (sum ? feature_dim : num_lods * feature_dim) || in_dim > IN ||
        (dtype_feats != WISP_F32 && dtype_feats != WISP_F16 && dtype_feats != WISP_BF16) || dtype_params != WISP_F32)
        return wisp_fail(WISP_ERR_UNSUPPORTED, "nerf_octree_query",
                         "this build supports feature_dim 1..16, 1..16 levels, hidden 64, in_dim = feature_dim ('sum') or levels * "
                         "feature_dim ('cat') <= 32, f32 / f16 / bf16 tables and fp32 parameters");
    WISP_REQUIRE(max_level >= 0 && max_level <= 15, "max_level out of range");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && exsum && points && trinkets && feats && levels && params && (rgb || density) && (octree || max_level == 0),
                 "null pointer");
    WISP_REQUIRE(!rgb || dirs, "null pointer");                                   // the colour needs a view direction
    WISP_REQUIRE(!ridx || (dirs && num_rays >= 1), "ridx needs ray_dirs with at least one ray");
    WISP_REQUIRE(((uintptr_t)trinkets & 15) == 0, "trinkets must be 16-byte aligned");
    OctreeNerfField fld;
    for (int l = 0; l < ONE_MAX_LODS; ++l) { fld.feats[l] = nullptr; fld.level[l] = 0; }
    for (int l = 0; l < num_lods; ++l) {
        WISP_REQUIRE(levels[l] >= 0 && levels[l] <= max_level && (l == 0 || levels[l] > levels[l - 1]),
                     "levels must ascend and end at or below max_level");
        WISP_REQUIRE(feats[l], "null feature table");
        fld.feats[l] = feats[l];
        fld.level[l] = levels[l];
    }
    fld.num_lods = num_lods; fld.feature_dim = feature_dim; fld.half_round = half_round ? 1 : 0; fld.sum = sum ? 1 : 0;
    fld.octree = octree; fld.exsum = exsum; fld.points = points; fld.trinkets = trinkets;
    hipStream_t s = (hipStream_t)stream;
    if (dtype_feats == WISP_F32) return noq_launch<float>(coords, dirs, ridx, num_rays, n, fld, in_dim, params, rgb, density, s);
    if (dtype_feats == WISP_F16) return noq_launch<__half>(coords, dirs, ridx, num_rays, n, fld, in_dim, params, rgb, density, s);
    return noq_launch<__hip_bfloat16>(coords, dirs, ridx, num_rays, n, fld, in_dim, params, rgb, density, s);
}
