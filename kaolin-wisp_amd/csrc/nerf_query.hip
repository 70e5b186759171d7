// The inference query of a nerf_hash.yaml radiance field (NeuralRadianceField.rgba, wisp/models/nefs/nerf.py:219-264) as ONE launch.
//
// The modular path runs, per chunk of samples: an index_select of the ray directions, the fp32 hash-grid lookup into a [S, 32]
// feature tensor (128 B written and 128 B read back per sample) and the exact-fp32 decoder.  Here a wave takes 64 samples: every
// lane walks the live levels of its own sample (wave-uniform, two levels at a time with sixteen gathers in flight, as in
// prune_query_kernel), the blended features go straight into the decoder's input tile in the wave's LDS slice, and the tile's two
// halves of 32 samples run all five layers on the matrix cores (nerf_mlp_f32_dev.h: the stages of nerf_mlp_kernel<float, ...>).
// The view direction is read per sample, or per ray through the sample's ray index.  Every value is the bits the modular path
// computes: the lookup is corner_setup + the forward kernel's fmaf chain, the decoder is the shared MFMA sequence.
#include "wisp_common.h"
#include "hashgrid_dev.h"
#include "nerf_mlp_f32_dev.h"

namespace {

using namespace wisp_mlp;

// one workgroup per CU (LDS), one wave per SIMD: what the aliased tiles leave room for.  Measured at 2^18 / 2^21 samples against the modular
// pair (0.42 / 3.17 ms): 2 waves 0.47 / 2.75 ms, 3 waves 0.41 / 2.06 ms, 4 waves 0.35 / 1.84 ms - more resident waves hide more of the gathers
constexpr int NQ_WAVES = 4;
constexpr int NQ_TILE = 64;               // samples per wave tile: one per lane in the lookup, two MFMA tiles of TS = 32
// LDS (floats): biases b1 [H], b2 [32], b3 [H], b4 [H], b5 [32]; W1 [H][LDI], W2 [32][LDH], W3 [H][LDH], W4 [H][LDH], W5 [32][LDH];
// per wave x0 [64][LDI] and two [32][LDH] tiles A and B whose tenants' lifetimes do not overlap:
//   A = h1 (written by L1, dead after L2), then h2 (written by L3, read by L4)
//   B = x2 (view code before L1, geometry features from L2, dead after L3), then h3 (written by L4, read by L5)
constexpr int NQ_B1 = 0, NQ_B2 = H, NQ_B3 = H + 32, NQ_B4 = 2 * H + 32, NQ_B5 = 3 * H + 32, NQ_NBIAS = 3 * H + 64;
constexpr int NQ_W1 = NQ_NBIAS, NQ_W2 = NQ_W1 + H * F32_LDI, NQ_W3 = NQ_W2 + 32 * F32_LDH, NQ_W4 = NQ_W3 + H * F32_LDH,
              NQ_W5 = NQ_W4 + H * F32_LDH, NQ_ACT = NQ_W5 + 32 * F32_LDH;
constexpr int NQ_X0 = 0, NQ_A = NQ_TILE * F32_LDI, NQ_B = NQ_A + TS * F32_LDH, NQ_ACT_WAVE = NQ_B + TS * F32_LDH;
constexpr size_t NQ_LDS_BYTES = (size_t)(NQ_ACT + NQ_WAVES * NQ_ACT_WAVE) * 4;
static_assert(NQ_LDS_BYTES <= 160 * 1024, "one workgroup must fit the CU's LDS");

// RGB = false: the density alone, the kernel stops after layer 2 (no view direction is read)
template <bool RGB>
__global__ void __launch_bounds__(NQ_WAVES * 64, 1)
nerf_query_kernel(const float* __restrict__ coords, const float* __restrict__ dirs, const int64_t* __restrict__ ridx, int64_t num_rays,
                  int64_t n_samples, const float* __restrict__ table, const int64_t* __restrict__ first_idx, HashLevels lv,
                  int num_lods, int live_lods, uint32_t tsize, int in_dim, const float* __restrict__ params,
                  float* __restrict__ out_rgb, float* __restrict__ out_density) {
    extern __shared__ __attribute__((aligned(16))) float nq_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* x0 = nq_smem + NQ_ACT + wave * NQ_ACT_WAVE + NQ_X0;
    float* ta = nq_smem + NQ_ACT + wave * NQ_ACT_WAVE + NQ_A;
    float* tb = nq_smem + NQ_ACT + wave * NQ_ACT_WAVE + NQ_B;

    // ---- stage the parameters: zero everything (padding rows / columns must be 0), then the real entries
    for (int e = threadIdx.x; e < NQ_ACT; e += NQ_WAVES * 64) nq_smem[e] = 0.0f;
    __syncthreads();
    f32_stage_density_params(params, in_dim, nq_smem + NQ_W1, nq_smem + NQ_B1, nq_smem + NQ_W2, nq_smem + NQ_B2, threadIdx.x,
                             NQ_WAVES * 64);
    if (RGB)
        f32_stage_color_params(params, in_dim, nq_smem + NQ_W3, nq_smem + NQ_B3, nq_smem + NQ_W4, nq_smem + NQ_B4, nq_smem + NQ_W5,
                               nq_smem + NQ_B5, threadIdx.x, NQ_WAVES * 64);
    __syncthreads();

    const int64_t ntiles = (n_samples + NQ_TILE - 1) / NQ_TILE;
    for (int64_t tile = (int64_t)blockIdx.x * NQ_WAVES + wave; tile < ntiles; tile += (int64_t)gridDim.x * NQ_WAVES) {
        const int64_t i = tile * NQ_TILE + lane;
        const bool live = i < n_samples;
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (live) { c[0] = coords[i * 3]; c[1] = coords[i * 3 + 1]; c[2] = coords[i * 3 + 2]; }
        // ---- lookup: the live levels two at a time (sixteen gathers in flight per lane), results into the input tile
        float* row = x0 + lane * F32_LDI;
        for (int l = 0; l < live_lods; l += 2) {
            const bool two = l + 1 < live_lods;
            CornerSetup<3> ca, cb;
            float2 va[8], vb[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { va[j] = make_float2(0.0f, 0.0f); vb[j] = make_float2(0.0f, 0.0f); ca.coef[j] = 0.0f; cb.coef[j] = 0.0f; }
            if (live) {
                const int32_t res = lv.res[l];
                const bool dense = lv.dense[l] != 0;
                corner_setup<3>(c, res, lv.hi[l], lv.hr[l], dense, tsize, true, ca);
                if (dense && res >= 258) corner_pin<3>(ca, first_idx[num_lods] - 1 - first_idx[l]);
                corner_gather_f32x2<3>(table + first_idx[l] * 2, ca, va);
                if (two) {
                    const int32_t res1 = lv.res[l + 1];
                    const bool dense1 = lv.dense[l + 1] != 0;
                    corner_setup<3>(c, res1, lv.hi[l + 1], lv.hr[l + 1], dense1, tsize, true, cb);
                    if (dense1 && res1 >= 258) corner_pin<3>(cb, first_idx[num_lods] - 1 - first_idx[l + 1]);
                    corner_gather_f32x2<3>(table + first_idx[l + 1] * 2, cb, vb);
                }
            }
            float a0, a1;
            corner_blend_f32x2<3>(va, ca, a0, a1);
            row[2 * l] = a0; row[2 * l + 1] = a1;
            if (two) {
                corner_blend_f32x2<3>(vb, cb, a0, a1);
                row[2 * l + 2] = a0; row[2 * l + 3] = a1;
            }
        }
        for (int k = 2 * live_lods; k < IN; ++k) row[k] = 0.0f;      // the zeroed finest levels ('cat') and the padding up to IN
        __builtin_amdgcn_wave_barrier();
        // ---- decoder for the tile's two halves of 32 samples; lane (n, half) works on sample `s`
#pragma unroll 1
        for (int part = 0; part < 2; ++part) {
            const float* xp = x0 + part * TS * F32_LDI;
            const int n = lane & 31, half = lane >> 5;
            const int64_t s = tile * NQ_TILE + part * TS + n;
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
            WISP_F32_LAYER1(nq_smem, NQ_W1, nq_smem, NQ_B1, xp, ta, n, lane)
            __builtin_amdgcn_wave_barrier();
            float y0 = 0.0f;
            WISP_F32_LAYER2(nq_smem, NQ_W2, nq_smem, NQ_B2, ta, n, lane, y0, RGB, tb)
            if (half == 0 && alive && out_density) out_density[s] = fmaxf(y0, 0.0f);
            __builtin_amdgcn_wave_barrier();
            if (RGB) {
                // L3: h2 = relu(W3 x2 + b3), B -> A;  L4: h3 = relu(W4 h2 + b4), A -> B;  L5: rgb = sigmoid(W5 h3 + b5)
                WISP_F32_LAYER_HIDDEN(nq_smem, NQ_W3, nq_smem, NQ_B3, F32_K3, tb, ta, n, lane)
                __builtin_amdgcn_wave_barrier();
                WISP_F32_LAYER_HIDDEN(nq_smem, NQ_W4, nq_smem, NQ_B4, H, ta, tb, n, lane)
                __builtin_amdgcn_wave_barrier();
                float sg[3] = {0.f, 0.f, 0.f};
                WISP_F32_LAYER5(nq_smem, NQ_W5, nq_smem, NQ_B5, tb, lane, sg)
                if (half == 0 && alive) { out_rgb[s * 3] = sg[0]; out_rgb[s * 3 + 1] = sg[1]; out_rgb[s * 3 + 2] = sg[2]; }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

int nq_cu_count() {
    static int n = [] { int d = 0, c = 0; (void)hipGetDevice(&d); (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d); return c > 0 ? c : 256; }();
    return n;
}

}  // namespace

extern "C" int wisp_nerf_query(const float* coords, const float* dirs, const int64_t* ridx, int64_t num_rays, int64_t n,
                               const void* table, int dtype_table, int feature_dim, int coord_dim, const int64_t* first_idx,
                               const int32_t* resolutions, int num_lods, int codebook_bitwidth, int zero_from_col,
                               const float* params, int dtype_params, int in_dim, int hidden, float* rgb, float* density,
                               wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "negative sample count");
    if (feature_dim != 2 || coord_dim != 3 || num_lods < 1 || num_lods > 16 || hidden != H || in_dim != num_lods * 2 || in_dim > IN ||
        dtype_table != WISP_F32 || dtype_params != WISP_F32)
        return wisp_fail(WISP_ERR_UNSUPPORTED, "nerf_query",
                         "this build supports feature_dim 2, 3-D, at most 16 levels, hidden 64, in_dim = levels * 2 <= 32, fp32 table and parameters");
    WISP_REQUIRE(codebook_bitwidth >= 1 && codebook_bitwidth <= 30, "codebook_bitwidth out of range");
    WISP_REQUIRE(zero_from_col >= 0 && zero_from_col <= in_dim && zero_from_col % 2 == 0, "zero_from_col must be a whole number of levels");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(coords && table && first_idx && resolutions && params && (rgb || density), "null pointer");
    WISP_REQUIRE(!rgb || dirs, "null pointer");                                   // the colour needs a view direction
    WISP_REQUIRE(!ridx || (dirs && num_rays >= 1), "ridx needs ray_dirs with at least one ray");
    HashLevels lv;
    const int64_t tsize = (int64_t)1 << codebook_bitwidth;
    WISP_REQUIRE(fill_levels(resolutions, num_lods, 3, tsize, lv) == 0, "bad resolution");
    auto kern = rgb ? nerf_query_kernel<true> : nerf_query_kernel<false>;
    const hipError_t e = rgb ? WISP_ALLOW_LDS(nerf_query_kernel<true>, NQ_LDS_BYTES) : WISP_ALLOW_LDS(nerf_query_kernel<false>, NQ_LDS_BYTES);
    if (e != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, "nerf_query", hipGetErrorString(e));
    const int64_t ntiles = ceil_div64(n, NQ_TILE);
    const int grid = (int)min64(ceil_div64(ntiles, NQ_WAVES), nq_cu_count());
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NQ_WAVES * 64), NQ_LDS_BYTES, (hipStream_t)stream, coords, dirs, ridx, num_rays, n,
                       (const float*)table, first_idx, lv, num_lods, zero_from_col / 2, (uint32_t)tsize, in_dim, params, rgb, density);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
