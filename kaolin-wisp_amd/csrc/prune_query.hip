// The density query of the occupancy prune (NeuralRadianceField.prune, wisp/models/nefs/nerf.py:175-212) as ONE launch.
//
// The modular path runs, per prune of the 128^3 cells of nerf_hash.yaml: five elementwise passes for the sample positions, the fp32
// hash-grid lookup (a [cells, 32] feature tensor, 268 MB, written and read back), the whole exact-fp32 decoder (view-direction
// encoding with 24 sinf / cosf per sample, five layers) and three more elementwise passes for the occupancy and the mask - and
// consumes the density alone, which is relu of output 0 of the SECOND layer.  Here a wave takes 64 cells: every lane computes its
// cell's sample position and walks the live levels (wave-uniform, as in hashgrid_fwd_kernel), the blended features go straight into
// the decoder's input tile in the wave's LDS slice, layers 1 and 2 run on the matrix cores for the tile's two halves of 32 samples
// (nerf_mlp_f32_dev.h: the stages of nerf_mlp_kernel<float, ...>), and the lanes that hold output 0 write the new occupancy and
// the keep mask.  Every value is the bits the modular path computes: the position is rounded where torch rounds it, the lookup is
// corner_setup + the forward kernel's fmaf chain, the decoder is the shared MFMA sequence.
#include "wisp_common.h"
#include "hashgrid_dev.h"
#include "nerf_mlp_f32_dev.h"

namespace {

using namespace wisp_mlp;

constexpr int PQ_WAVES = 8;               // one workgroup per CU (LDS), two waves per SIMD
constexpr int PQ_TILE = 64;               // cells per wave tile: one per lane in the lookup, two MFMA tiles of TS = 32
// LDS (floats): b1 [H], b2 [32]; W1 [H][LDI], W2 [32][LDH]; per wave x0 [64][LDI], h1 [32][LDH]
constexpr int PQ_B1 = 0, PQ_B2 = H, PQ_W1 = H + 32, PQ_W2 = PQ_W1 + H * F32_LDI, PQ_ACT = PQ_W2 + 32 * F32_LDH;
constexpr int PQ_X0 = 0, PQ_H1 = PQ_TILE * F32_LDI, PQ_ACT_WAVE = PQ_H1 + TS * F32_LDH;
constexpr size_t PQ_LDS_BYTES = (size_t)(PQ_ACT + PQ_WAVES * PQ_ACT_WAVE) * 4;
static_assert(PQ_LDS_BYTES <= 160 * 1024, "one workgroup must fit the CU's LDS");

// DEBUG: also writes the decoder's input tile (feats [cells, in_dim]) and the density (test-only entry point)
template <bool DEBUG>
__global__ void __launch_bounds__(PQ_WAVES * 64, 1)
prune_query_kernel(const int16_t* __restrict__ points, const float* __restrict__ unit, int64_t cells, float scale,
                   const float* __restrict__ table, const int64_t* __restrict__ first_idx, HashLevels lv, int num_lods,
                   int live_lods, uint32_t tsize, int in_dim, const float* __restrict__ params,
                   const float* __restrict__ occ_in, float decay, float min_density, float* __restrict__ occ_out,
                   uint8_t* __restrict__ keep, float* __restrict__ dbg_feats, float* __restrict__ dbg_density) {
    extern __shared__ __attribute__((aligned(16))) float pq_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* x0 = pq_smem + PQ_ACT + wave * PQ_ACT_WAVE + PQ_X0;
    float* h1 = pq_smem + PQ_ACT + wave * PQ_ACT_WAVE + PQ_H1;

    // ---- stage the density network's parameters: zero everything (padding rows / columns must be 0), then the real entries
    for (int e = threadIdx.x; e < PQ_ACT; e += PQ_WAVES * 64) pq_smem[e] = 0.0f;
    __syncthreads();
    f32_stage_density_params(params, in_dim, pq_smem + PQ_W1, pq_smem + PQ_B1, pq_smem + PQ_W2, pq_smem + PQ_B2, threadIdx.x,
                             PQ_WAVES * 64);
    __syncthreads();

    const int64_t ntiles = (cells + PQ_TILE - 1) / PQ_TILE;
    for (int64_t tile = (int64_t)blockIdx.x * PQ_WAVES + wave; tile < ntiles; tile += (int64_t)gridDim.x * PQ_WAVES) {
        const int64_t i = tile * PQ_TILE + lane;
        const bool live = i < cells;
        // ---- sample position ((p + u) / res) * 2 - 1 as torch rounds it: one rounding for the sum, the two scalings by powers of
        // two are exact (`scale` = 2 / res), one rounding for the difference
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (live) {
#pragma clang fp contract(off)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float s = (float)points[i * 3 + a] + unit[i * 3 + a];
                const float t = s * scale;
                c[a] = t - 1.0f;
            }
        }
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
        if (DEBUG && live)
            for (int k = 0; k < in_dim; ++k) dbg_feats[i * in_dim + k] = row[k];
        // ---- decoder, layers 1 and 2, for the tile's two halves of 32 samples; output 0 lands in the lanes below 32
#pragma unroll 1
        for (int part = 0; part < 2; ++part) {
            const float* xp = x0 + part * TS * F32_LDI;
            const int n = lane & 31;
            WISP_F32_LAYER1(pq_smem, PQ_W1, pq_smem, PQ_B1, xp, h1, n, lane)
            __builtin_amdgcn_wave_barrier();
            float y0 = 0.0f;
            WISP_F32_LAYER2(pq_smem, PQ_W2, pq_smem, PQ_B2, h1, n, lane, y0, false, h1)
            __builtin_amdgcn_wave_barrier();
            const int64_t s = tile * PQ_TILE + part * TS + (lane & 31);
            if (lane < 32 && s < cells) {
                const float density = fmaxf(y0, 0.0f);
                const float old = occ_in[s] * decay;
                float occ = fmaxf(density, old);                     // torch.maximum: a NaN on either side is the result
                if (density != density) occ = density; else if (old != old) occ = old;
                occ_out[s] = occ;
                keep[s] = occ > min_density ? 1 : 0;
                if (DEBUG) dbg_density[s] = density;
            }
        }
    }
}

int pq_cu_count() {
    static int n = [] { int d = 0, c = 0; (void)hipGetDevice(&d); (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d); return c > 0 ? c : 256; }();
    return n;
}

int prune_query(const int16_t* points, const float* unit, int64_t cells, int level, const void* table, int dtype_table,
                int feature_dim, int coord_dim, const int64_t* first_idx, const int32_t* resolutions, int num_lods,
                int codebook_bitwidth, int zero_from_col, const float* params, int dtype_params, int in_dim, int hidden,
                const float* occ_in, float decay, float min_density, float* occ_out, uint8_t* keep, float* dbg_feats,
                float* dbg_density, bool debug, wisp_stream_t stream) {
    WISP_REQUIRE(cells >= 0, "negative cell count");
    if (feature_dim != 2 || coord_dim != 3 || num_lods < 1 || num_lods > 16 || hidden != H || in_dim != num_lods * 2 || in_dim > IN ||
        dtype_table != WISP_F32 || dtype_params != WISP_F32)
        return wisp_fail(WISP_ERR_UNSUPPORTED, "nerf_prune_query",
                         "this build supports feature_dim 2, 3-D, at most 16 levels, hidden 64, in_dim = levels * 2 <= 32, fp32 table and parameters");
    WISP_REQUIRE(level >= 0 && level <= 14, "level out of range");               // int16 cell coordinates
    WISP_REQUIRE(codebook_bitwidth >= 1 && codebook_bitwidth <= 30, "codebook_bitwidth out of range");
    WISP_REQUIRE(zero_from_col >= 0 && zero_from_col <= in_dim && zero_from_col % 2 == 0, "zero_from_col must be a whole number of levels");
    if (cells == 0) return WISP_OK;
    WISP_REQUIRE(points && unit && table && first_idx && resolutions && params && occ_in && occ_out && keep, "null pointer");
    WISP_REQUIRE(!debug || (dbg_feats && dbg_density), "null pointer");
    HashLevels lv;
    const int64_t tsize = (int64_t)1 << codebook_bitwidth;
    WISP_REQUIRE(fill_levels(resolutions, num_lods, 3, tsize, lv) == 0, "bad resolution");
    auto kern = debug ? prune_query_kernel<true> : prune_query_kernel<false>;
    const hipError_t e = debug ? WISP_ALLOW_LDS(prune_query_kernel<true>, PQ_LDS_BYTES) : WISP_ALLOW_LDS(prune_query_kernel<false>, PQ_LDS_BYTES);
    if (e != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, "nerf_prune_query", hipGetErrorString(e));
    const int64_t ntiles = ceil_div64(cells, PQ_TILE);
    const int grid = (int)min64(ceil_div64(ntiles, PQ_WAVES), pq_cu_count());
    const float scale = ldexpf(1.0f, 1 - level);                                 // 2 / res, res = 2^level
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PQ_WAVES * 64), PQ_LDS_BYTES, (hipStream_t)stream, points, unit, cells, scale,
                       (const float*)table, first_idx, lv, num_lods, zero_from_col / 2, (uint32_t)tsize, in_dim, params, occ_in, decay,
                       min_density, occ_out, keep, dbg_feats, dbg_density);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

}  // namespace

extern "C" int wisp_nerf_prune_query(const int16_t* dense_points, const float* unit_samples, int64_t cells, int level,
                                     const void* table, int dtype_table, int feature_dim, int coord_dim, const int64_t* first_idx,
                                     const int32_t* resolutions, int num_lods, int codebook_bitwidth, int zero_from_col,
                                     const float* params, int dtype_params, int in_dim, int hidden, const float* occ_in, float decay,
                                     float min_density, float* occ_out, uint8_t* keep, wisp_stream_t stream) {
    return prune_query(dense_points, unit_samples, cells, level, table, dtype_table, feature_dim, coord_dim, first_idx, resolutions,
                       num_lods, codebook_bitwidth, zero_from_col, params, dtype_params, in_dim, hidden, occ_in, decay, min_density,
                       occ_out, keep, nullptr, nullptr, false, stream);
}

extern "C" int wisp_nerf_prune_query_debug(const int16_t* dense_points, const float* unit_samples, int64_t cells, int level,
                                           const void* table, int dtype_table, int feature_dim, int coord_dim,
                                           const int64_t* first_idx, const int32_t* resolutions, int num_lods, int codebook_bitwidth,
                                           int zero_from_col, const float* params, int dtype_params, int in_dim, int hidden,
                                           const float* occ_in, float decay, float min_density, float* occ_out, uint8_t* keep,
                                           float* feats, float* density, wisp_stream_t stream) {
    return prune_query(dense_points, unit_samples, cells, level, table, dtype_table, feature_dim, coord_dim, first_idx, resolutions,
                       num_lods, codebook_bitwidth, zero_from_col, params, dtype_params, in_dim, hidden, occ_in, decay, min_density,
                       occ_out, keep, feats, density, true, stream);
}
