// The 64-samples-per-wave skeleton of a radiance field's one-launch inference query - NeuralRadianceField.rgba
// (wisp/models/nefs/nerf.py:219-264) after and including the grid lookup - written once as a kernel templated over an ENCODER
// policy: parameter staging, the tile loop, the view encoding, the five layers of the exact-fp32 decoder (the stage macros of
// nerf_mlp_f32_dev.h, in the order nerf_query_kernel and nerf_octree_query_kernel expand them) and the stores.  The encoder is what
// differs between grids:
//
//   struct Enc {
//       using Field = ...;                                  // passed to the kernel by value
//       // fill the decoder's input row of ONE sample: row[0 .. width) - the feature columns, zero padded up to `width`; a lane
//       // that is not `live` (behind the last sample) writes zeros and reads nothing
//       static __device__ void encode(const Field&, bool live, float px, float py, float pz, float* row, int width);
//   };
//
// nerf_triplane_query.hip instantiates it.  nerf_query.hip and nerf_octree_query.hip carry their own expansions of the same
// skeleton: their tests pin those files byte for byte, so moving them onto this header is a follow-up.
#pragma once
#include "wisp_common.h"
#include "nerf_mlp_f32_dev.h"

namespace wisp_nfq {

using namespace wisp_mlp;

// one workgroup per CU (LDS), one wave per SIMD, as nerf_query.hip found necessary for the same tiles
constexpr int NFQ_WAVES = 4;
constexpr int NFQ_TILE = 64;              // samples per wave tile: one per lane in the lookup, two MFMA tiles of TS = 32
// LDS (floats), the layout of nerf_query.hip: biases b1 [H], b2 [32], b3 [H], b4 [H], b5 [32]; W1 [H][LDI], W2 [32][LDH],
// W3 [H][LDH], W4 [H][LDH], W5 [32][LDH]; per wave x0 [64][LDI] and two [32][LDH] tiles A and B whose tenants do not overlap:
//   A = h1 (written by L1, dead after L2), then h2 (written by L3, read by L4)
//   B = x2 (view code before L1, geometry features from L2, dead after L3), then h3 (written by L4, read by L5)
constexpr int NFQ_B1 = 0, NFQ_B2 = H, NFQ_B3 = H + 32, NFQ_B4 = 2 * H + 32, NFQ_B5 = 3 * H + 32, NFQ_NBIAS = 3 * H + 64;
constexpr int NFQ_W1 = NFQ_NBIAS, NFQ_W2 = NFQ_W1 + H * F32_LDI, NFQ_W3 = NFQ_W2 + 32 * F32_LDH, NFQ_W4 = NFQ_W3 + H * F32_LDH,
              NFQ_W5 = NFQ_W4 + H * F32_LDH, NFQ_ACT = NFQ_W5 + 32 * F32_LDH;
constexpr int NFQ_X0 = 0, NFQ_A = NFQ_TILE * F32_LDI, NFQ_B = NFQ_A + TS * F32_LDH, NFQ_ACT_WAVE = NFQ_B + TS * F32_LDH;
constexpr size_t NFQ_LDS_BYTES = (size_t)(NFQ_ACT + NFQ_WAVES * NFQ_ACT_WAVE) * 4;
static_assert(NFQ_LDS_BYTES <= 160 * 1024, "one workgroup must fit the CU's LDS");

// RGB = false: the density alone, the kernel stops after layer 2 (no view direction is read).  feats_out (tests): NULL, or
// [n_samples, in_dim] - the decoder's input rows as the encoder left them.
template <typename Enc, bool RGB>
__global__ void __launch_bounds__(NFQ_WAVES * 64, 1)
nerf_field_query_kernel(const float* __restrict__ coords, const float* __restrict__ dirs, const int64_t* __restrict__ ridx,
                        int64_t num_rays, int64_t n_samples, typename Enc::Field fld, int in_dim, const float* __restrict__ params,
                        float* __restrict__ out_rgb, float* __restrict__ out_density, float* __restrict__ feats_out) {
    extern __shared__ __attribute__((aligned(16))) float nfq_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* x0 = nfq_smem + NFQ_ACT + wave * NFQ_ACT_WAVE + NFQ_X0;
    float* ta = nfq_smem + NFQ_ACT + wave * NFQ_ACT_WAVE + NFQ_A;
    float* tb = nfq_smem + NFQ_ACT + wave * NFQ_ACT_WAVE + NFQ_B;

    // ---- stage the parameters: zero everything (padding rows / columns must be 0), then the real entries
    for (int e = threadIdx.x; e < NFQ_ACT; e += NFQ_WAVES * 64) nfq_smem[e] = 0.0f;
    __syncthreads();
    f32_stage_density_params(params, in_dim, nfq_smem + NFQ_W1, nfq_smem + NFQ_B1, nfq_smem + NFQ_W2, nfq_smem + NFQ_B2, threadIdx.x,
                             NFQ_WAVES * 64);
    if (RGB)
        f32_stage_color_params(params, in_dim, nfq_smem + NFQ_W3, nfq_smem + NFQ_B3, nfq_smem + NFQ_W4, nfq_smem + NFQ_B4,
                               nfq_smem + NFQ_W5, nfq_smem + NFQ_B5, threadIdx.x, NFQ_WAVES * 64);
    __syncthreads();

    const int64_t ntiles = (n_samples + NFQ_TILE - 1) / NFQ_TILE;
    for (int64_t tile = (int64_t)blockIdx.x * NFQ_WAVES + wave; tile < ntiles; tile += (int64_t)gridDim.x * NFQ_WAVES) {
        const int64_t i = tile * NFQ_TILE + lane;
        const bool live = i < n_samples;
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (live) { c[0] = coords[i * 3]; c[1] = coords[i * 3 + 1]; c[2] = coords[i * 3 + 2]; }
        // ---- lookup: the sample's feature row (zero padded up to IN) into the input tile
        float* row = x0 + lane * F32_LDI;
        Enc::encode(fld, live, c[0], c[1], c[2], row, IN);
        if (feats_out && live)
            for (int k = 0; k < in_dim; ++k) feats_out[i * in_dim + k] = row[k];
        __builtin_amdgcn_wave_barrier();
        // ---- decoder for the tile's two halves of 32 samples; lane (n, half) works on sample `s`
#pragma unroll 1
        for (int part = 0; part < 2; ++part) {
            const float* xp = x0 + part * TS * F32_LDI;
            const int n = lane & 31, half = lane >> 5;
            const int64_t s = tile * NFQ_TILE + part * TS + n;
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
            WISP_F32_LAYER1(nfq_smem, NFQ_W1, nfq_smem, NFQ_B1, xp, ta, n, lane)
            __builtin_amdgcn_wave_barrier();
            float y0 = 0.0f;
            WISP_F32_LAYER2(nfq_smem, NFQ_W2, nfq_smem, NFQ_B2, ta, n, lane, y0, RGB, tb)
            if (half == 0 && alive && out_density) out_density[s] = fmaxf(y0, 0.0f);
            __builtin_amdgcn_wave_barrier();
            if (RGB) {
                // L3: h2 = relu(W3 x2 + b3), B -> A;  L4: h3 = relu(W4 h2 + b4), A -> B;  L5: rgb = sigmoid(W5 h3 + b5)
                WISP_F32_LAYER_HIDDEN(nfq_smem, NFQ_W3, nfq_smem, NFQ_B3, F32_K3, tb, ta, n, lane)
                __builtin_amdgcn_wave_barrier();
                WISP_F32_LAYER_HIDDEN(nfq_smem, NFQ_W4, nfq_smem, NFQ_B4, H, ta, tb, n, lane)
                __builtin_amdgcn_wave_barrier();
                float sg[3] = {0.f, 0.f, 0.f};
                WISP_F32_LAYER5(nfq_smem, NFQ_W5, nfq_smem, NFQ_B5, tb, lane, sg)
                if (half == 0 && alive) { out_rgb[s * 3] = sg[0]; out_rgb[s * 3 + 1] = sg[1]; out_rgb[s * 3 + 2] = sg[2]; }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static inline int nfq_cu_count() {
    static int n = [] { int d = 0, c = 0; (void)hipGetDevice(&d); (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d); return c > 0 ? c : 256; }();
    return n;
}

// the launch: 4 waves per workgroup, min(ceil(tiles / 4), CU count) workgroups that walk the tiles; n >= 1, arguments checked
template <typename Enc>
static inline int nerf_field_query_launch(const char* fn, const float* coords, const float* dirs, const int64_t* ridx, int64_t num_rays,
                                          int64_t n, const typename Enc::Field& fld, int in_dim, const float* params, float* rgb,
                                          float* density, float* feats_out, hipStream_t stream) {
    auto kern = rgb ? nerf_field_query_kernel<Enc, true> : nerf_field_query_kernel<Enc, false>;
    const hipError_t e = rgb ? WISP_ALLOW_LDS((nerf_field_query_kernel<Enc, true>), NFQ_LDS_BYTES)
                             : WISP_ALLOW_LDS((nerf_field_query_kernel<Enc, false>), NFQ_LDS_BYTES);
    if (e != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, fn, hipGetErrorString(e));
    const int64_t ntiles = ceil_div64(n, NFQ_TILE);
    const int grid = (int)min64(ceil_div64(ntiles, NFQ_WAVES), nfq_cu_count());
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NFQ_WAVES * 64), NFQ_LDS_BYTES, stream, coords, dirs, ridx, num_rays, n, fld, in_dim,
                       params, rgb, density, feats_out);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, fn, hipGetErrorString(le));
    return WISP_OK;
}

}  // namespace wisp_nfq
