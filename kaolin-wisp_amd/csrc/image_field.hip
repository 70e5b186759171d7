// ImageNeuralField.rgb for whole pixel ranges in ONE launch, for gfx950 (MI355X): pixel index -> coordinate -> 2-D multi-resolution
// hash lookup -> 3-octave positional embedding -> Linear + relu -> Linear -> sigmoid, with the colour written as fp32 and / or u8
// and / or compared against the 8-bit ground truth.
//
// Replaces the validation render of wisp/trainers/image_trainer.py:112-119 (1 M-pixel chunks of nef.rgb: lookup, cat, two GEMMs,
// sigmoid - the [n, 46] feature row written to HBM and read back three times) and the float ground truth it is compared with.
// Design:
//   * one pixel per lane, nothing per pixel leaves the registers but the outputs asked for (12 + 3 bytes);
//   * the decoder's weights are wave-uniform: they are read through the scalar unit (16 dwords per s_load) and enter the vector
//     FMAs as their scalar operand - no LDS, no barrier but the one of the error reduction.  The hidden layer is walked in
//     pieces of 32 units (32 accumulators + 46 inputs per lane, hidden 128 = four pieces);
//   * the squared-error partials are summed in a fixed order (lane, wave shuffle tree, wave order) in double - no atomics, so
//     two launches write the same bytes.
// Level arithmetic: corner_setup of hashgrid_dev.h, the library's own.  The gather and the blend of the four corners RESTATE
// the plain path of hashgrid_fwd_kernel (hashgrid.hip: `acc[k] += table[idx[j]][k] * coef[j]`, corners in index order, the
// res >= 258 clamp of dense levels included) without its packed-load special cases, which change no bit.
// The per-pixel forward - level blend, embedding, decoder, sigmoid - lives in image_field_dev.h as __device__ functions, which the
// fused training step (image_field_train.hip) calls as well: a colour is the same bits in both.
// Numerics contract: include/wisp_hip.h (wisp_image_field_render), DESIGN.md section 7.
#include "wisp_common.h"
#include "hashgrid_dev.h"
#include "image_field_dev.h"

#define IF_THREADS 256

// torch.linspace(start, end, steps)[i] in fp32 (aten RangeFactories: two-sided, one fused multiply-add per element)
static __device__ __forceinline__ float linspace_at(float start, float end, float step, int steps, int i) {
#pragma clang fp contract(off)
    if (steps == 1) return start;
    if (i < steps / 2) return __fmaf_rn(step, (float)i, start);
    return __fmaf_rn(-step, (float)(steps - 1 - i), end);
}

struct ImageGrid {
    int h, w;
    float step_x, step_y;                         // fl32(2 / (w - 1)), fl32(-2 / (h - 1))
};

static __device__ __forceinline__ void pixel_coords(const ImageGrid& g, int64_t p, float* __restrict__ c) {
    const int64_t row = p / g.w;
    const int col = (int)(p - row * g.w);
    c[0] = linspace_at(-1.0f, 1.0f, g.step_x, g.w, col);
    c[1] = linspace_at(1.0f, -1.0f, g.step_y, g.h, (int)row);
}

static __device__ __forceinline__ float u8_to_unit(uint8_t v) { return (float)v / 255.0f; }     // IEEE division, not a reciprocal

// ---------------------------------------------------------------------------------------------------- wisp_image_sample
__global__ void __launch_bounds__(256)
image_sample_kernel(const uint8_t* __restrict__ image, ImageGrid g, const int64_t* __restrict__ pix, int64_t n,
                    float* __restrict__ coords, float* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t p = pix[i];
    if (p < 0) p += (int64_t)g.h * g.w;                                   // torch indexing semantics, as wisp_gather_rows
    if (coords) {
        float c[2];
        pixel_coords(g, p, c);
        coords[i * 2] = c[0]; coords[i * 2 + 1] = c[1];
    }
    if (rgb) {
        const uint8_t* __restrict__ t = image + p * 3;
        rgb[i * 3] = u8_to_unit(t[0]); rgb[i * 3 + 1] = u8_to_unit(t[1]); rgb[i * 3 + 2] = u8_to_unit(t[2]);
    }
}

static ImageGrid make_grid(int height, int width) {
    ImageGrid g{};
    g.h = height; g.w = width;
    g.step_x = width > 1 ? 2.0f / (float)(width - 1) : 0.0f;              // (end - start) / (steps - 1), one fp32 division
    g.step_y = height > 1 ? -2.0f / (float)(height - 1) : 0.0f;
    return g;
}

extern "C" int wisp_image_sample(const uint8_t* image, int height, int width, const int64_t* pix, int64_t n, float* coords,
                                 float* rgb, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "negative count");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(height >= 1 && width >= 1, "empty image");
    WISP_REQUIRE(height < (1 << 24) && width < (1 << 24), "image side must be below 2^24");      // (float)index stays exact
    WISP_REQUIRE(pix, "null pixel index");
    WISP_REQUIRE(image || !rgb, "colours need the image");
    WISP_REQUIRE(ceil_div64(n, 256) < ((int64_t)1 << 31), "too many indices for one launch");
    hipLaunchKernelGGL(image_sample_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, (hipStream_t)stream, image,
                       make_grid(height, width), pix, n, coords, rgb);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

// ---------------------------------------------------------------------------------------------------- wisp_image_field_render
// weights: [IF_IN][hp] first layer, transposed (row k = the weights of input k for every hidden unit) | b1 [hp] | W2 [3][hp] | b2 [3]
// hp = hidden width padded to a multiple of IF_PIECE with zero columns (a padded unit is relu(0) * 0).
__global__ void __launch_bounds__(IF_THREADS)
image_field_render_kernel(const float* __restrict__ coords, int64_t first, int64_t n, ImageGrid g,
                          const float* __restrict__ codebook, const int64_t* __restrict__ first_idx, HashLevels lv, int num_lods,
                          int active_lods, uint32_t tsize, int tsize_pow2, const float* __restrict__ weights, int hp,
                          const uint8_t* __restrict__ gts, float* __restrict__ out_f32, uint8_t* __restrict__ out_u8,
                          double* __restrict__ err_partial) {
    const int64_t i = (int64_t)blockIdx.x * IF_THREADS + threadIdx.x;
    const bool live = i < n;
    float x[IF_IN];
    float c[2] = {0.0f, 0.0f};
    if (live) {
        if (coords) { c[0] = coords[i * 2]; c[1] = coords[i * 2 + 1]; }
        else pixel_coords(g, first + i, c);
    }
    // ---- grid features of the active levels ('cat': column 2 l, 2 l + 1), zero beyond them
#pragma unroll
    for (int l = 0; l < IF_MAX_LODS; ++l) {
        float acc[2] = {0.0f, 0.0f};
        if (l < active_lods && live) {
            CornerSetup<2> cs;
            image_level_corners(c, lv.res[l], lv.hi[l], lv.hr[l], lv.dense[l] != 0, tsize, tsize_pow2 != 0, first_idx[l],
                                first_idx[num_lods], cs);
            image_level_blend(codebook + first_idx[l] * 2, cs, acc);
        }
        x[2 * l] = acc[0]; x[2 * l + 1] = acc[1];
    }
    // ---- positional embedding, then the decoder and the sigmoid (image_field_dev.h)
    image_embed(c, x + 2 * IF_MAX_LODS);
    float o[3];
    image_decode_packed(x, weights, hp, o);
    float col[3] = {image_sigmoid(o[0]), image_sigmoid(o[1]), image_sigmoid(o[2])};
    double err = 0.0;
    if (live) {
        if (out_f32) { out_f32[i * 3] = col[0]; out_f32[i * 3 + 1] = col[1]; out_f32[i * 3 + 2] = col[2]; }
        if (out_u8) {
#pragma unroll
            for (int k = 0; k < 3; ++k) out_u8[i * 3 + k] = (uint8_t)(col[k] * 255.0f);           // truncating, (img * 255).byte()
        }
        if (err_partial) {
#pragma clang fp contract(off)
            const uint8_t* __restrict__ t = gts + (first + i) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float d = col[k] - u8_to_unit(t[k]);
                const float sq = d * d;
                err += (double)sq;
            }
        }
    }
    if (err_partial) {                                                      // (kernel argument: uniform for the whole grid)
        __shared__ double wave_sum[IF_THREADS / 64];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) err += __shfl_xor(err, off, 64);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = err;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = wave_sum[0];
#pragma unroll
            for (int k = 1; k < IF_THREADS / 64; ++k) s += wave_sum[k];
            err_partial[blockIdx.x] = s;
        }
    }
}

extern "C" int64_t wisp_image_field_render_partials(int64_t n) { return n > 0 ? ceil_div64(n, IF_THREADS) : 0; }

extern "C" int wisp_image_field_render(const float* coords, int64_t first, int64_t n, int height, int width, const float* codebook,
                                       const int64_t* first_idx, const int32_t* resolutions, int num_lods, int active_lods,
                                       int codebook_bitwidth, const float* weights, int hidden_padded, const uint8_t* gts,
                                       float* out_f32, uint8_t* out_u8, double* err_partials, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0 && first >= 0, "negative range");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(codebook && first_idx && resolutions && weights, "null pointer");
    WISP_REQUIRE(num_lods >= 1 && num_lods <= IF_MAX_LODS, "num_lods must be in 1..16");
    WISP_REQUIRE(active_lods >= 0 && active_lods <= num_lods, "active_lods out of range");
    WISP_REQUIRE(codebook_bitwidth >= 1 && codebook_bitwidth <= 30, "codebook_bitwidth out of range");
    WISP_REQUIRE(hidden_padded >= IF_PIECE && hidden_padded <= 128 && hidden_padded % IF_PIECE == 0,
                 "hidden width must be padded to a multiple of 32, at most 128");
    WISP_REQUIRE(((uintptr_t)weights & 63) == 0, "weights must be 64-byte aligned");
    WISP_REQUIRE(((uintptr_t)codebook & 7) == 0, "codebook must be 8-byte aligned");
    WISP_REQUIRE(height >= 1 && width >= 1 && height < (1 << 24) && width < (1 << 24), "image side must be in 1 .. 2^24 - 1");
    WISP_REQUIRE(coords || first + n <= (int64_t)height * width, "pixel range leaves the image");
    WISP_REQUIRE(gts || !err_partials, "error sums need the ground-truth image");
    WISP_REQUIRE(out_f32 || out_u8 || err_partials, "no output asked for");
    const int64_t blocks = ceil_div64(n, IF_THREADS);
    WISP_REQUIRE(blocks < ((int64_t)1 << 31), "range too long for one launch");
    HashLevels lv;
    const int64_t tsize = (int64_t)1 << codebook_bitwidth;
    WISP_REQUIRE(fill_levels(resolutions, num_lods, 2, tsize, lv) == 0, "bad resolution");
    const int pow2 = 1;
    hipLaunchKernelGGL(image_field_render_kernel, dim3((unsigned)blocks), dim3(IF_THREADS), 0, (hipStream_t)stream, coords, first, n,
                       make_grid(height, width), codebook, first_idx, lv, num_lods, active_lods, (uint32_t)tsize, pow2, weights,
                       hidden_padded, gts, out_f32, out_u8, err_partials);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
