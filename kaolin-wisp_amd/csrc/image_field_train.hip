// One optimisation step's forward + loss + backward of the reference's ImageTrainer (wisp/trainers/image_trainer.py:52-84, `step`)
// for an ImageNeuralField over a 2-D HashGrid (wisp/models/nefs/image_nef.py:66-97 over wisp/models/grids/hash_grid.py:205-233;
// image_hash.yaml: 'cat', 16 levels x 2 features, [features, 14 embedding values] -> Linear(46, 64) -> relu -> Linear(64, 3) ->
// sigmoid, 4096 pixels per step):
//     pred = sigmoid(decoder([features(x), embed(x)])) ;  loss = F.mse_loss(pred, rgb) = sum (pred - rgb)^2 / (3 n) ;  backward
// The image twin of wisp_hash_sdf_train_step (hash_sdf_train.hip).  Through autograd over the modular ops the step is a 2-D hash
// lookup, the embedder's sin / cos / cat ops, a concatenation, two GEMMs with their elementwise companions, a sigmoid, the loss, and
// all of that again backwards - about thirty launches of launch latency at 4096 pixels.  Here, two launches (and one memset):
//   image_field_train_kernel         16 lanes own a sample, 16 samples a workgroup pass.  The decoder arrives in torch's native layout
//                                    and is staged into LDS once per workgroup (rows padded to an odd stride: the 16 lanes of a
//                                    group read 16 different rows).  Forward, with the __device__ functions of image_field_dev.h
//                                    that wisp_image_field_render is made of: lane c blends level c (active levels only) and
//                                    keeps its corner rows and blend factors in registers, lanes 0..5 form the embedding; lane c
//                                    walks hidden units c, c + 16, ... - a unit starts at its bias and takes one fma per input in
//                                    column order, active feature columns first, then the 14 embedding values; lanes 0..2 walk
//                                    one output each over the hidden units in ascending order and take the sigmoid: the colour is
//                                    bit for bit the render kernel's.  Then d = s - t, g = 2 d / (float)(3 n) (an IEEE
//                                    division), dO = g * (s * (1 - s)); d hidden = (dO . W2 column) on the units whose
//                                    pre-activation is positive, d feature column = sum over units - both in fp64, rounded once.
//                                    The table gradient is scattered right there by the lane that blended the level, to the
//                                    corner rows it still holds (the forward's bits, the dense-level pin included).  Per
//                                    workgroup the decoder's weight gradients and the squared error are summed by the thread
//                                    that owns the entry, in sample order, in fp64, and stored as one fp64 partial row - no atomics.
//   image_field_train_reduce_kernel  adds the partial rows up in workgroup order in fp64, rounds once, ADDS the sums to the decoder's
//                                    gradient tensors (native layout) and writes the loss.
// Table gradient.  At 4096 pixels x 15 levels x 4 corners x 8 B the scatter adds about 2 MB, small against the chip-wide atomic
// rate; what matters is where the terms meet: resolution 16 reaches 256 rows with 16 384 terms.  A level whose indices reach at most
// 2^16 table entries takes its gradient through fp64 accumulators in scratch (IftWide below, hash_sdf_train.hip's scheme): exact fp64 products, fp64
// atomic adds, one rounding per entry in the reduce kernel; the step zeroes the accumulators it will use with one memset.  Larger
// levels - at most one term per two rows on average - take f32 atomic adds (global_atomic_add_f32 under -munsafe-fp-atomics), as
// the reference's backward (hashgrid_interpolate_cuda.cu) does on every level.
// Determinism: the loss and the four decoder gradients have a fixed summation order and are bitwise repeatable; the table gradient
// depends on arrival order only in the last bits of its fp64 sums (small levels) or its f32 sums (large ones).
#include "wisp_common.h"
#include "image_field_dev.h"

#define IFT_BLOCK 256
#define IFT_GROUP 16                                   // lanes per sample
#define IFT_GROUPS (IFT_BLOCK / IFT_GROUP)             // samples per workgroup pass
#define IFT_MAX_GRID 256                               // workgroups = partial rows: one per compute unit
#define IFT_MAX_LDS (160 * 1024)                       // one workgroup may hold the whole LDS of a compute unit
#define IFT_WIDE_ENTRIES (1 << 16)                     // a level of at most this many table entries is summed in fp64
#define IFT_MAX_N ((int64_t)1 << 22)                   // (float)(3 n) stays exact

struct ImageTrainField {
    const float* codebook;
    int64_t begin[IF_MAX_LODS + 1];                    // first row of every level, rows of the table
    HashLevels lv;
    int num_lods, active_lods;
    uint32_t tsize;
    const float *w1, *b1, *w2, *b2;                    // torch's native layout: [H][2 L + 14], [H], [3][H], [3]
    int hidden;
};

// off[i] .. off[i + 1]: fp64 accumulators of the i-th small level, tbl[i]: its first entry in the table, lvl[l]: the position of
// level l in that list or -1
struct IftWide {
    int64_t off[IF_MAX_LODS + 1];
    int64_t tbl[IF_MAX_LODS];
    int32_t lvl[IF_MAX_LODS];
    int n;
};

// entries of a partial row: d W1 [H][in_dim], d b1 [H], d W2 [3][H], d b2 [3], sum of squares - in that order
static inline int ift_entries(int hidden, int num_lods) { return hidden * (2 * num_lods + IF_EMBED) + 4 * hidden + 4; }
static inline int ift_row_stride(int hidden, int num_lods) { return (ift_entries(hidden, num_lods) + 15) / 16 * 16; }
static inline int ift_grid(int64_t n) { return (int)min64(ceil_div64(n, IFT_GROUPS), IFT_MAX_GRID); }
// LDS of a workgroup: the partial row (fp64) | W1 [H][in_dim | 1] | b1 [H] | W2 [3][H] | b2 [4] | per group: inputs [in_dim], relu
// output [H], d hidden [H], d output [4], squares [4], d feature column [32]
static inline size_t ift_lds_bytes(int hidden, int num_lods) {
    const int in_dim = 2 * num_lods + IF_EMBED;
    return (size_t)ift_row_stride(hidden, num_lods) * sizeof(double) +
           ((size_t)hidden * (in_dim | 1) + 4 * hidden + 4 + (size_t)IFT_GROUPS * (in_dim + 2 * hidden + 8 + 2 * IF_MAX_LODS)) * sizeof(float);
}
// the largest admitted shape, hidden 128 over 16 levels: 51328 (partial row) + 24064 (W1) + 2064 + 21888 = 99344 bytes
static_assert(((IF_MAX_HIDDEN * IF_IN + 4 * IF_MAX_HIDDEN + 4 + 15) / 16 * 16) * sizeof(double) +
              ((size_t)IF_MAX_HIDDEN * (IF_IN | 1) + 4 * IF_MAX_HIDDEN + 4 + (size_t)IFT_GROUPS * (IF_IN + 2 * IF_MAX_HIDDEN + 8 + 2 * IF_MAX_LODS)) *
              sizeof(float) <= IFT_MAX_LDS, "the largest shape must fit one workgroup's LDS");

__global__ void __launch_bounds__(IFT_BLOCK)
image_field_train_kernel(const float* __restrict__ coords, const float* __restrict__ rgb, int64_t n, ImageTrainField fld, float denom,
                         float* __restrict__ grad_codebook, double* __restrict__ partials /* [grid][row] */, int row_stride,
                         IftWide wide, double* __restrict__ wacc, float* __restrict__ pred) {
    extern __shared__ double s_ift[];
    const int H = fld.hidden, L2 = 2 * fld.num_lods, act2 = 2 * fld.active_lods;
    const int in_dim = L2 + IF_EMBED, in_pad = in_dim | 1;
    const int n_entries = H * in_dim + 4 * H + 4;
    double* s_own = s_ift;                                      // [row_stride]   this workgroup's partial sums, one owner per entry
    float* s_w1 = reinterpret_cast<float*>(s_own + row_stride); // [H][in_pad]
    float* s_b1 = s_w1 + H * in_pad;                            // [H]
    float* s_w2 = s_b1 + H;                                     // [3][H]
    float* s_b2 = s_w2 + 3 * H;                                 // [4]
    float* s_x = s_b2 + 4;                                      // [groups][in_dim]   decoder inputs
    float* s_a = s_x + IFT_GROUPS * in_dim;                     // [groups][H]        relu output
    float* s_dh = s_a + IFT_GROUPS * H;                         // [groups][H]        d loss / d pre-activation
    float* s_do = s_dh + IFT_GROUPS * H;                        // [groups][4]        d loss / d output (before the sigmoid)
    float* s_sq = s_do + IFT_GROUPS * 4;                        // [groups][4]        squared errors
    float* s_dx = s_sq + IFT_GROUPS * 4;                        // [groups][32]       d loss / d feature column
    for (int e = threadIdx.x; e < H * in_dim; e += IFT_BLOCK) {
        const int hh = e / in_dim, k = e - hh * in_dim;
        s_w1[hh * in_pad + k] = fld.w1[e];
    }
    for (int e = threadIdx.x; e < H; e += IFT_BLOCK) s_b1[e] = fld.b1[e];
    for (int e = threadIdx.x; e < 3 * H; e += IFT_BLOCK) s_w2[e] = fld.w2[e];
    if (threadIdx.x < 3) s_b2[threadIdx.x] = fld.b2[threadIdx.x];
    for (int e = threadIdx.x; e < n_entries; e += IFT_BLOCK) s_own[e] = 0.0;
    const int c = threadIdx.x & (IFT_GROUP - 1), grp = threadIdx.x / IFT_GROUP;
    float* gx = s_x + grp * in_dim;
    float* ga = s_a + grp * H;
    float* gdh = s_dh + grp * H;
    float* gdo = s_do + grp * 4;
    float* gsq = s_sq + grp * 4;
    float* gdx = s_dx + grp * (2 * IF_MAX_LODS);
    const int64_t rounds = (n + IFT_GROUPS - 1) / IFT_GROUPS;
    __syncthreads();
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * IFT_GROUPS + grp;
        if (i < n) {                                     // (a group enters or stays out as a whole)
            const float xy[2] = {coords[i * 2], coords[i * 2 + 1]};
            // ---- forward: wisp_image_field_render's colour
            const bool blends = c < fld.active_lods;     // lane c owns level c
            CornerSetup<2> cs;
            if (blends) {
                float acc[2];
                image_level_corners(xy, fld.lv.res[c], fld.lv.hi[c], fld.lv.hr[c], fld.lv.dense[c] != 0, fld.tsize, true, fld.begin[c],
                                    fld.begin[fld.num_lods], cs);
                image_level_blend(fld.codebook + fld.begin[c] * 2, cs, acc);
                gx[2 * c] = acc[0]; gx[2 * c + 1] = acc[1];
            } else if (c < fld.num_lods) {               // a level that is not blended: 'cat' leaves its columns zero
                gx[2 * c] = 0.0f; gx[2 * c + 1] = 0.0f;
            }
            if (c < 6) image_embed_pair(xy, c, gx[L2 + 2 + c], gx[L2 + 8 + c]);
            if (c < 2) gx[L2 + c] = xy[c];
            __builtin_amdgcn_wave_barrier();             // a group's lanes are in one wave: LDS order suffices
            for (int hh = c; hh < H; hh += IFT_GROUP) {
                const float* __restrict__ w = s_w1 + hh * in_pad;
                float acc = s_b1[hh];
                for (int k = 0; k < act2; ++k) acc = image_fma(gx[k], w[k], acc);
                for (int k = L2; k < in_dim; ++k) acc = image_fma(gx[k], w[k], acc);
                ga[hh] = image_relu(acc);
                gdh[hh] = acc > 0.0f ? 1.0f : 0.0f;      // (the relu's derivative; replaced by d hidden below)
            }
            __builtin_amdgcn_wave_barrier();
            if (c < 3) {
                const float* __restrict__ u = s_w2 + c * H;
                float o = s_b2[c];
                for (int hh = 0; hh < H; ++hh) o = image_fma(ga[hh], u[hh], o);
                const float s = image_sigmoid(o);
                {
#pragma clang fp contract(off)
                    const float d = s - rgb[i * 3 + c];
                    const float g = 2.0f * d / denom;    // d [sum (s - t)^2 / (3 n)] / d s, an IEEE division
                    gdo[c] = g * (s * (1.0f - s));
                    gsq[c] = d * d;
                }
                if (pred) pred[i * 3 + c] = s;
            }
            __builtin_amdgcn_wave_barrier();
            // ---- decoder backward: sums over outputs and hidden units in fp64 (a product of two floats is exact there), rounded once
            for (int hh = c; hh < H; hh += IFT_GROUP) {
                double v = (double)gdo[0] * (double)s_w2[hh];
                v = __builtin_fma((double)gdo[1], (double)s_w2[H + hh], v);
                v = __builtin_fma((double)gdo[2], (double)s_w2[2 * H + hh], v);
                gdh[hh] = gdh[hh] != 0.0f ? (float)v : 0.0f;
            }
            __builtin_amdgcn_wave_barrier();
            for (int col = c; col < act2; col += IFT_GROUP) {      // nothing consumes d / d coordinate: feature columns only
                double dx0 = 0.0, dx1 = 0.0;
                int hh = 0;
                for (; hh + 1 < H; hh += 2) {
                    dx0 = __builtin_fma((double)gdh[hh], (double)s_w1[hh * in_pad + col], dx0);
                    dx1 = __builtin_fma((double)gdh[hh + 1], (double)s_w1[(hh + 1) * in_pad + col], dx1);
                }
                if (hh < H) dx0 = __builtin_fma((double)gdh[hh], (double)s_w1[hh * in_pad + col], dx0);
                gdx[col] = (float)(dx0 + dx1);
            }
            __builtin_amdgcn_wave_barrier();
            // ---- table gradient: the lane that blended a level scatters to the corner rows it read
            if (blends) {
                const float d0 = gdx[2 * c], d1 = gdx[2 * c + 1];
                const int wl = wide.lvl[c];
                if (wl >= 0) {                           // a small level: exact fp64 products into its fp64 accumulators
                    double* __restrict__ base = wacc + wide.off[wl];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        double* p = base + (int64_t)(uint32_t)cs.idx[j] * 2;
                        const double v0 = (double)cs.coef[j] * (double)d0, v1 = (double)cs.coef[j] * (double)d1;
                        if (v0 != 0.0) atomicAdd(p, v0);             // global_atomic_add_f64
                        if (v1 != 0.0) atomicAdd(p + 1, v1);
                    }
                } else {
                    float* __restrict__ base = grad_codebook + fld.begin[c] * 2;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
                        float* p = base + (int64_t)(uint32_t)cs.idx[j] * 2;
                        const float v0 = cs.coef[j] * d0, v1 = cs.coef[j] * d1;
                        if (v0 != 0.0f) atomicAdd(p, v0);            // global_atomic_add_f32
                        if (v1 != 0.0f) atomicAdd(p + 1, v1);
                    }
                }
            }
        } else {
            for (int hh = c; hh < H; hh += IFT_GROUP) { ga[hh] = 0.0f; gdh[hh] = 0.0f; }
            for (int e = c; e < in_dim; e += IFT_GROUP) gx[e] = 0.0f;
            if (c < 4) { gdo[c] = 0.0f; gsq[c] = 0.0f; }
        }
        __syncthreads();
        // ---- weight gradients and the squared error of this pass: the thread that owns an entry adds the samples up in order
        for (int e = threadIdx.x; e < n_entries; e += IFT_BLOCK) {
            double acc = 0.0;
            if (e < H * in_dim) {
                const int hh = e / in_dim, k = e - hh * in_dim;
                for (int q = 0; q < IFT_GROUPS; ++q) acc = __builtin_fma((double)s_dh[q * H + hh], (double)s_x[q * in_dim + k], acc);
            } else if (e < H * in_dim + H) {
                const int hh = e - H * in_dim;
                for (int q = 0; q < IFT_GROUPS; ++q) acc += (double)s_dh[q * H + hh];
            } else if (e < H * in_dim + 4 * H) {
                const int r = e - H * in_dim - H, k = r / H, hh = r - k * H;
                for (int q = 0; q < IFT_GROUPS; ++q) acc = __builtin_fma((double)s_do[q * 4 + k], (double)s_a[q * H + hh], acc);
            } else if (e < H * in_dim + 4 * H + 3) {
                const int k = e - H * in_dim - 4 * H;
                for (int q = 0; q < IFT_GROUPS; ++q) acc += (double)s_do[q * 4 + k];
            } else {
                for (int q = 0; q < IFT_GROUPS; ++q) acc += ((double)s_sq[q * 4] + (double)s_sq[q * 4 + 1]) + (double)s_sq[q * 4 + 2];
            }
            s_own[e] += acc;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < n_entries; e += IFT_BLOCK) partials[(int64_t)blockIdx.x * row_stride + e] = s_own[e];
}

__global__ void __launch_bounds__(256)
image_field_train_reduce_kernel(const double* __restrict__ partials, int rows, int row_stride, int H, int in_dim, float* __restrict__ gw1,
                                float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2, float* __restrict__ loss,
                                double count /* 3 n */, IftWide wide, const double* __restrict__ wacc, float* __restrict__ grad_codebook) {
    // 16 lanes per entry: lane r adds rows r, r + 16, ... in order, then a fixed butterfly over the 16 lanes - in fp64, rounded once
    const int n_entries = H * in_dim + 4 * H + 4;
    const int r0 = threadIdx.x & 15;
    for (int e = blockIdx.x * 16 + (threadIdx.x >> 4); e < n_entries + 15; e += gridDim.x * 16) {      // (whole groups stay together)
        const bool in = e < n_entries;
        double sum = 0.0;
        if (in)
            for (int r = r0; r < rows; r += 16) sum += partials[(int64_t)r * row_stride + e];
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 16);
        if (!in || r0 != 0) continue;
        if (e < H * in_dim) gw1[e] += (float)sum;
        else if (e < H * in_dim + H) gb1[e - H * in_dim] += (float)sum;
        else if (e < H * in_dim + 4 * H) gw2[e - H * in_dim - H] += (float)sum;
        else if (e < H * in_dim + 4 * H + 3) gb2[e - H * in_dim - 4 * H] += (float)sum;
        else loss[0] = (float)(sum / count);
    }
    // the small levels' fp64 sums, rounded once and ADDED to the table gradient (an untouched accumulator leaves its entry alone)
    const int64_t total = wide.off[wide.n];
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const double v = wacc[e];
        if (v == 0.0) continue;
        int i = 0;
        while (e >= wide.off[i + 1]) ++i;
        grad_codebook[wide.tbl[i] + (e - wide.off[i])] += (float)v;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
extern "C" int64_t wisp_image_field_train_scratch_bytes(int64_t n, int num_lods, int hidden) {
    if (n < 1 || n > IFT_MAX_N || num_lods < 1 || num_lods > IF_MAX_LODS || hidden < 1 || hidden > IF_MAX_HIDDEN) return -1;
    if (ift_lds_bytes(hidden, num_lods) > IFT_MAX_LDS) return -1;
    // the fp64 partial rows, then room for every level's fp64 accumulators (which levels are small depends on the resolutions)
    return (int64_t)ift_grid(n) * ift_row_stride(hidden, num_lods) * (int64_t)sizeof(double) +
           (int64_t)num_lods * IFT_WIDE_ENTRIES * (int64_t)sizeof(double);
}

extern "C" int wisp_image_field_train_step(const float* coords, const float* rgb, int64_t n, const float* codebook,
                                           const int64_t* first_idx, const int32_t* resolutions, int num_lods, int active_lods,
                                           int codebook_bitwidth, const float* w1, const float* b1, const float* w2, const float* b2,
                                           int hidden, float* grad_codebook, float* grad_w1, float* grad_b1, float* grad_w2,
                                           float* grad_b2, float* loss, float* pred, void* scratch, int64_t scratch_bytes,
                                           wisp_stream_t stream) {
    WISP_REQUIRE(n >= 1, "bad sizes");
    WISP_REQUIRE(n <= IFT_MAX_N, "at most 2^22 samples a step: (float)(3 n) must be exact");
    WISP_REQUIRE(num_lods >= 1 && num_lods <= IF_MAX_LODS, "num_lods must be in 1..16");
    WISP_REQUIRE(active_lods >= 0 && active_lods <= num_lods, "active_lods out of range");
    WISP_REQUIRE(codebook_bitwidth >= 1 && codebook_bitwidth <= 30, "codebook_bitwidth out of range");
    WISP_REQUIRE(hidden >= 1 && hidden <= IF_MAX_HIDDEN, "hidden width must be in 1..128");
    WISP_REQUIRE(coords && rgb && codebook && first_idx && resolutions && w1 && b1 && w2 && b2 && grad_codebook && grad_w1 && grad_b1 &&
                 grad_w2 && grad_b2 && loss && scratch, "null pointer");
    WISP_REQUIRE(((uintptr_t)codebook & 7) == 0, "codebook must be 8-byte aligned");
    WISP_REQUIRE(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
    const int64_t need = wisp_image_field_train_scratch_bytes(n, num_lods, hidden);
    WISP_REQUIRE(need >= 0, "LDS budget exceeded");
    WISP_REQUIRE(scratch_bytes >= need, "scratch too small (wisp_image_field_train_scratch_bytes)");
    ImageTrainField fld;
    const int64_t tsize = (int64_t)1 << codebook_bitwidth;
    WISP_REQUIRE(fill_levels(resolutions, num_lods, 2, tsize, fld.lv) == 0, "bad resolution");
    // Every index the forward and the scatter can form must lie inside the level's own rows: a hashed index is below 2^bitwidth,
    // a dense one reaches res^2 - 1 (from resolution 258 on it is pinned into the table instead, as in the render kernel).
    WISP_REQUIRE(first_idx[0] >= 0, "negative first row");
    for (int l = 0; l < num_lods; ++l) {
        const int64_t rows = first_idx[l + 1] - first_idx[l], r = resolutions[l];
        WISP_REQUIRE(rows >= 1, "a level without rows");
        WISP_REQUIRE(fld.lv.dense[l] ? (r >= 258 || rows >= r * r) : rows >= tsize, "a level has fewer rows than an index reaches");
    }
    fld.codebook = codebook;
    for (int l = 0; l <= IF_MAX_LODS; ++l) fld.begin[l] = first_idx[l <= num_lods ? l : num_lods];
    fld.num_lods = num_lods; fld.active_lods = active_lods; fld.tsize = (uint32_t)tsize;
    fld.w1 = w1; fld.b1 = b1; fld.w2 = w2; fld.b2 = b2; fld.hidden = hidden;
    const size_t lds = ift_lds_bytes(hidden, num_lods);
    const int grid = ift_grid(n), row_stride = ift_row_stride(hidden, num_lods), in_dim = 2 * num_lods + IF_EMBED;
    double* partials = static_cast<double*>(scratch);
    double* wacc = partials + (size_t)grid * row_stride;
    IftWide wide;
    wide.n = 0;
    wide.off[0] = 0;
    for (int l = 0; l < IF_MAX_LODS; ++l) {
        wide.lvl[l] = -1;
        if (l >= active_lods) continue;
        // the rows a level's indices reach (checked above to exist): res^2 of a dense level - whatever the table's layout declares
        // beyond them, a HashGrid built with coord_dim = 3 gives a level min(2^bitwidth, res^3) rows -, 2^bitwidth of a hashed one
        const int64_t r = resolutions[l], entries = 2 * (fld.lv.dense[l] ? r * r : tsize);
        if (r >= 258 || entries > IFT_WIDE_ENTRIES) continue;                     // (a pinned index may leave the level's own rows)
        wide.lvl[l] = wide.n;
        wide.tbl[wide.n] = first_idx[l] * 2;
        wide.off[wide.n + 1] = wide.off[wide.n] + entries;
        ++wide.n;
    }
    for (int i = wide.n + 1; i <= IF_MAX_LODS; ++i) wide.off[i] = wide.off[wide.n];
    for (int i = wide.n; i < IF_MAX_LODS; ++i) wide.tbl[i] = 0;
    hipStream_t s = (hipStream_t)stream;
    if (const hipError_t e = WISP_ALLOW_LDS(image_field_train_kernel, lds)) return wisp_fail(WISP_ERR_LAUNCH, __func__, hipGetErrorString(e));
    if (wide.off[wide.n] > 0 && hipMemsetAsync(wacc, 0, (size_t)wide.off[wide.n] * sizeof(double), s) != hipSuccess)
        return wisp_fail(WISP_ERR_LAUNCH, __func__, "hipMemsetAsync failed");
    hipLaunchKernelGGL(image_field_train_kernel, dim3(grid), dim3(IFT_BLOCK), lds, s, coords, rgb, n, fld, (float)(3 * n), grad_codebook,
                       partials, row_stride, wide, wacc, pred);
    hipLaunchKernelGGL(image_field_train_reduce_kernel, dim3((ift_entries(hidden, num_lods) + 15) / 16), dim3(256), 0, s, partials, grid,
                       row_stride, hidden, in_dim, grad_w1, grad_b1, grad_w2, grad_b2, loss, (double)(3 * n), wide, wacc, grad_codebook);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
