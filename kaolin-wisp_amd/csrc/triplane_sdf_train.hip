// One optimisation step's forward + loss + backward of the reference's SDFTrainer (wisp/trainers/sdf_trainer.py:65-124, only_last)
// for a NeuralSDF over a TriplanarGrid (wisp/models/nefs/neural_sdf.py:120-155 over wisp/models/grids/triplanar_grid.py:97-146 and
// :205-233; nglod_triplanar.yaml: 'sum', one level of three 4 x 33 x 33 planes, [position, features] -> Linear(15, 128) -> relu ->
// Linear(128, 1), 512 coordinates per step):
//     pred = decoder([x, features(x)]) ;  loss = sum (pred - gt)^2 / B ;  backward
// The triplanar twin of wisp_hash_sdf_train_step (hash_sdf_train.hip).  Through autograd over the modular ops the step is a triplane
// forward, a concatenation, two GEMMs with their elementwise companions, the loss, and all of that again backwards, ending in
// wisp_triplane_bwd; at 512 coordinates every one of those launches is launch latency.  Here, the two launches described in
// sdf_step_dev.h; the column sum, the owner-summed partial row, the reduce, the fp64 accumulators (SdfWide) and the host side are
// that header's.  This file's:
//   triplane_sdf_train_kernel  the kernel's frame (weight staging, LDS carve-up, the sample loop, the loss block: restated from
//                    hash_sdf_train_kernel, see sdf_step_dev.h for why) and the plane gradient, scattered in it: the lane that
//                    blended column j recomputes the lookup's corner and weights (tri_sdf_corner, the function tri_sdf_blend
//                    runs: the same bits) and adds w_corner * dfeat[j] to the texels it read; a corner the forward left out
//                    (x0 + 1 >= R or y0 + 1 >= R) gets nothing.  'sum': every level receives the gradient of the summed column;
//                    'cat': a column belongs to one (level, plane, channel).
//   wide planes      a plane of at most 2^16 entries (feature_dim * R * R) - the shipped 4 x 33 x 33 plane, where 512 samples pile
//                    onto 1089 texels - takes its gradient through the fp64 accumulators of SdfWide; a larger plane takes f32
//                    atomic adds straight into its gradient tensor.
// The plane gradients go through atomics in both regimes - fp64 atomics still arrive in any order: their sums are repeatable only
// where they are exact.
#include "wisp_common.h"
#include "triplane_sdf_eval_dev.h"
#include "sdf_step_dev.h"

#define TST_MAX_PLANES (TSDF_MAX_LODS * 3)

struct TstWide : SdfWide<TST_MAX_PLANES> {};           // slot[k]: plane k of the field's plane list; dst: that plane's gradient
struct TstGrads { float* grad[TST_MAX_PLANES]; };       // the gradient of every plane, in the order of TriSdfField::planes

// the largest admitted shape, hidden 256 over 48 columns (51 inputs): 52224 (W1) + 2048 + 3264 (inputs) + 32768 + 128 + 3072 +
// 54280 (partial row) = 147784 bytes
static_assert(sdf_step_lds_bytes(SDF_MAX_HIDDEN, TSDF_MAX_COLS, 3 + TSDF_MAX_COLS) <= SDF_STEP_MAX_LDS,
              "the largest shape (hidden 256, 48 columns) must fit one workgroup's LDS");

__global__ void __launch_bounds__(SDF_STEP_BLOCK)
triplane_sdf_train_kernel(const float* __restrict__ coords, const float* __restrict__ gts, int64_t n, TriSdfField fld, float inv_batch,
                          TstGrads gp, float* __restrict__ partials /* [grid][row] */, int row_stride, TstWide wide,
                          double* __restrict__ wacc) {
    extern __shared__ float s_tst[];
    const SdfDecoderLds s = sdf_decoder_stage(s_tst, fld.dec, TriSdfEnc::group_floats(fld));
    const int H = fld.dec.hidden, cols = fld.dec.cols, F = fld.feature_dim, F3 = 3 * F;
    const int in_dim = 3 + cols;
    float* s_ga = s.in + SDF_STEP_GROUPS * s.stride;    // [groups][H]      d loss / d pre-activation
    float* s_gr = s_ga + SDF_STEP_GROUPS * H;           // [groups][H]      d loss / d pred * relu output (for d w2)
    float* s_g = s_gr + SDF_STEP_GROUPS * H;            // [groups]         d loss / d pred
    float* s_sq = s_g + SDF_STEP_GROUPS;                // [groups]         squared error
    float* s_dx = s_sq + SDF_STEP_GROUPS;               // [groups][cols]   d loss / d feature column
    // partial sums of this workgroup: d W1 [H][in_dim], d b1 [H], d w2 [H], d b2, loss - in that order; every entry has one owner
    float* s_own = s_dx + SDF_STEP_GROUPS * cols;       // [n_entries]
    const int n_entries = H * in_dim + 2 * H + 2;
    for (int e = threadIdx.x; e < n_entries; e += blockDim.x) s_own[e] = 0.0f;
    const int c = threadIdx.x & (SDF_GROUP - 1), grp = threadIdx.x / SDF_GROUP;
    float* gin = s.in + grp * s.stride;
    float* ga = s_ga + grp * H;
    float* gr = s_gr + grp * H;
    float* gdx = s_dx + grp * cols;
    const int64_t rounds = (n + SDF_STEP_GROUPS - 1) / SDF_STEP_GROUPS;
    __syncthreads();
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * SDF_STEP_GROUPS + grp;
        if (i < n) {                                     // (a group enters or stays out as a whole: the shuffles are 16 wide)
            const float px = coords[i * 3], py = coords[i * 3 + 1], pz = coords[i * 3 + 2];
            // ---- forward: wisp_triplane_sdf_query's value
            tri_sdf_point_inputs(fld, gin, c, px, py, pz);
            const float pred = sdf_decode<true>(fld.dec, s, gin, c, ga, gr);
            float g, sq;
            {
#pragma clang fp contract(off)
                const float diff = pred - gts[i];
                g = 2.0f * diff * inv_batch;             // d [sum (pred - gt)^2 / B] / d pred
                sq = diff * diff;
                for (int hh = c; hh < H; hh += SDF_GROUP) { ga[hh] *= g; gr[hh] *= g; }
            }
            if (c == 0) { s_g[grp] = g; s_sq[grp] = sq; }
            __builtin_amdgcn_wave_barrier();             // a group's lanes are in one wave: LDS order suffices
            sdf_step_column_sum(s, ga, gdx, c, H, cols);
            __builtin_amdgcn_wave_barrier();
            // ---- plane gradient: the lane that blended a column scatters it (the column split of tri_sdf_point_inputs)
            for (int j = c; j < cols; j += SDF_GROUP) {
                const int l0 = fld.sum ? 0 : j / F3, l1 = fld.sum ? fld.num_lods : l0 + 1;
                const int rem = j - (fld.sum ? 0 : l0 * F3);
                const int p = rem / F, ch = rem - p * F;
                const float gx = p == 0 ? py : px;
                const float gy = p == 2 ? py : pz;
                const float d = gdx[j];                  // 'sum': every level receives the gradient of the summed column
                for (int l = l0; l < l1; ++l) {
                    const int R = fld.size[l], k = l * 3 + p;
                    const TriSdfCorner cn = tri_sdf_corner(R, ch, gx, gy);
                    const bool v01 = cn.vx1, v10 = cn.vy1, v11 = cn.vx1 && cn.vy1;
                    const int wl = wide.slot[k];
                    if (wl >= 0) {                       // a small plane: exact fp64 products into its fp64 accumulators
                        double* q = wacc + wide.off[wl] + cn.off;
                        const double t00 = (double)cn.w00 * (double)d, t01 = (double)cn.w01 * (double)d;
                        const double t10 = (double)cn.w10 * (double)d, t11 = (double)cn.w11 * (double)d;
                        if (t00 != 0.0) atomicAdd(q, t00);                           // global_atomic_add_f64
                        if (v01 && t01 != 0.0) atomicAdd(q + 1, t01);
                        if (v10 && t10 != 0.0) atomicAdd(q + R, t10);
                        if (v11 && t11 != 0.0) atomicAdd(q + (int64_t)R + 1, t11);
                    } else {
#pragma clang fp contract(off)
                        float* q = gp.grad[k] + cn.off;
                        const float t00 = cn.w00 * d, t01 = cn.w01 * d, t10 = cn.w10 * d, t11 = cn.w11 * d;
                        if (t00 != 0.0f) atomicAdd(q, t00);                          // global_atomic_add_f32
                        if (v01 && t01 != 0.0f) atomicAdd(q + 1, t01);
                        if (v10 && t10 != 0.0f) atomicAdd(q + R, t10);
                        if (v11 && t11 != 0.0f) atomicAdd(q + (int64_t)R + 1, t11);
                    }
                }
            }
        } else {
            for (int hh = c; hh < H; hh += SDF_GROUP) { ga[hh] = 0.0f; gr[hh] = 0.0f; }
            for (int e = c; e < in_dim; e += SDF_GROUP) gin[e] = 0.0f;
            if (c == 0) { s_g[grp] = 0.0f; s_sq[grp] = 0.0f; }
        }
        __syncthreads();
        sdf_step_owner_sum(s, s_ga, s_gr, s_g, s_sq, s_own, H, in_dim);
        __syncthreads();
    }
    for (int e = threadIdx.x; e < n_entries; e += blockDim.x) partials[(int64_t)blockIdx.x * row_stride + e] = s_own[e];
}

__global__ void __launch_bounds__(256)
triplane_sdf_train_reduce_kernel(const float* __restrict__ partials, int rows, int row_stride, int H, int in_dim,
                                 float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2,
                                 float* __restrict__ loss, float inv_batch, TstWide wide, const double* __restrict__ wacc) {
    sdf_step_reduce_body(partials, rows, row_stride, H, in_dim, gw1, gb1, gw2, gb2, loss, inv_batch, wide, wacc);
}

// ---------------------------------------------------------------------------------------------------- host side
// the shape rules of tri_sdf_fill, without the pointers: the feature columns, or -1
static inline int tst_cols(const int32_t* sizes, int num_lods, int feature_dim, int multiscale, int hidden) {
    if (!sizes || num_lods < 1 || num_lods > TSDF_MAX_LODS || feature_dim < 1 || (multiscale != 0 && multiscale != 1) || hidden < 1 ||
        hidden > SDF_MAX_HIDDEN) return -1;
    const int64_t cols = (int64_t)(multiscale ? 1 : num_lods) * 3 * feature_dim;
    if (cols > TSDF_MAX_COLS || sdf_step_lds_bytes(hidden, (int)cols, 3 + (int)cols) > SDF_STEP_MAX_LDS) return -1;
    for (int l = 0; l < num_lods; ++l)
        if (sizes[l] < 1) return -1;
    return (int)cols;
}
static inline int64_t tst_plane_entries(int feature_dim, int size) { return (int64_t)feature_dim * size * size; }

extern "C" int64_t wisp_triplane_sdf_train_scratch_bytes(int64_t n, const int32_t* sizes, int num_lods, int feature_dim,
                                                         int multiscale, int hidden) {
    if (n < 1) return -1;
    const int cols = tst_cols(sizes, num_lods, feature_dim, multiscale, hidden);
    if (cols < 0) return -1;
    // the partial rows, then the fp64 accumulators of the small planes (three per level)
    int64_t wide = 0;
    for (int l = 0; l < num_lods; ++l) {
        const int64_t entries = tst_plane_entries(feature_dim, sizes[l]);
        if (entries <= SDF_STEP_WIDE_ENTRIES) wide += 3 * entries;
    }
    return sdf_step_partials_bytes(n, hidden, cols) + wide * (int64_t)sizeof(double);
}

extern "C" int wisp_triplane_sdf_train_step(const float* coords, const float* gts, int64_t n, const float* const* planes,
                                            const int32_t* sizes, int num_lods, int feature_dim, int multiscale, const float* w1,
                                            const float* b1, const float* w2, const float* b2, int hidden,
                                            float* const* grad_planes, float* grad_w1, float* grad_b1, float* grad_w2,
                                            float* grad_b2, float* loss, void* scratch, int64_t scratch_bytes,
                                            wisp_stream_t stream) {
    WISP_REQUIRE(n >= 1, "bad sizes");
    TriSdfField fld;
    if (const int rc = tri_sdf_fill(fld, __func__, planes, sizes, num_lods, feature_dim, multiscale, w1, b1, w2, b2, hidden,
                                    SDF_STEP_GROUPS)) return rc;
    WISP_REQUIRE(coords && gts && grad_planes && grad_w1 && grad_b1 && grad_w2 && grad_b2 && loss && scratch, "null pointer");
    for (int k = 0; k < num_lods * 3; ++k) WISP_REQUIRE(grad_planes[k], "null plane gradient pointer");
    const int64_t need = wisp_triplane_sdf_train_scratch_bytes(n, sizes, num_lods, feature_dim, multiscale, hidden);
    WISP_REQUIRE(need >= 0, "LDS budget exceeded");
    WISP_REQUIRE(scratch_bytes >= need, "scratch too small (wisp_triplane_sdf_train_scratch_bytes)");
    TstWide wide;
    TstGrads gp = {};
    sdf_wide_clear(wide);
    for (int k = 0; k < num_lods * 3; ++k) {
        gp.grad[k] = grad_planes[k];
        // every offset the scatter can form lies inside the plane: channel < feature_dim, x0 and y0 in [0, R - 1], and a corner at
        // x0 + 1 or y0 + 1 is written only where it is below R
        const int64_t entries = tst_plane_entries(feature_dim, sizes[k / 3]);
        if (entries <= SDF_STEP_WIDE_ENTRIES) sdf_wide_add(wide, k, grad_planes[k], entries);
    }
    return sdf_step_launch<triplane_sdf_train_kernel, triplane_sdf_train_reduce_kernel>(
        __func__, coords, gts, n, fld, TriSdfEnc::group_floats(fld), gp, grad_w1, grad_b1, grad_w2, grad_b2, loss, scratch, wide,
        (hipStream_t)stream);
}
