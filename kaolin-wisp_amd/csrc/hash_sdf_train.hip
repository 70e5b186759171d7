// One optimisation step's forward + loss + backward of the reference's SDFTrainer (wisp/trainers/sdf_trainer.py:65-124, only_last)
// for a NeuralSDF over a HashGrid (wisp/models/nefs/neural_sdf.py:120-155 over wisp/models/grids/hash_grid.py:205-233;
// nglod_hash.yaml: 'cat', 4 levels x 8 features, [position, features] -> Linear(35, 128) -> relu -> Linear(128, 1), 512
// coordinates per step):
//     pred = decoder([x, features(x)]) ;  loss = sum (pred - gt)^2 / B ;  backward
// The hash-grid twin of wisp_sdf_train_step (spc_grad.hip).  Through autograd over the modular ops the step is a hashgrid forward,
// a zeroing slice, a concatenation, two GEMMs with their elementwise companions, the loss, and all of that again backwards; at
// 512 coordinates every one of those launches is launch latency.  Here, the two launches described in sdf_step_dev.h; the column
// sum, the owner-summed partial row, the reduce, the fp64 accumulators (SdfWide) and the host side are that header's.  This file's:
//   hash_sdf_train_kernel  the kernel's frame (weight staging, LDS carve-up, the sample loop, the loss block: the triplanar kernel
//                     restates it, see sdf_step_dev.h for why) and the table gradient, scattered in it: the lane that blended a
//                     column pair recomputes its corner_setup (the same bits) and adds coef[j] * dfeat to the pair's eight rows of
//                     grad_codebook with f32 atomic adds - the form of hashgrid_bwd_kernel (hashgrid.hip), global_atomic_add_f32
//                     under -munsafe-fp-atomics.  Columns at or above zero_from_col are neither gathered nor scattered; for 'sum'
//                     every level receives the same feature gradient.
//   wide levels       a level of at most 2^16 table entries - the coarse ones, where many samples of a batch meet on a row
//                     (resolution 16: 4913 corners for every batch size) - takes its gradient through the fp64 accumulators of
//                     SdfWide instead; the admission rule is in wisp_hash_sdf_train_step.
// The table gradient goes through atomics, as the reference's backward (hashgrid_interpolate_cuda.cu) and this library's
// small-batch hash backward do: its sums depend on arrival order and are repeatable only where they are exact.
#include "wisp_common.h"
#include "hash_sdf_eval_dev.h"
#include "sdf_step_dev.h"

struct HstWide : SdfWide<HSDF_MAX_LODS> {};            // slot[l]: level l; dst: the level's first entry in grad_codebook

// the largest admitted shape, hidden 256 over 'cat' of 32 columns (35 inputs): 35840 (W1) + 2048 + 2240 (inputs) + 32768 + 128 +
// 2048 + 37896 (partial row) = 112968 bytes
static_assert(sdf_step_lds_bytes(SDF_MAX_HIDDEN, HSDF_MAX_COLS, 3 + HSDF_MAX_COLS) <= SDF_STEP_MAX_LDS,
              "the largest 'cat' shape must fit one workgroup's LDS");

__global__ void __launch_bounds__(SDF_STEP_BLOCK)
hash_sdf_train_kernel(const float* __restrict__ coords, const float* __restrict__ gts, int64_t n, HashSdfField fld, float inv_batch,
                      float* __restrict__ grad_codebook, float* __restrict__ partials /* [grid][row] */, int row_stride,
                      HstWide wide, double* __restrict__ wacc) {
    extern __shared__ float s_hst[];
    const SdfDecoderLds s = sdf_decoder_stage(s_hst, fld.dec, HashSdfEnc<float>::group_floats(fld));
    const int H = fld.dec.hidden, cols = fld.dec.cols, F = fld.feature_dim;
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
    const int level_cols = fld.num_lods * F;
    const int64_t rounds = (n + SDF_STEP_GROUPS - 1) / SDF_STEP_GROUPS;
    __syncthreads();
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * SDF_STEP_GROUPS + grp;
        if (i < n) {                                     // (a group enters or stays out as a whole: the shuffles are 16 wide)
            const float px = coords[i * 3], py = coords[i * 3 + 1], pz = coords[i * 3 + 2];
            // ---- forward: wisp_hash_sdf_query's value
            hash_sdf_point_inputs<float>(fld, gin, c, px, py, pz);
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
            // ---- table gradient: the lane that blended a column pair scatters it
            for (int q = c; 2 * q < level_cols; q += SDF_GROUP) {
                const int col = 2 * q;
                if (col >= fld.zero_from_col) continue;
                const int l = col / F, k = col - l * F;
                const int fcol = fld.sum ? k : col;      // 'sum': every level receives the gradient of the summed column
                const float d0 = gdx[fcol];
                const float d1 = (col + 1 < fld.zero_from_col) ? gdx[fcol + 1] : 0.0f;
                const float pos[3] = {px, py, pz};
                CornerSetup<3> cs;
                const bool dense = fld.lv.dense[l] != 0;
                corner_setup<3>(pos, fld.lv.res[l], fld.lv.hi[l], fld.lv.hr[l], dense, fld.tsize, true, cs);
                const int64_t first = fld.begin[l];
                if (dense) {                             // the forward's pin: the gradient goes to the row that was read
                    const int64_t last = fld.begin[fld.num_lods] - 1 - first;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if ((int64_t)(uint32_t)cs.idx[j] > last) cs.idx[j] = (int32_t)last;
                }
                const int wl = wide.slot[l];
                if (wl >= 0) {                           // a small level: exact fp64 products into its fp64 accumulators
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        double* p = wacc + wide.off[wl] + (int64_t)(uint32_t)cs.idx[j] * F + k;
                        const double v0 = (double)cs.coef[j] * (double)d0, v1 = (double)cs.coef[j] * (double)d1;
                        if (v0 != 0.0) atomicAdd(p, v0);             // global_atomic_add_f64
                        if (v1 != 0.0) atomicAdd(p + 1, v1);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
#pragma clang fp contract(off)
                        float* p = grad_codebook + (first + (int64_t)(uint32_t)cs.idx[j]) * F + k;
                        const float v0 = cs.coef[j] * d0, v1 = cs.coef[j] * d1;
                        if (v0 != 0.0f) atomicAdd(p, v0);            // global_atomic_add_f32
                        if (v1 != 0.0f) atomicAdd(p + 1, v1);
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
hash_sdf_train_reduce_kernel(const float* __restrict__ partials, int rows, int row_stride, int H, int in_dim, float* __restrict__ gw1,
                             float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2, float* __restrict__ loss,
                             float inv_batch, HstWide wide, const double* __restrict__ wacc) {
    sdf_step_reduce_body(partials, rows, row_stride, H, in_dim, gw1, gb1, gw2, gb2, loss, inv_batch, wide, wacc);
}

// ---------------------------------------------------------------------------------------------------- host side
extern "C" int64_t wisp_hash_sdf_train_scratch_bytes(int64_t n, int num_lods, int feature_dim, int multiscale, int hidden) {
    if (n < 1 || num_lods < 1 || num_lods > HSDF_MAX_LODS || (feature_dim != 2 && feature_dim != 4 && feature_dim != 8) ||
        (multiscale != 0 && multiscale != 1) || hidden < 1 || hidden > SDF_MAX_HIDDEN) return -1;
    const int cols = multiscale ? feature_dim : num_lods * feature_dim;
    if (cols > HSDF_MAX_COLS ||
        sdf_step_lds_bytes(hidden, cols, hash_sdf_group_floats(cols, num_lods, feature_dim, multiscale)) > SDF_STEP_MAX_LDS) return -1;
    // the partial rows, then room for every level's fp64 accumulators (which levels are small depends on the resolutions)
    return sdf_step_partials_bytes(n, hidden, cols) + (int64_t)num_lods * SDF_STEP_WIDE_ENTRIES * (int64_t)sizeof(double);
}

extern "C" int wisp_hash_sdf_train_step(const float* coords, const float* gts, int64_t n, const void* codebook, int feats_dtype,
                                        const int64_t* begin_idxes, const int32_t* resolutions, int num_lods, int feature_dim,
                                        int codebook_bitwidth, int multiscale, int zero_from_col, const float* w1, const float* b1,
                                        const float* w2, const float* b2, int hidden, float* grad_codebook, float* grad_w1,
                                        float* grad_b1, float* grad_w2, float* grad_b2, float* loss, void* scratch,
                                        int64_t scratch_bytes, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 1, "bad sizes");
    HashSdfField fld;
    if (const int rc = hash_sdf_fill(fld, __func__, codebook, feats_dtype, begin_idxes, resolutions, num_lods, feature_dim,
                                     codebook_bitwidth, multiscale, zero_from_col, w1, b1, w2, b2, hidden)) return rc;
    WISP_REQUIRE(feats_dtype == WISP_F32, "the table must be f32 under training");
    WISP_REQUIRE(coords && gts && grad_codebook && grad_w1 && grad_b1 && grad_w2 && grad_b2 && loss && scratch, "null pointer");
    const int64_t need = wisp_hash_sdf_train_scratch_bytes(n, num_lods, feature_dim, multiscale, hidden);
    WISP_REQUIRE(need >= 0, "LDS budget exceeded");
    WISP_REQUIRE(scratch_bytes >= need, "scratch too small (wisp_hash_sdf_train_scratch_bytes)");
    HstWide wide;
    sdf_wide_clear(wide);
    for (int l = 0; l < num_lods && l * feature_dim < zero_from_col; ++l) {
        const int64_t rows = begin_idxes[l + 1] - begin_idxes[l], entries = rows * feature_dim;
        // Every index the scatter can form must lie inside the level's own accumulators.  A hashed index is below 2^bitwidth <= rows
        // (hash_sdf_fill); a dense one reaches res^3 - 1, and hash_sdf_fill admits a dense level that declares fewer rows (the
        // forward and the f32 scatter pin into the whole table): such a level keeps the f32 scatter.  (From resolution 258 on an
        // index can be pinned to the table's last row; res^3 is then far above the threshold anyway.)
        const int64_t r = resolutions[l];
        if (entries > SDF_STEP_WIDE_ENTRIES || r >= 258 || (fld.lv.dense[l] && rows < r * r * r)) continue;
        sdf_wide_add(wide, l, grad_codebook + begin_idxes[l] * feature_dim, entries);
    }
    return sdf_step_launch<hash_sdf_train_kernel, hash_sdf_train_reduce_kernel>(
        __func__, coords, gts, n, fld, HashSdfEnc<float>::group_floats(fld), grad_codebook, grad_w1, grad_b1, grad_w2, grad_b2, loss,
        scratch, wide, (hipStream_t)stream);
}
