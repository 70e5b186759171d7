// One optimisation step's forward + loss + backward of the reference's SDFTrainer (wisp/trainers/sdf_trainer.py:65-124, only_last)
// for a NeuralSDF over a HashGrid (wisp/models/nefs/neural_sdf.py:120-155 over wisp/models/grids/hash_grid.py:205-233;
// nglod_hash.yaml: 'cat', 4 levels x 8 features, [position, features] -> Linear(35, 128) -> relu -> Linear(128, 1), 512
// coordinates per step):
//     pred = decoder([x, features(x)]) ;  loss = sum (pred - gt)^2 / B ;  backward
// The hash-grid twin of wisp_sdf_train_step (spc_grad.hip).  Through autograd over the modular ops the step is a hashgrid forward,
// a zeroing slice, a concatenation, two GEMMs with their elementwise companions, the loss, and all of that again backwards; at
// 512 coordinates every one of those launches is launch latency.  Here, two launches:
//   hash_sdf_train_kernel         16 lanes own a sample.  The forward is hash_sdf_eval_point's two halves (hash_sdf_eval_dev.h),
//                                 statement for statement: the predicted distance is bit for bit what wisp_hash_sdf_query returns
//                                 for the same parameters.  Then g = 2 (pred - gt) / B and the decoder backward as in the
//                                 one-output sdf_train_kernel<1>: lane c keeps hidden units c, c + 16, ..., the gradient of the decoder's
//                                 feature columns is a column sum over LDS.  The table gradient is scattered right there: the lane
//                                 that blended a column pair recomputes its corner_setup (the same bits) and adds coef[j] * dfeat
//                                 to the pair's eight rows of grad_codebook with f32 atomic adds - the form of hashgrid_bwd_kernel
//                                 (hashgrid.hip), global_atomic_add_f32 under -munsafe-fp-atomics.  Columns at or above
//                                 zero_from_col are neither gathered nor scattered; for 'sum' every level receives the same
//                                 feature gradient.  Per workgroup the decoder's weight gradients and the squared error are summed
//                                 by the thread that owns the entry, in sample order, and stored as one partial row - no atomics.
//   hash_sdf_train_reduce_kernel  adds the partial rows up in workgroup order, ADDS the sums to the decoder's gradient tensors,
//                                 writes the loss (sdf_train_reduce_kernel's scheme for one output; that kernel lives in
//                                 another translation unit, serves the octree steps of both fields and sums in fp32).
// The sums over hidden units, samples and partial rows run in fp64 and are rounded to fp32 once each (products of two floats are
// exact in fp64): that keeps every gradient as close to the float64 result as the modular path's library GEMMs are.
// A level of at most 2^16 table entries - the coarse ones, where many samples of a batch meet on a row - takes its gradient through
// fp64 accumulators in scratch instead (HstWide below): exact fp64 products, fp64 atomic adds, one rounding per entry in the reduce
// kernel; the step zeroes the accumulators with one memset in front of the two launches.
// Determinism: the loss and the four decoder gradients have a fixed summation order and are bitwise repeatable.  The table
// gradient goes through float atomics, as the reference's backward (hashgrid_interpolate_cuda.cu) and this library's small-batch
// hash backward do: its sums depend on arrival order and are repeatable only where they are exact.
#include "wisp_common.h"
#include "hash_sdf_eval_dev.h"

#define HST_BLOCK 256
#define HST_GROUPS (HST_BLOCK / HSDF_GROUP)            // samples per workgroup pass
#define HST_MAX_LDS (160 * 1024)                       // one workgroup may hold the whole LDS of a compute unit
#define HST_WIDE_ENTRIES (1 << 16)                     // a level of at most this many table entries is summed in fp64

// The small levels - where a batch puts many samples on one row (resolution 16: 4913 corners for every batch size) - do not take
// their gradient by f32 atomics: a row's sum of m terms would carry m roundings in arrival order.  They get fp64 accumulators in
// scratch (zeroed by the step), the scatter adds the exact fp64 product coef * dfeat with fp64 atomic adds, and the reduce kernel
// rounds every accumulator once into grad_codebook.  off[i] .. off[i + 1]: accumulators of the i-th such level, tbl[i]: its first
// entry in the table, lvl[l]: the position of level l in that list or -1.
struct HstWide {
    int64_t off[HSDF_MAX_LODS + 1];
    int64_t tbl[HSDF_MAX_LODS];
    int32_t lvl[HSDF_MAX_LODS];
    int n;
};

static inline int hst_entries(int hidden, int cols) { return hidden * (3 + cols) + 2 * hidden + 2; }
static inline int hst_row_stride(int hidden, int cols) { return (hst_entries(hidden, cols) + 15) / 16 * 16; }
static inline int hst_grid(int64_t n) { return (int)min64(ceil_div64(n, HST_GROUPS), 1024); }
// LDS of a workgroup: what hash_sdf_stage lays out (weights, the groups' decoder inputs) | d loss / d pre-activation [groups][H] |
// d loss / d pred * relu output [groups][H] | d loss / d pred [groups] | squared error [groups] | d loss / d feature column
// [groups][cols] | the workgroup's partial row
static inline size_t hst_lds_bytes(int hidden, int cols, int num_lods, int feature_dim, int sum) {
    return hash_sdf_lds_bytes(hidden, cols, num_lods, feature_dim, sum, HST_GROUPS) +
           ((size_t)HST_GROUPS * (2 * hidden + 2 + cols) + (size_t)hst_entries(hidden, cols)) * sizeof(float);
}
// the largest admitted shape, hidden 256 over 'cat' of 32 columns (35 inputs): 35840 (W1) + 2048 + 2240 (inputs) + 32768 + 128 +
// 2048 + 37896 (partial row) = 112968 bytes
static_assert(((size_t)HSDF_MAX_HIDDEN * ((3 + HSDF_MAX_COLS) | 1) + 2 * HSDF_MAX_HIDDEN + (size_t)HST_GROUPS * (3 + HSDF_MAX_COLS) +
               (size_t)HST_GROUPS * (2 * HSDF_MAX_HIDDEN + 2 + HSDF_MAX_COLS) +
               (size_t)HSDF_MAX_HIDDEN * (3 + HSDF_MAX_COLS) + 2 * HSDF_MAX_HIDDEN + 2) * sizeof(float) <= HST_MAX_LDS,
              "the largest 'cat' shape must fit one workgroup's LDS");

__global__ void __launch_bounds__(HST_BLOCK)
hash_sdf_train_kernel(const float* __restrict__ coords, const float* __restrict__ gts, int64_t n, HashSdfField fld, float inv_batch,
                      float* __restrict__ grad_codebook, float* __restrict__ partials /* [grid][row] */, int row_stride,
                      HstWide wide, double* __restrict__ wacc) {
    extern __shared__ float s_hst[];
    const HashSdfLds s = hash_sdf_stage(s_hst, fld);
    const int H = fld.hidden, cols = fld.cols, F = fld.feature_dim;
    const int in_dim = 3 + cols;
    float* s_ga = s.in + HST_GROUPS * s.stride;         // [groups][H]      d loss / d pre-activation
    float* s_gr = s_ga + HST_GROUPS * H;                // [groups][H]      d loss / d pred * relu output (for d w2)
    float* s_g = s_gr + HST_GROUPS * H;                 // [groups]         d loss / d pred
    float* s_sq = s_g + HST_GROUPS;                     // [groups]         squared error
    float* s_dx = s_sq + HST_GROUPS;                    // [groups][cols]   d loss / d feature column
    // partial sums of this workgroup: d W1 [H][in_dim], d b1 [H], d w2 [H], d b2, loss - in that order; every entry has one owner
    float* s_own = s_dx + HST_GROUPS * cols;            // [n_entries]
    const int n_entries = H * in_dim + 2 * H + 2;
    for (int e = threadIdx.x; e < n_entries; e += blockDim.x) s_own[e] = 0.0f;
    const int c = threadIdx.x & (HSDF_GROUP - 1), grp = threadIdx.x / HSDF_GROUP;
    float* gin = s.in + grp * s.stride;
    float* ga = s_ga + grp * H;
    float* gr = s_gr + grp * H;
    float* gdx = s_dx + grp * cols;
    const int level_cols = fld.num_lods * F;
    const int64_t rounds = (n + HST_GROUPS - 1) / HST_GROUPS;
    __syncthreads();
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * HST_GROUPS + grp;
        if (i < n) {                                     // (a group enters or stays out as a whole: the shuffles are 16 wide)
            const float px = coords[i * 3], py = coords[i * 3 + 1], pz = coords[i * 3 + 2];
            // ---- forward: wisp_hash_sdf_query's value
            hash_sdf_point_inputs<float>(fld, gin, c, px, py, pz);
            const float pred = hash_sdf_decode<true>(fld, s, gin, c, ga, gr);
            float g, sq;
            {
#pragma clang fp contract(off)
                const float diff = pred - gts[i];
                g = 2.0f * diff * inv_batch;             // d [sum (pred - gt)^2 / B] / d pred
                sq = diff * diff;
                for (int hh = c; hh < H; hh += HSDF_GROUP) { ga[hh] *= g; gr[hh] *= g; }
            }
            if (c == 0) { s_g[grp] = g; s_sq[grp] = sq; }
            __builtin_amdgcn_wave_barrier();             // a group's lanes are in one wave: LDS order suffices
            // ---- gradient of the decoder input, feature columns only (nothing consumes d / d position)
            //      summed in fp64 (every product of two floats is exact there) and rounded once: a chain of up to 256 fp32 fma
            //      steps was up to three times as far from the float64 result as the modular path's GEMM
            for (int col = c; col < cols; col += HSDF_GROUP) {
                double dx0 = 0.0, dx1 = 0.0;
                int hh = 0;
                for (; hh + 1 < H; hh += 2) {
                    dx0 = __builtin_fma((double)ga[hh], (double)s.w1[hh * s.in_pad + 3 + col], dx0);
                    dx1 = __builtin_fma((double)ga[hh + 1], (double)s.w1[(hh + 1) * s.in_pad + 3 + col], dx1);
                }
                if (hh < H) dx0 = __builtin_fma((double)ga[hh], (double)s.w1[hh * s.in_pad + 3 + col], dx0);
                gdx[col] = (float)(dx0 + dx1);
            }
            __builtin_amdgcn_wave_barrier();
            // ---- table gradient: the lane that blended a column pair scatters it
            for (int q = c; 2 * q < level_cols; q += HSDF_GROUP) {
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
                const int wl = wide.lvl[l];
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
            for (int hh = c; hh < H; hh += HSDF_GROUP) { ga[hh] = 0.0f; gr[hh] = 0.0f; }
            for (int e = c; e < in_dim; e += HSDF_GROUP) gin[e] = 0.0f;
            if (c == 0) { s_g[grp] = 0.0f; s_sq[grp] = 0.0f; }
        }
        __syncthreads();
        // ---- weight gradients of this pass: the thread that owns an entry adds the samples up in order - in fp64, rounded into
        //      the fp32 partial sum once per pass
        for (int e = threadIdx.x; e < n_entries; e += blockDim.x) {
            double acc = 0.0;
            if (e < H * in_dim) {
                const int hh = e / in_dim, k = e - hh * in_dim;
                for (int q = 0; q < HST_GROUPS; ++q) acc = __builtin_fma((double)s_ga[q * H + hh], (double)s.in[q * s.stride + k], acc);
            } else if (e < H * in_dim + H) {
                const int hh = e - H * in_dim;
                for (int q = 0; q < HST_GROUPS; ++q) acc += (double)s_ga[q * H + hh];
            } else if (e < H * in_dim + 2 * H) {
                const int hh = e - H * in_dim - H;
                for (int q = 0; q < HST_GROUPS; ++q) acc += (double)s_gr[q * H + hh];
            } else if (e == H * in_dim + 2 * H) {
                for (int q = 0; q < HST_GROUPS; ++q) acc += (double)s_g[q];
            } else {
                for (int q = 0; q < HST_GROUPS; ++q) acc += (double)s_sq[q];
            }
            s_own[e] = (float)((double)s_own[e] + acc);
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < n_entries; e += blockDim.x) partials[(int64_t)blockIdx.x * row_stride + e] = s_own[e];
}

__global__ void __launch_bounds__(256)
hash_sdf_train_reduce_kernel(const float* __restrict__ partials, int rows, int row_stride, int H, int in_dim, float* __restrict__ gw1,
                             float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2, float* __restrict__ loss,
                             float inv_batch, HstWide wide, const double* __restrict__ wacc, float* __restrict__ grad_codebook) {
    // 16 lanes per entry: lane r adds rows r, r + 16, ... in order, then a fixed butterfly over the 16 lanes - in fp64, rounded once
    const int n_entries = H * in_dim + 2 * H + 2;
    const int r0 = threadIdx.x & 15;
    for (int e = blockIdx.x * 16 + (threadIdx.x >> 4); e < n_entries + 15; e += gridDim.x * 16) {      // (whole groups stay together)
        const bool in = e < n_entries;
        double sum = 0.0;
        if (in)
            for (int r = r0; r < rows; r += 16) sum += (double)partials[(int64_t)r * row_stride + e];
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 16);
        if (!in || r0 != 0) continue;
        const float acc = (float)sum;
        if (e < H * in_dim) gw1[e] += acc;
        else if (e < H * in_dim + H) gb1[e - H * in_dim] += acc;
        else if (e < H * in_dim + 2 * H) gw2[e - H * in_dim - H] += acc;
        else if (e == H * in_dim + 2 * H) gb2[0] += acc;
        else loss[0] = acc * inv_batch;
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
extern "C" int64_t wisp_hash_sdf_train_scratch_bytes(int64_t n, int num_lods, int feature_dim, int multiscale, int hidden) {
    if (n < 1 || num_lods < 1 || num_lods > HSDF_MAX_LODS || (feature_dim != 2 && feature_dim != 4 && feature_dim != 8) ||
        (multiscale != 0 && multiscale != 1) || hidden < 1 || hidden > HSDF_MAX_HIDDEN) return -1;
    const int cols = multiscale ? feature_dim : num_lods * feature_dim;
    if (cols > HSDF_MAX_COLS || hst_lds_bytes(hidden, cols, num_lods, feature_dim, multiscale) > HST_MAX_LDS) return -1;
    // the partial rows, then room for every level's fp64 accumulators (which levels are small depends on the resolutions)
    return (int64_t)hst_grid(n) * hst_row_stride(hidden, cols) * (int64_t)sizeof(float) +
           (int64_t)num_lods * HST_WIDE_ENTRIES * (int64_t)sizeof(double);
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
    const size_t lds = hst_lds_bytes(hidden, fld.cols, num_lods, feature_dim, multiscale);
    const int grid = hst_grid(n), row_stride = hst_row_stride(hidden, fld.cols), in_dim = 3 + fld.cols;
    float* partials = static_cast<float*>(scratch);
    double* wacc = reinterpret_cast<double*>(partials + (size_t)grid * row_stride);      // (row_stride is a multiple of 16 floats)
    HstWide wide;
    wide.n = 0;
    wide.off[0] = 0;
    for (int l = 0; l < HSDF_MAX_LODS; ++l) {
        wide.lvl[l] = -1;
        if (l >= num_lods || l * feature_dim >= zero_from_col) continue;
        const int64_t rows = begin_idxes[l + 1] - begin_idxes[l], entries = rows * feature_dim;
        // Every index the scatter can form must lie inside the level's own accumulators.  A hashed index is below 2^bitwidth <= rows
        // (hash_sdf_fill); a dense one reaches res^3 - 1, and hash_sdf_fill admits a dense level that declares fewer rows (the
        // forward and the f32 scatter pin into the whole table): such a level keeps the f32 scatter.  (From resolution 258 on an
        // index can be pinned to the table's last row; res^3 is then far above the threshold anyway.)
        const int64_t r = resolutions[l];
        if (entries > HST_WIDE_ENTRIES || r >= 258 || (fld.lv.dense[l] && rows < r * r * r)) continue;
        wide.lvl[l] = wide.n;
        wide.tbl[wide.n] = begin_idxes[l] * feature_dim;
        wide.off[wide.n + 1] = wide.off[wide.n] + entries;
        ++wide.n;
    }
    for (int i = wide.n + 1; i <= HSDF_MAX_LODS; ++i) wide.off[i] = wide.off[wide.n];
    for (int i = wide.n; i < HSDF_MAX_LODS; ++i) wide.tbl[i] = 0;
    const float inv_batch = 1.0f / (float)n;
    hipStream_t s = (hipStream_t)stream;
    if (const hipError_t e = WISP_ALLOW_LDS(hash_sdf_train_kernel, lds)) return wisp_fail(WISP_ERR_LAUNCH, __func__, hipGetErrorString(e));
    if (wide.off[wide.n] > 0 && hipMemsetAsync(wacc, 0, (size_t)wide.off[wide.n] * sizeof(double), s) != hipSuccess)
        return wisp_fail(WISP_ERR_LAUNCH, __func__, "hipMemsetAsync failed");
    hipLaunchKernelGGL(hash_sdf_train_kernel, dim3(grid), dim3(HST_BLOCK), lds, s, coords, gts, n, fld, inv_batch, grad_codebook,
                       partials, row_stride, wide, wacc);
    hipLaunchKernelGGL(hash_sdf_train_reduce_kernel, dim3((hst_entries(hidden, fld.cols) + 15) / 16), dim3(256), 0, s, partials, grid,
                       row_stride, hidden, in_dim, grad_w1, grad_b1, grad_w2, grad_b2, loss, inv_batch, wide, wacc, grad_codebook);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
