// One optimisation step's forward + loss + backward of the reference's SDFTrainer (wisp/trainers/sdf_trainer.py:65-124, only_last)
// for a NeuralSDF over a TriplanarGrid (wisp/models/nefs/neural_sdf.py:120-155 over wisp/models/grids/triplanar_grid.py:97-146 and
// :205-233; nglod_triplanar.yaml: 'sum', one level of three 4 x 33 x 33 planes, [position, features] -> Linear(15, 128) -> relu ->
// Linear(128, 1), 512 coordinates per step):
//     pred = decoder([x, features(x)]) ;  loss = sum (pred - gt)^2 / B ;  backward
// The triplanar twin of wisp_hash_sdf_train_step (hash_sdf_train.hip), with the same two launches and conventions.  Through autograd
// over the modular ops the step is a triplane forward, a concatenation, two GEMMs with their elementwise companions, the loss, and
// all of that again backwards, ending in wisp_triplane_bwd; at 512 coordinates every one of those launches is launch latency.
//   triplane_sdf_train_kernel         16 lanes own a sample.  The forward is tri_sdf_point_inputs + tri_sdf_decode
//                                     (triplane_sdf_eval_dev.h), statement for statement: the predicted distance is bit for bit what
//                                     wisp_triplane_sdf_query returns for the same parameters.  Then g = 2 (pred - gt) / B and the
//                                     decoder backward of hash_sdf_train_kernel: lane c keeps hidden units c, c + 16, ..., the
//                                     gradient of the decoder's feature columns is a column sum over LDS.  The plane gradient is
//                                     scattered right there: the lane that blended column j recomputes the lookup's corner and
//                                     weights (tri_sdf_corner: tri_sdf_blend's statements, the same bits) and adds w_corner *
//                                     dfeat[j] to the texels it read; a corner the forward left out (x0 + 1 >= R or y0 + 1 >= R)
//                                     gets nothing.  'sum': every level receives the gradient of the summed column; 'cat': a column
//                                     belongs to one (level, plane, channel).  Nothing consumes d / d position: not computed.  Per
//                                     workgroup the decoder's weight gradients and the squared error are summed by the thread that
//                                     owns the entry, in sample order, and stored as one partial row - no atomics.
//   triplane_sdf_train_reduce_kernel  adds the partial rows up in workgroup order, ADDS the sums to the decoder's gradient tensors,
//                                     writes the loss, and rounds the fp64 plane accumulators (below) into the plane gradients.
// The sums over hidden units, samples and partial rows run in fp64 and are rounded to fp32 once each (products of two floats are
// exact in fp64).  The column sum, the owner-summed partial row and the reduce of the rows do not depend on the grid; they are
// RESTATED here from hash_sdf_train.hip, which is left as it is (lifting them into a shared header would have had to be shown not to
// move a bit of the hash step's results).
// Two scatter regimes per plane, with the hash step's threshold: a plane of at most 2^16 entries (feature_dim * R * R) - the shipped
// 4 x 33 x 33 plane, where 512 samples pile onto 1089 texels - takes its gradient through fp64 accumulators in scratch (TstWide
// below): exact fp64 products, fp64 atomic adds, one rounding per entry in the reduce kernel; the step zeroes the accumulators with
// one memset in front of the two launches.  A larger plane takes f32 atomic adds straight into its gradient tensor.
// Determinism: the loss and the four decoder gradients have a fixed summation order and are bitwise repeatable.  The plane
// gradients go through atomics in both regimes - fp64 atomics still arrive in any order: their sums are repeatable only where they
// are exact.
#include "wisp_common.h"
#include "triplane_sdf_eval_dev.h"

#define TST_BLOCK 256
#define TST_GROUPS (TST_BLOCK / TSDF_GROUP)            // samples per workgroup pass
#define TST_MAX_LDS (160 * 1024)                       // one workgroup may hold the whole LDS of a compute unit
#define TST_WIDE_ENTRIES (1 << 16)                     // a plane of at most this many entries is summed in fp64
#define TST_MAX_PLANES (TSDF_MAX_LODS * 3)

// The small planes' fp64 accumulators.  off[i] .. off[i + 1]: accumulators of the i-th such plane, plane[i]: its index in the
// field's plane list, slot[k]: the position of plane k in that list or -1 (f32 atomic adds into grad[k]).
struct TstWide {
    int64_t off[TST_MAX_PLANES + 1];
    int32_t plane[TST_MAX_PLANES];
    int32_t slot[TST_MAX_PLANES];
    int n;
};
struct TstGrads { float* grad[TST_MAX_PLANES]; };       // the gradient of every plane, in the order of TriSdfField::planes

static inline int tst_entries(int hidden, int cols) { return hidden * (3 + cols) + 2 * hidden + 2; }
static inline int tst_row_stride(int hidden, int cols) { return (tst_entries(hidden, cols) + 15) / 16 * 16; }
static inline int tst_grid(int64_t n) { return (int)min64(ceil_div64(n, TST_GROUPS), 1024); }
// LDS of a workgroup: what tri_sdf_stage lays out (weights, the groups' decoder inputs) | d loss / d pre-activation [groups][H] |
// d loss / d pred * relu output [groups][H] | d loss / d pred [groups] | squared error [groups] | d loss / d feature column
// [groups][cols] | the workgroup's partial row
static inline size_t tst_lds_bytes(int hidden, int cols) {
    return tri_sdf_lds_bytes(hidden, cols, TST_GROUPS) +
           ((size_t)TST_GROUPS * (2 * hidden + 2 + cols) + (size_t)tst_entries(hidden, cols)) * sizeof(float);
}
// the largest admitted shape, hidden 256 over 48 columns (51 inputs): 52224 (W1) + 2048 + 3264 (inputs) + 32768 + 128 + 3072 +
// 54280 (partial row) = 147784 bytes
static_assert(((size_t)TSDF_MAX_HIDDEN * ((3 + TSDF_MAX_COLS) | 1) + 2 * TSDF_MAX_HIDDEN + (size_t)TST_GROUPS * (3 + TSDF_MAX_COLS) +
               (size_t)TST_GROUPS * (2 * TSDF_MAX_HIDDEN + 2 + TSDF_MAX_COLS) +
               (size_t)TSDF_MAX_HIDDEN * (3 + TSDF_MAX_COLS) + 2 * TSDF_MAX_HIDDEN + 2) * sizeof(float) <= TST_MAX_LDS,
              "the largest shape (hidden 256, 48 columns) must fit one workgroup's LDS");

__global__ void __launch_bounds__(TST_BLOCK)
triplane_sdf_train_kernel(const float* __restrict__ coords, const float* __restrict__ gts, int64_t n, TriSdfField fld, float inv_batch,
                          TstGrads gp, float* __restrict__ partials /* [grid][row] */, int row_stride, TstWide wide,
                          double* __restrict__ wacc) {
    extern __shared__ float s_tst[];
    const TriSdfLds s = tri_sdf_stage(s_tst, fld);
    const int H = fld.hidden, cols = fld.cols, F = fld.feature_dim, F3 = 3 * F;
    const int in_dim = 3 + cols;
    float* s_ga = s.in + TST_GROUPS * s.stride;         // [groups][H]      d loss / d pre-activation
    float* s_gr = s_ga + TST_GROUPS * H;                // [groups][H]      d loss / d pred * relu output (for d w2)
    float* s_g = s_gr + TST_GROUPS * H;                 // [groups]         d loss / d pred
    float* s_sq = s_g + TST_GROUPS;                     // [groups]         squared error
    float* s_dx = s_sq + TST_GROUPS;                    // [groups][cols]   d loss / d feature column
    // partial sums of this workgroup: d W1 [H][in_dim], d b1 [H], d w2 [H], d b2, loss - in that order; every entry has one owner
    float* s_own = s_dx + TST_GROUPS * cols;            // [n_entries]
    const int n_entries = H * in_dim + 2 * H + 2;
    for (int e = threadIdx.x; e < n_entries; e += blockDim.x) s_own[e] = 0.0f;
    const int c = threadIdx.x & (TSDF_GROUP - 1), grp = threadIdx.x / TSDF_GROUP;
    float* gin = s.in + grp * s.stride;
    float* ga = s_ga + grp * H;
    float* gr = s_gr + grp * H;
    float* gdx = s_dx + grp * cols;
    const int64_t rounds = (n + TST_GROUPS - 1) / TST_GROUPS;
    __syncthreads();
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * TST_GROUPS + grp;
        if (i < n) {                                     // (a group enters or stays out as a whole: the shuffles are 16 wide)
            const float px = coords[i * 3], py = coords[i * 3 + 1], pz = coords[i * 3 + 2];
            // ---- forward: wisp_triplane_sdf_query's value
            tri_sdf_point_inputs(fld, gin, c, px, py, pz);
            const float pred = tri_sdf_decode<true>(fld, s, gin, c, ga, gr);
            float g, sq;
            {
#pragma clang fp contract(off)
                const float diff = pred - gts[i];
                g = 2.0f * diff * inv_batch;             // d [sum (pred - gt)^2 / B] / d pred
                sq = diff * diff;
                for (int hh = c; hh < H; hh += TSDF_GROUP) { ga[hh] *= g; gr[hh] *= g; }
            }
            if (c == 0) { s_g[grp] = g; s_sq[grp] = sq; }
            __builtin_amdgcn_wave_barrier();             // a group's lanes are in one wave: LDS order suffices
            // ---- gradient of the decoder input, feature columns only (nothing consumes d / d position), summed in fp64 (every
            //      product of two floats is exact there) and rounded once
            for (int col = c; col < cols; col += TSDF_GROUP) {
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
            // ---- plane gradient: the lane that blended a column scatters it (the column split of tri_sdf_point_inputs)
            for (int j = c; j < cols; j += TSDF_GROUP) {
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
            for (int hh = c; hh < H; hh += TSDF_GROUP) { ga[hh] = 0.0f; gr[hh] = 0.0f; }
            for (int e = c; e < in_dim; e += TSDF_GROUP) gin[e] = 0.0f;
            if (c == 0) { s_g[grp] = 0.0f; s_sq[grp] = 0.0f; }
        }
        __syncthreads();
        // ---- weight gradients of this pass: the thread that owns an entry adds the samples up in order - in fp64, rounded into
        //      the fp32 partial sum once per pass
        for (int e = threadIdx.x; e < n_entries; e += blockDim.x) {
            double acc = 0.0;
            if (e < H * in_dim) {
                const int hh = e / in_dim, k = e - hh * in_dim;
                for (int q = 0; q < TST_GROUPS; ++q) acc = __builtin_fma((double)s_ga[q * H + hh], (double)s.in[q * s.stride + k], acc);
            } else if (e < H * in_dim + H) {
                const int hh = e - H * in_dim;
                for (int q = 0; q < TST_GROUPS; ++q) acc += (double)s_ga[q * H + hh];
            } else if (e < H * in_dim + 2 * H) {
                const int hh = e - H * in_dim - H;
                for (int q = 0; q < TST_GROUPS; ++q) acc += (double)s_gr[q * H + hh];
            } else if (e == H * in_dim + 2 * H) {
                for (int q = 0; q < TST_GROUPS; ++q) acc += (double)s_g[q];
            } else {
                for (int q = 0; q < TST_GROUPS; ++q) acc += (double)s_sq[q];
            }
            s_own[e] = (float)((double)s_own[e] + acc);
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < n_entries; e += blockDim.x) partials[(int64_t)blockIdx.x * row_stride + e] = s_own[e];
}

__global__ void __launch_bounds__(256)
triplane_sdf_train_reduce_kernel(const float* __restrict__ partials, int rows, int row_stride, int H, int in_dim,
                                 float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2,
                                 float* __restrict__ loss, float inv_batch, TstWide wide, const double* __restrict__ wacc, TstGrads gp) {
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
    // the small planes' fp64 sums, rounded once and ADDED to the plane gradient (an untouched accumulator leaves its entry alone)
    const int64_t total = wide.off[wide.n];
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const double v = wacc[e];
        if (v == 0.0) continue;
        int i = 0;
        while (e >= wide.off[i + 1]) ++i;
        gp.grad[wide.plane[i]][e - wide.off[i]] += (float)v;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
// the shape rules of tri_sdf_fill, without the pointers: the feature columns, or -1
static inline int tst_cols(const int32_t* sizes, int num_lods, int feature_dim, int multiscale, int hidden) {
    if (!sizes || num_lods < 1 || num_lods > TSDF_MAX_LODS || feature_dim < 1 || (multiscale != 0 && multiscale != 1) || hidden < 1 ||
        hidden > TSDF_MAX_HIDDEN) return -1;
    const int64_t cols = (int64_t)(multiscale ? 1 : num_lods) * 3 * feature_dim;
    if (cols > TSDF_MAX_COLS || tst_lds_bytes(hidden, (int)cols) > TST_MAX_LDS) return -1;
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
        if (entries <= TST_WIDE_ENTRIES) wide += 3 * entries;
    }
    return (int64_t)tst_grid(n) * tst_row_stride(hidden, cols) * (int64_t)sizeof(float) + wide * (int64_t)sizeof(double);
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
                                    TST_GROUPS)) return rc;
    WISP_REQUIRE(coords && gts && grad_planes && grad_w1 && grad_b1 && grad_w2 && grad_b2 && loss && scratch, "null pointer");
    for (int k = 0; k < num_lods * 3; ++k) WISP_REQUIRE(grad_planes[k], "null plane gradient pointer");
    const int64_t need = wisp_triplane_sdf_train_scratch_bytes(n, sizes, num_lods, feature_dim, multiscale, hidden);
    WISP_REQUIRE(need >= 0, "LDS budget exceeded");
    WISP_REQUIRE(scratch_bytes >= need, "scratch too small (wisp_triplane_sdf_train_scratch_bytes)");
    const size_t lds = tst_lds_bytes(hidden, fld.cols);
    const int grid = tst_grid(n), row_stride = tst_row_stride(hidden, fld.cols), in_dim = 3 + fld.cols;
    float* partials = static_cast<float*>(scratch);
    double* wacc = reinterpret_cast<double*>(partials + (size_t)grid * row_stride);      // (row_stride is a multiple of 16 floats)
    TstWide wide;
    TstGrads gp;
    wide.n = 0;
    wide.off[0] = 0;
    for (int k = 0; k < TST_MAX_PLANES; ++k) {
        wide.slot[k] = -1;
        gp.grad[k] = k < num_lods * 3 ? grad_planes[k] : nullptr;
        if (k >= num_lods * 3) continue;
        // every offset the scatter can form lies inside the plane: channel < feature_dim, x0 and y0 in [0, R - 1], and a corner at
        // x0 + 1 or y0 + 1 is written only where it is below R
        const int64_t entries = tst_plane_entries(feature_dim, sizes[k / 3]);
        if (entries > TST_WIDE_ENTRIES) continue;
        wide.slot[k] = wide.n;
        wide.plane[wide.n] = k;
        wide.off[wide.n + 1] = wide.off[wide.n] + entries;
        ++wide.n;
    }
    for (int i = wide.n + 1; i <= TST_MAX_PLANES; ++i) wide.off[i] = wide.off[wide.n];
    for (int i = wide.n; i < TST_MAX_PLANES; ++i) wide.plane[i] = 0;
    const float inv_batch = 1.0f / (float)n;
    hipStream_t s = (hipStream_t)stream;
    if (const hipError_t e = WISP_ALLOW_LDS(triplane_sdf_train_kernel, lds)) return wisp_fail(WISP_ERR_LAUNCH, __func__, hipGetErrorString(e));
    if (wide.off[wide.n] > 0 && hipMemsetAsync(wacc, 0, (size_t)wide.off[wide.n] * sizeof(double), s) != hipSuccess)
        return wisp_fail(WISP_ERR_LAUNCH, __func__, "hipMemsetAsync failed");
    hipLaunchKernelGGL(triplane_sdf_train_kernel, dim3(grid), dim3(TST_BLOCK), lds, s, coords, gts, n, fld, inv_batch, gp, partials,
                       row_stride, wide, wacc);
    hipLaunchKernelGGL(triplane_sdf_train_reduce_kernel, dim3((tst_entries(hidden, fld.cols) + 15) / 16), dim3(256), 0, s, partials, grid,
                       row_stride, hidden, in_dim, grad_w1, grad_b1, grad_w2, grad_b2, loss, inv_batch, wide, wacc, gp);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
