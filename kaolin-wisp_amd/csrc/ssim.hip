// Structural similarity of two fp32 images under a Gaussian window, in fp64 (replaces the host round trip through
// skimage.metrics.structural_similarity of wisp/ops/image/metrics.py:70-90; the definition is restated in include/wisp_hip.h).
//
// fp32 is not enough here: on a nearly flat region uxx - ux * ux cancels against C2 = 9e-4 and an fp32 map is off by 1e-4.  Every
// value is widened at the LDS read and all arithmetic after it is fp64; x * x and x * y of two fp32 values are exact in fp64.
//
// One workgroup of 256 threads = one 16 x 16 tile of one channel.  Both images' halo, (16 + 2r)^2 floats each, is staged in LDS
// with the boundary reflected AT THE LOAD (no branch per tap); a horizontal pass leaves the five row sums (x, y, xx, yy, xy) of
// every halo row in LDS as doubles, a vertical pass takes each thread's pixel from them.  The tile's sum over the cropped
// interior goes to the caller's scratch, and a second launch of one workgroup adds the tile sums of each channel in one fixed
// order: two calls over the same inputs give the same bits.  No floating-point atomics, no fences.
// The kernel is compiled twice: for the reference's window (radius 5: taps unrolled, 26 KB of LDS) and for any radius up to 15.
#include "wisp_common.h"

#define SSIM_T 16                                   // tile edge; SSIM_T * SSIM_T threads
#define SSIM_THREADS (SSIM_T * SSIM_T)
#define SSIM_MAX_R 15
#define SSIM_HALO_STRIDE 48                         // floats per halo row (>= 46): two 16-lane rows of one 32-lane LDS group share no bank

struct SsimArgs {
    const float* x;
    const float* y;
    int64_t x_row, x_pix, y_row, y_pix;
    int H, W, C, radius;
    int tiles_x, tiles;
    double cov_norm, c1, c2;
    double w[2 * SSIM_MAX_R + 1];
    double* map;                                    // [H, W, C] or null
    double* partials;                               // [C, tiles]
};

// The statistic of ONE pixel from its five window means - the one statement of the formula, for the mean and the map alike.
// Contraction is off: with it, ux * ux + uy * uy and 2 * (ux * uy) of identical images round differently and S is not exactly 1.
static __device__ __forceinline__ double ssim_pixel(double ux, double uy, double uxx, double uyy, double uxy, double cov_norm,
                                                    double c1, double c2) {
#pragma clang fp contract(off)
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    return ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
}

// scipy.ndimage's mode='reflect' (d c b a | a b c d | d c b a) for an index at most one image away; tiles that hang over the far
// edge ask for indices further out, whose pixels are never written: those are clamped so that the load stays inside the image
static __device__ __forceinline__ int ssim_reflect(int i, int n) {
    i = i < 0 ? -i - 1 : i;
    i = i >= n ? 2 * n - 1 - i : i;
    return min(max(i, 0), n - 1);
}

// sum of one double per thread over the workgroup in a fixed order (a tree over LDS); s_red: SSIM_THREADS doubles
static __device__ __forceinline__ double ssim_block_sum(double v, double* s_red) {
    s_red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int half = SSIM_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s_red[threadIdx.x] += s_red[threadIdx.x + half];
        __syncthreads();
    }
    return s_red[0];
}

// R > 0: the radius, known to the compiler; R == 0: a.radius, anything up to SSIM_MAX_R
template <int R>
__global__ void __launch_bounds__(SSIM_THREADS)
ssim_tile_kernel(const SsimArgs a) {
    constexpr int MAX_R = R > 0 ? R : SSIM_MAX_R, HALO = SSIM_T + 2 * MAX_R;
    __shared__ float s_x[HALO][SSIM_HALO_STRIDE];
    __shared__ float s_y[HALO][SSIM_HALO_STRIDE];
    __shared__ double s_h[5][HALO][SSIM_T];         // row sums of x, y, xx, yy, xy; afterwards the reduction's buffer
    __shared__ double s_w[2 * MAX_R + 1];
    const int tid = threadIdx.x, tx = tid & (SSIM_T - 1), ty = tid / SSIM_T;
    const int r = R > 0 ? R : a.radius, win = 2 * r + 1, halo = SSIM_T + 2 * r;
    const int c = blockIdx.y;
    const int tile = blockIdx.x;
    const int x0 = (tile % a.tiles_x) * SSIM_T, y0 = (tile / a.tiles_x) * SSIM_T;

    if (tid < win) s_w[tid] = a.w[tid];
    for (int i = tid; i < halo * halo; i += SSIM_THREADS) {
        const int hy = i / halo, hx = i - hy * halo;
        const int gy = ssim_reflect(y0 - r + hy, a.H), gx = ssim_reflect(x0 - r + hx, a.W);
        s_x[hy][hx] = a.x[(int64_t)gy * a.x_row + (int64_t)gx * a.x_pix + c];
        s_y[hy][hx] = a.y[(int64_t)gy * a.y_row + (int64_t)gx * a.y_pix + c];
    }
    __syncthreads();

    // horizontal pass: halo row `row`, output column tx
    for (int row = ty; row < halo; row += SSIM_T) {
        double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
        for (int k = 0; k < win; ++k) {
            const double w = s_w[k], px = (double)s_x[row][tx + k], py = (double)s_y[row][tx + k];
            hx = fma(w, px, hx);
            hy = fma(w, py, hy);
            hxx = fma(w, px * px, hxx);
            hyy = fma(w, py * py, hyy);
            hxy = fma(w, px * py, hxy);
        }
        s_h[0][row][tx] = hx; s_h[1][row][tx] = hy; s_h[2][row][tx] = hxx; s_h[3][row][tx] = hyy; s_h[4][row][tx] = hxy;
    }
    __syncthreads();

    // vertical pass: pixel (y0 + ty, x0 + tx)
    double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
#pragma unroll
    for (int k = 0; k < win; ++k) {
        const double w = s_w[k];
        ux = fma(w, s_h[0][ty + k][tx], ux);
        uy = fma(w, s_h[1][ty + k][tx], uy);
        uxx = fma(w, s_h[2][ty + k][tx], uxx);
        uyy = fma(w, s_h[3][ty + k][tx], uyy);
        uxy = fma(w, s_h[4][ty + k][tx], uxy);
    }
    const int py = y0 + ty, px = x0 + tx;
    double s = 0.0;
    if (py < a.H && px < a.W) {
        s = ssim_pixel(ux, uy, uxx, uyy, uxy, a.cov_norm, a.c1, a.c2);
        if (a.map) a.map[((int64_t)py * a.W + px) * a.C + c] = s;
        if (py < r || py >= a.H - r || px < r || px >= a.W - r) s = 0.0;     // the mean is over the crop [r, H - r) x [r, W - r)
    }
    __syncthreads();                                 // every read of s_h is done: it becomes the reduction's buffer
    const double tile_sum = ssim_block_sum(s, &s_h[0][0][0]);
    if (tid == 0) a.partials[(int64_t)c * a.tiles + tile] = tile_sum;
}

// One workgroup: out[ch] = the channel's tile sums, added in a fixed order, over the number of cropped pixels; out[C] = their mean.
__global__ void __launch_bounds__(SSIM_THREADS)
ssim_sum_kernel(const double* __restrict__ partials, int tiles, int C, double count, double* __restrict__ out) {
    __shared__ double s_red[SSIM_THREADS];
    double mean_of_channels = 0.0;                   // (thread 0's copy is the one written)
    for (int ch = 0; ch < C; ++ch) {
        double part = 0.0;
        for (int i = threadIdx.x; i < tiles; i += SSIM_THREADS) part += partials[(int64_t)ch * tiles + i];
        const double channel = ssim_block_sum(part, s_red) / count;
        __syncthreads();                             // (s_red[0] has been read by everyone before the next channel overwrites it)
        if (threadIdx.x == 0) out[ch] = channel;
        mean_of_channels += channel;
    }
    if (threadIdx.x == 0) out[C] = mean_of_channels / (double)C;
}

static inline int64_t ssim_tiles(int H, int W) { return ceil_div64(H, SSIM_T) * ceil_div64(W, SSIM_T); }

extern "C" int64_t wisp_ssim_scratch_bytes(int H, int W, int C) {
    if (H <= 0 || W <= 0 || C <= 0) return 0;
    return 8 * (int64_t)C * ssim_tiles(H, W);        // one double per channel and tile
}

extern "C" int wisp_ssim(const float* x, int64_t x_row_stride, int64_t x_pix_stride, const float* y, int64_t y_row_stride,
                         int64_t y_pix_stride, int H, int W, int C, int radius, const double* weights, double cov_norm, double c1,
                         double c2, double* out, double* map, void* scratch, int64_t scratch_bytes, wisp_stream_t stream) {
    WISP_REQUIRE(C >= 1 && C <= 4, "C must be 1..4");
    WISP_REQUIRE(radius >= 1 && radius <= SSIM_MAX_R, "radius must be 1..15");
    WISP_REQUIRE(H >= 2 * radius + 1 && W >= 2 * radius + 1, "image smaller than the window (H, W >= 2 * radius + 1)");
    WISP_REQUIRE(x && y && weights && out && scratch, "null pointer");
    WISP_REQUIRE(x_pix_stride >= C && y_pix_stride >= C, "pixel stride smaller than C");
    WISP_REQUIRE(x_row_stride >= (int64_t)(W - 1) * x_pix_stride + C && y_row_stride >= (int64_t)(W - 1) * y_pix_stride + C,
                 "row stride smaller than one row of pixels");
    WISP_REQUIRE((int64_t)H * x_row_stride < 0x80000000LL && (int64_t)H * y_row_stride < 0x80000000LL,
                 "image too large (H * row_stride must be below 2^31)");
    WISP_REQUIRE(scratch_bytes >= wisp_ssim_scratch_bytes(H, W, C), "scratch smaller than wisp_ssim_scratch_bytes");
    SsimArgs a;
    a.x = x; a.y = y;
    a.x_row = x_row_stride; a.x_pix = x_pix_stride; a.y_row = y_row_stride; a.y_pix = y_pix_stride;
    a.H = H; a.W = W; a.C = C; a.radius = radius;
    a.tiles_x = (int)ceil_div64(W, SSIM_T);
    a.tiles = (int)ssim_tiles(H, W);
    a.cov_norm = cov_norm; a.c1 = c1; a.c2 = c2;
    for (int k = 0; k < 2 * SSIM_MAX_R + 1; ++k) a.w[k] = k < 2 * radius + 1 ? weights[k] : 0.0;
    a.map = map;
    a.partials = (double*)scratch;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)a.tiles, (unsigned)C);
    if (radius == 5) hipLaunchKernelGGL(ssim_tile_kernel<5>, grid, dim3(SSIM_THREADS), 0, s, a);
    else hipLaunchKernelGGL(ssim_tile_kernel<0>, grid, dim3(SSIM_THREADS), 0, s, a);
    WISP_CHECK_LAUNCH();
    hipLaunchKernelGGL(ssim_sum_kernel, dim3(1), dim3(SSIM_THREADS), 0, s, a.partials, a.tiles, C,
                       (double)(H - 2 * radius) * (double)(W - 2 * radius), out);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
