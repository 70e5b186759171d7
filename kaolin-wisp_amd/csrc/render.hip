// Packed (ragged) volume integration for gfx950.
//
// Replaces kaolin.render.spc.{cumsum, sum_reduce, exponential_integration} and the scatter block of
// PackedRFTracer.trace (wisp/tracers/packed_rf_tracer.py:143-165; semantics SURVEY.md Appendix A.4/A.5).
// The reference runs exp, a CUB scan, a multiply, three atomic segmented reductions and four index_put
// kernels; here one wave owns one pack (= one ray's samples): the exclusive transmittance sum is a 64-lane
// shuffle scan carried across 64-sample chunks, the per-ray colour / alpha / depth sums are wave
// reductions (deterministic, no atomics), and background blending + the scatter to per-ray buffers are
// fused into the same kernel.
#include "wisp_common.h"
#include "raygen_dev.h"
#include "step_tail_dev.h"
#include "sphere_trace_dev.h"

// Wave-wide inclusive scan / sum on the VALU (DPP), no LDS traffic: Hillis-Steele inside each 16-lane row (row_shr 1, 2, 4, 8),
// then the row totals travel with row_bcast:15 (into rows 1 and 3) and row_bcast:31 (into rows 2 and 3).  Lanes without a
// source add 0.  These kernels run one wave per ray and are bound by the LATENCY of their dependent chain - with
// ds_bpermute shuffles (~100+ cycles each, 30-50 per ray) that chain was most of the kernel.
#define WISP_DPP_ADD(V, CTRL, RMASK)                                                                                  \
    V += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, V), CTRL, RMASK, 0xf, false))
static __device__ __forceinline__ float wave_incl_scan_f(float v, int /*lane*/) {
    WISP_DPP_ADD(v, 0x111, 0xf);      // row_shr:1
    WISP_DPP_ADD(v, 0x112, 0xf);      // row_shr:2
    WISP_DPP_ADD(v, 0x114, 0xf);      // row_shr:4
    WISP_DPP_ADD(v, 0x118, 0xf);      // row_shr:8
    WISP_DPP_ADD(v, 0x142, 0xa);      // row_bcast:15 -> rows 1, 3
    WISP_DPP_ADD(v, 0x143, 0xc);      // row_bcast:31 -> rows 2, 3
    return v;
}
#undef WISP_DPP_ADD

static __device__ __forceinline__ float wave_last_f(float v) {      // value of lane 63, wave-uniform
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

static __device__ __forceinline__ float wave_sum_f(float v) { return wave_last_f(wave_incl_scan_f(v, 0)); }

// ---------------------------------------------------------------------------------------------- generic pack ops
__global__ void __launch_bounds__(256)
packed_sum_reduce_kernel(const float* __restrict__ feats, int64_t s_total, int channels,
                         const int64_t* __restrict__ pack_starts, int64_t num_packs, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= num_packs) return;
    const int64_t b = pack_starts[p], e = (p + 1 < num_packs) ? pack_starts[p + 1] : s_total;
    for (int c = 0; c < channels; ++c) {
        float acc = 0.0f;
        for (int64_t i = b + lane; i < e; i += 64) acc += feats[i * channels + c];
        acc = wave_sum_f(acc);
        if (lane == 0) out[p * channels + c] = acc;
    }
}

__global__ void __launch_bounds__(256)
packed_cumsum_kernel(const float* __restrict__ feats, int64_t s_total, int channels,
                     const int64_t* __restrict__ pack_starts, int64_t num_packs, int exclusive, int reverse,
                     float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= num_packs) return;
    const int64_t b = pack_starts[p], e = (p + 1 < num_packs) ? pack_starts[p + 1] : s_total;
    const int64_t len = e - b;
    for (int c = 0; c < channels; ++c) {
        float carry = 0.0f;
        for (int64_t k0 = 0; k0 < len; k0 += 64) {
            const int64_t k = k0 + lane;
            const int64_t i = reverse ? (e - 1 - k) : (b + k);
            const float v = (k < len) ? feats[i * channels + c] : 0.0f;
            const float inc = wave_incl_scan_f(v, lane);
            if (k < len) out[i * channels + c] = carry + (exclusive ? inc - v : inc);
            carry += wave_last_f(inc);
        }
    }
}

extern "C" int wisp_packed_sum_reduce(const float* feats, int64_t num_samples, int channels, const int64_t* pack_starts,
                                      int64_t num_packs, float* out, wisp_stream_t stream) {
    WISP_REQUIRE(num_samples >= 0 && num_packs >= 0 && channels >= 1, "bad sizes");
    if (num_packs == 0) return WISP_OK;
    WISP_REQUIRE(feats && pack_starts && out, "null pointer");
    hipLaunchKernelGGL(packed_sum_reduce_kernel, dim3((unsigned)ceil_div64(num_packs, 4)), dim3(256), 0,
                       (hipStream_t)stream, feats, num_samples, channels, pack_starts, num_packs, out);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_packed_cumsum(const float* feats, int64_t num_samples, int channels, const int64_t* pack_starts,
                                  int64_t num_packs, int exclusive, int reverse, float* out, wisp_stream_t stream) {
    WISP_REQUIRE(num_samples >= 0 && num_packs >= 0 && channels >= 1, "bad sizes");
    if (num_packs == 0) return WISP_OK;
    WISP_REQUIRE(feats && pack_starts && out, "null pointer");
    hipLaunchKernelGGL(packed_cumsum_kernel, dim3((unsigned)ceil_div64(num_packs, 4)), dim3(256), 0,
                       (hipStream_t)stream, feats, num_samples, channels, pack_starts, num_packs, exclusive, reverse, out);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

// ---------------------------------------------------------------------------------------------- fused compositing
struct Bg { float r, g, b; };

// One wave per ray, ONE wave per workgroup: these kernels are bound by the latency of a ray's dependent chain, and a
// workgroup of several rays holds its slots until its longest ray is done (4 -> 1 waves per workgroup: -2 us per kernel).
#define PACK_WAVES 1

__global__ void __launch_bounds__(256)
composite_init_kernel(int64_t num_rays, Bg bg, float* __restrict__ rgb, float* __restrict__ alpha,
                      float* __restrict__ depth, uint8_t* __restrict__ hit) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= num_rays) return;
    rgb[r * 3] = bg.r; rgb[r * 3 + 1] = bg.g; rgb[r * 3 + 2] = bg.b;     // packed_rf_tracer.py:143
    alpha[r] = 0.0f;
    if (depth) depth[r] = 0.0f;
    hit[r] = 0;
}

// BY_RAY = false: pack p covers samples [pack_starts[p], pack_starts[p+1]) and its ray is ridx[first sample].
// BY_RAY = true : `pack_starts` is the per-ray offset table [R+1]; wave r handles ray r and also writes the
//                 background for rays without samples, so no init pass, no boundary->starts compaction and no
//                 device->host read of the pack count are needed.
template <bool BY_RAY>
__global__ void __launch_bounds__(256)
composite_fwd_kernel(const float* __restrict__ color, const float* __restrict__ density,
                     const float* __restrict__ deltas, const float* __restrict__ depths,
                     const int64_t* __restrict__ ridx, const int64_t* __restrict__ pack_starts, int64_t num_packs,
                     int64_t s_total, Bg bg, float* __restrict__ out_rgb, float* __restrict__ out_alpha,
                     float* __restrict__ out_depth, uint8_t* __restrict__ out_hit, float* __restrict__ weights) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= num_packs) return;
    const int64_t b = pack_starts[p], e = (BY_RAY || p + 1 < num_packs) ? pack_starts[p + 1] : s_total;
    if (BY_RAY && b == e) {
        if (lane == 0) {
            out_alpha[p] = 0.0f; out_hit[p] = 0;
            out_rgb[p * 3] = bg.r; out_rgb[p * 3 + 1] = bg.g; out_rgb[p * 3 + 2] = bg.b;
            if (out_depth) out_depth[p] = 0.0f;
        }
        return;
    }
    float carry = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, sd = 0.0f;
    for (int64_t k0 = b; k0 < e; k0 += 64) {
        const int64_t i = k0 + lane;
        const bool live = i < e;
        const float tau = live ? density[i] * deltas[i] : 0.0f;           // :152
        const float inc = wave_incl_scan_f(tau, lane);
        const float excl = carry + (inc - tau);
        carry += wave_last_f(inc);
        if (live) {
            const float T = expf(-excl);                                  // exponential_integration, exclusive=True
            const float w = T * (1.0f - expf(-tau));
            weights[i] = w;
            sr += w * color[i * 3]; sg += w * color[i * 3 + 1]; sb += w * color[i * 3 + 2];
            sa += w;
            if (depths) sd += w * depths[i];
        }
    }
    sr = wave_sum_f(sr); sg = wave_sum_f(sg); sb = wave_sum_f(sb); sa = wave_sum_f(sa);
    if (depths) sd = wave_sum_f(sd);
    if (lane == 0) {
        const int64_t r = BY_RAY ? p : ridx[b];
        out_alpha[r] = sa;                                                // :160-161
        out_hit[r] = sa > 0.0f ? 1 : 0;                                   // :162
        const float om = 1.0f - sa;
        out_rgb[r * 3] = bg.r * om + sr; out_rgb[r * 3 + 1] = bg.g * om + sg; out_rgb[r * 3 + 2] = bg.b * om + sb;  // :165
        if (out_depth) out_depth[r] = sd;                                 // :157-158
    }
}

// dL/dc_i = w_i g_rgb ; G_i = g_rgb.(c_i - bg) + g_alpha + g_depth t_i ;
// dL/dtau_i = G_i T_i exp(-tau_i) - sum_{k>i} G_k w_k ; dL/dsigma_i = dL/dtau_i * delta_i
template <bool BY_RAY>
__global__ void __launch_bounds__(256)
composite_bwd_kernel(const float* __restrict__ grad_rgb, const float* __restrict__ grad_alpha,
                     const float* __restrict__ grad_depth, const float* __restrict__ color,
                     const float* __restrict__ density, const float* __restrict__ deltas,
                     const float* __restrict__ depths, const int64_t* __restrict__ ridx,
                     const int64_t* __restrict__ pack_starts, int64_t num_packs, int64_t s_total, Bg bg,
                     float* __restrict__ grad_color, float* __restrict__ grad_density) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= num_packs) return;
    const int64_t b = pack_starts[p], e = (BY_RAY || p + 1 < num_packs) ? pack_starts[p + 1] : s_total;
    if (BY_RAY && b == e) return;
    const int64_t r = BY_RAY ? p : ridx[b];
    const float gr = grad_rgb[r * 3], gg = grad_rgb[r * 3 + 1], gb = grad_rgb[r * 3 + 2];
    const float ga = grad_alpha ? grad_alpha[r] : 0.0f;
    const float gd = (grad_depth && depths) ? grad_depth[r] : 0.0f;
    // pass 1: total of G_k w_k over the pack
    float carry = 0.0f, tot = 0.0f;
    for (int64_t k0 = b; k0 < e; k0 += 64) {
        const int64_t i = k0 + lane;
        const bool live = i < e;
        const float tau = live ? density[i] * deltas[i] : 0.0f;
        const float inc = wave_incl_scan_f(tau, lane);
        const float excl = carry + (inc - tau);
        carry += wave_last_f(inc);
        if (live) {
            const float w = expf(-excl) * (1.0f - expf(-tau));
            float G = gr * (color[i * 3] - bg.r) + gg * (color[i * 3 + 1] - bg.g) + gb * (color[i * 3 + 2] - bg.b) + ga;
            if (depths) G += gd * depths[i];
            tot += G * w;
        }
    }
    tot = wave_sum_f(tot);
    // pass 2: gradients, suffix = total - inclusive prefix of G w
    carry = 0.0f;
    float gcarry = 0.0f;
    for (int64_t k0 = b; k0 < e; k0 += 64) {
        const int64_t i = k0 + lane;
        const bool live = i < e;
        const float dl = live ? deltas[i] : 0.0f;
        const float tau = live ? density[i] * dl : 0.0f;
        const float inc = wave_incl_scan_f(tau, lane);
        const float excl = carry + (inc - tau);
        carry += wave_last_f(inc);
        float T = 0.0f, et = 0.0f, w = 0.0f, G = 0.0f;
        if (live) {
            T = expf(-excl); et = expf(-tau); w = T * (1.0f - et);
            G = gr * (color[i * 3] - bg.r) + gg * (color[i * 3 + 1] - bg.g) + gb * (color[i * 3 + 2] - bg.b) + ga;
            if (depths) G += gd * depths[i];
        }
        const float gw = G * w;
        const float ginc = wave_incl_scan_f(gw, lane);
        const float suffix = tot - (gcarry + ginc);
        gcarry += wave_last_f(ginc);
        if (live) {
            grad_color[i * 3] = w * gr; grad_color[i * 3 + 1] = w * gg; grad_color[i * 3 + 2] = w * gb;
            grad_density[i] = (G * T * et - suffix) * dl;
        }
    }
}

extern "C" int wisp_composite_fwd(const float* color, const float* density, const float* deltas, const float* depths,
                                  const int64_t* ridx, const int64_t* pack_starts, int64_t num_packs,
                                  int64_t num_samples, int64_t num_rays, const float* bg, float* out_rgb,
                                  float* out_alpha, float* out_depth, uint8_t* out_hit, float* weights,
                                  wisp_stream_t stream) {
    WISP_REQUIRE(num_rays >= 0 && num_packs >= 0 && num_samples >= 0, "bad sizes");
    WISP_REQUIRE(bg, "null bg");
    if (num_rays == 0) return WISP_OK;
    WISP_REQUIRE(out_rgb && out_alpha && out_hit, "null output");
    WISP_REQUIRE(out_depth == nullptr || depths != nullptr, "out_depth needs depths");
    hipStream_t s = (hipStream_t)stream;
    const Bg b{bg[0], bg[1], bg[2]};
    if (ridx == nullptr) {      // per-ray offsets mode: pack_starts = ray_offsets [num_rays + 1], num_packs must equal num_rays
        WISP_REQUIRE(pack_starts && num_packs == num_rays, "ray-offset mode needs offsets[R+1] and num_packs == num_rays");
        WISP_REQUIRE(num_samples == 0 || (color && density && deltas && weights), "null pointer");
        hipLaunchKernelGGL(composite_fwd_kernel<true>, dim3((unsigned)ceil_div64(num_rays, PACK_WAVES)), dim3(64 * PACK_WAVES), 0, s, color,
                           density, deltas, out_depth ? depths : nullptr, ridx, pack_starts, num_rays, num_samples, b,
                           out_rgb, out_alpha, out_depth, out_hit, weights);
        WISP_CHECK_LAUNCH();
        return WISP_OK;
    }
    hipLaunchKernelGGL(composite_init_kernel, dim3((unsigned)ceil_div64(num_rays, 256)), dim3(256), 0, s, num_rays, b,
                       out_rgb, out_alpha, out_depth, out_hit);
    if (num_packs > 0) {
        WISP_REQUIRE(color && density && deltas && ridx && pack_starts && weights, "null pointer");
        hipLaunchKernelGGL(composite_fwd_kernel<false>, dim3((unsigned)ceil_div64(num_packs, 4)), dim3(256), 0, s, color,
                           density, deltas, out_depth ? depths : nullptr, ridx, pack_starts, num_packs, num_samples, b,
                           out_rgb, out_alpha, out_depth, out_hit, weights);
    }
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_composite_bwd(const float* grad_rgb, const float* grad_alpha, const float* grad_depth,
                                  const float* color, const float* density, const float* deltas, const float* depths,
                                  const int64_t* ridx, const int64_t* pack_starts, int64_t num_packs,
                                  int64_t num_samples, const float* bg, float* grad_color, float* grad_density,
                                  wisp_stream_t stream) {
    WISP_REQUIRE(num_packs >= 0 && num_samples >= 0 && bg, "bad sizes");
    if (num_packs == 0) return WISP_OK;
    WISP_REQUIRE(grad_rgb && color && density && deltas && pack_starts && grad_color && grad_density, "null pointer");
    const Bg b{bg[0], bg[1], bg[2]};
    if (ridx == nullptr)        // per-ray offsets mode (see wisp_composite_fwd): num_packs = number of rays
        hipLaunchKernelGGL(composite_bwd_kernel<true>, dim3((unsigned)ceil_div64(num_packs, PACK_WAVES)), dim3(64 * PACK_WAVES), 0,
                           (hipStream_t)stream, grad_rgb, grad_alpha, grad_depth, color, density, deltas, depths, ridx,
                           pack_starts, num_packs, num_samples, b, grad_color, grad_density);
    else
        hipLaunchKernelGGL(composite_bwd_kernel<false>, dim3((unsigned)ceil_div64(num_packs, 4)), dim3(256), 0,
                           (hipStream_t)stream, grad_rgb, grad_alpha, grad_depth, color, density, deltas, depths, ridx,
                           pack_starts, num_packs, num_samples, b, grad_color, grad_density);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

// ---------------------------------------------------------------------------------------------- sphere-tracing helper
// find_depth_bound (wisp/csrc/render/find_depth_bound_cuda.cu:16-45): for every ray (pack) advance its current nugget
// index to the first nugget whose [entry, exit] contains, or lies beyond, the query depth; -1 when there is none.
// Bug-compatible with the reference on purpose: the search of pack i is bounded by the CURRENT index of pack i+1
// (not that pack's first nugget), and the last pack is bounded by num_packs rather than num_nugs (.cu:29).
// One deliberate difference: a finished neighbour (-1) makes that bound 0xFFFFFFFF and the reference then reads past the end
// of `depth` when the query lies beyond every remaining nugget (undefined there); here the scan also stops at num_nugs -> -1.
__global__ void __launch_bounds__(256)
find_depth_bound_kernel(int64_t num_packs, int64_t num_nugs, const float* __restrict__ query,
                        const int32_t* __restrict__ curr_in, int32_t* __restrict__ curr_out,
                        const float* __restrict__ depth) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_packs) return;
    int32_t result = -1;
    const int32_t start = curr_in[t];
    if (start > -1) {
        uint32_t i = (uint32_t)start;
        uint32_t stop = (t == num_packs - 1) ? (uint32_t)num_packs : (uint32_t)curr_in[t + 1];
        if ((int64_t)stop > num_nugs) stop = (uint32_t)num_nugs;
        const float q = query[t];
        while (i < stop) {
            const float entry = depth[2 * (int64_t)i], exit_ = depth[2 * (int64_t)i + 1];
            if ((q >= entry && q <= exit_) || q < entry) { result = (int32_t)i; break; }
            ++i;
        }
    }
    curr_out[t] = result;
}

extern "C" int wisp_find_depth_bound(const float* query, const int32_t* curr_idxes, const float* nug_depth,
                                     int64_t num_packs, int64_t num_nugs, int32_t* out, wisp_stream_t stream) {
    WISP_REQUIRE(num_packs >= 0 && num_nugs >= 0, "bad sizes");
    if (num_packs == 0) return WISP_OK;
    WISP_REQUIRE(query && curr_idxes && nug_depth && out, "null pointer");
    hipLaunchKernelGGL(find_depth_bound_kernel, dim3((unsigned)ceil_div64(num_packs, 256)), dim3(256), 0, (hipStream_t)stream,
                       num_packs, num_nugs, query, curr_idxes, out, nug_depth);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

// ---------------------------------------------------------------------------------------------- fused sphere-trace step
// One iteration of PackedSDFTracer.trace's marching loop (wisp/tracers/packed_sdf_tracer.py:118-146) for every active
// ray in ONE launch, one thread per pack: sphere_trace_step (sphere_trace_dev.h; find_depth_bound with the same bounds quirks
// as above).  The reference issues ~25 masked torch kernels per iteration for this.
__global__ void __launch_bounds__(256)
sphere_trace_step_kernel(SphereTraceState st) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= st.num_packs) return;
    float px, py, pz;
    sphere_trace_step(st, p, true, px, py, pz);
}

extern "C" int wisp_sphere_trace_step(int64_t num_packs, const float* nug_o, const float* nug_d, const float* nug_depth,
                                      const int32_t* nug_pidx, float dist_max, float thr_close, float thr_avg, float* t,
                                      const float* dist,
                                      float* dist_prev, uint8_t* mask, uint8_t* hit, const int32_t* curr_in,
                                      int32_t* curr_out, int64_t* curr_pidx, float* x, wisp_stream_t stream) {
    WISP_REQUIRE(num_packs >= 0, "negative count");
    if (num_packs == 0) return WISP_OK;
    const SphereTraceState st{num_packs, nug_o, nug_d, nug_depth, nug_pidx, dist_max, thr_close, thr_avg, t,
                              const_cast<float*>(dist), dist_prev, mask, hit, curr_in, curr_out, curr_pidx, x};   // (dist is only read here)
    WISP_REQUIRE(sphere_trace_state_complete(st), "null pointer");
    hipLaunchKernelGGL(sphere_trace_step_kernel, dim3((unsigned)ceil_div64(num_packs, 256)), dim3(256), 0, (hipStream_t)stream, st);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

// ---------------------------------------------------------------------------------------------- ray generation
// generate_pinhole_rays / generate_ortho_rays (wisp/ops/raygen/raygen.py:40-119) for one camera: pixel coordinates ->
// principal-point shift -> NDC -> camera-space ray -> world space (inverse of the view transform: R^T (p - t)) ->
// normalised direction.  Every step is a separately rounded fp32 operation, in the reference's order.
// The per-pixel arithmetic lives in raygen_dev.h (wisp_camera_ray): wisp_multiview_sample (dataset.hip) makes the same rays.
template <bool ORTHO>
__global__ void __launch_bounds__(256)
raygen_kernel(const float* __restrict__ pixel_x, const float* __restrict__ pixel_y, int64_t n, RayCam cam,
              float* __restrict__ origins, float* __restrict__ dirs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float ow[3], dn[3];
    wisp_camera_ray<ORTHO>(pixel_x[i], pixel_y[i], cam, ow, dn);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        origins[i * 3 + c] = ow[c];
        dirs[i * 3 + c] = dn[c];
    }
}

extern "C" int wisp_generate_rays(const float* pixel_x, const float* pixel_y, int64_t num_pixels, int ortho, float x0,
                                  float y0, float width, float height, float scale_x, float scale_y,
                                  const float* view_rotation, const float* view_translation, float* origins, float* dirs,
                                  wisp_stream_t stream) {
    WISP_REQUIRE(num_pixels >= 0, "negative count");
    if (num_pixels == 0) return WISP_OK;
    WISP_REQUIRE(pixel_x && pixel_y && view_rotation && view_translation && origins && dirs, "null pointer");
    WISP_REQUIRE(width > 0.0f && height > 0.0f, "bad image size");
    RayCam cam;
    cam.x0 = x0; cam.y0 = y0; cam.width = width; cam.height = height; cam.sx = scale_x; cam.sy = scale_y;
    for (int k = 0; k < 9; ++k) cam.r[k] = view_rotation[k];             // host arrays
    for (int k = 0; k < 3; ++k) cam.t[k] = view_translation[k];
    const dim3 grid((unsigned)ceil_div64(num_pixels, 256));
    if (ortho)
        hipLaunchKernelGGL(raygen_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, pixel_x, pixel_y, num_pixels, cam, origins, dirs);
    else
        hipLaunchKernelGGL(raygen_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, pixel_x, pixel_y, num_pixels, cam, origins, dirs);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

// ---------------------------------------------------------------------------------------------- photometric loss
// mean over all elements of huber (smooth-L1, beta = 1) / L2 / L1 between the composited colours and the ground truth
// (MultiviewTrainer.step, wisp/trainers/multiview_trainer.py:140-154) together with its gradient w.r.t. the colours:
// d loss / d rgb = clamp(x, -1, 1) / N, 2 x / N, sign(x) / N for x = rgb - gt.  A grid-stride pass writes the gradient and one
// partial sum per workgroup; a one-workgroup second launch adds the partials in index order - reproducible value.
// (Until round 3 the workgroup that finished last did that inside the first launch - device-scope fence + ticket per workgroup.
//  On this part such a fence writes back and invalidates an XCD's L2; see composite_loss_kernel for what 8192 of them cost.)
#define LOSS_BLOCKS 256
__global__ void __launch_bounds__(256)
rgb_loss_kernel(const float* __restrict__ rgb, const float* __restrict__ gt, int64_t n, int kind, float inv_n,
                float* __restrict__ grad, float* __restrict__ partial) {
    __shared__ float part[4];
    float acc = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float x = rgb[i] - gt[i];
        float l, g;
        if (kind == 0) { const float a = fabsf(x); l = a < 1.0f ? 0.5f * x * x : a - 0.5f; g = fminf(fmaxf(x, -1.0f), 1.0f); }
        else if (kind == 1) { l = x * x; g = 2.0f * x; }
        else { l = fabsf(x); g = (x > 0.0f) ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
        acc += l;
        grad[i] = g * inv_n;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// one workgroup adds the partials in a fixed order: wisp_tail::loss_sum, step_tail_dev.h (the same body runs as a side workgroup of the
// hash-grid reduce launch in the native training step)
__global__ void __launch_bounds__(STEP_TAIL_THREADS)
loss_sum_kernel(const float* __restrict__ partial, int n, float inv_n, float* __restrict__ loss) {
    __shared__ float part[STEP_TAIL_LOSS_LDS_FLOATS];
    wisp_tail::loss_sum(partial, n, inv_n, loss, (int)threadIdx.x, part);
}

extern "C" int wisp_loss_sum(const float* partials, int num_partials, float inv_n, float* loss, wisp_stream_t stream) {
    WISP_REQUIRE(partials && num_partials >= 0 && loss, "bad arguments");
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, num_partials, inv_n, loss);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_rgb_loss(const float* rgb, const float* gt, int64_t num_elements, int kind, float* grad, float* loss,
                             float* workspace, wisp_stream_t stream) {
    WISP_REQUIRE(num_elements > 0 && rgb && gt && grad && loss && workspace, "bad arguments");
    WISP_REQUIRE(kind >= 0 && kind <= 2, "kind: 0 huber, 1 l2, 2 l1");
    const int blocks = (int)min64(ceil_div64(num_elements, 256), LOSS_BLOCKS);
    const float inv_n = 1.0f / (float)num_elements;
    hipLaunchKernelGGL(rgb_loss_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rgb, gt, num_elements, kind, inv_n, grad,
                       workspace + 1);
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, workspace + 1, blocks, inv_n, loss);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

// ---------------------------------------------------------------------------------------------- composite + loss + backward
// The three launches a training step makes between the decoder's forward and backward - compositing (packed_rf_tracer.py:143-165),
// the photometric loss with its gradient (multiview_trainer.py:140-154) and the compositing backward - as ONE pass per ray: a
// wave composites its ray, forms the loss terms and d loss / d rgb of that ray on the spot and runs the backward recurrences
// while the ray's samples are still in registers (rays of at most 64 samples, the usual case) or in cache (longer rays: the
// same two extra passes as composite_bwd_kernel).  What the separate kernels wrote only for each other never reaches memory:
// the weights, rgb / alpha / hit and the colour gradient per ray.  Same arithmetic, same order, per ray; the loss is the sum of
// per-workgroup partials added in index order by a one-wave second launch (reproducible), its terms are grouped per ray
// instead of per thread-strided element, so its value agrees with wisp_rgb_loss to rounding, not bit for bit.
// W waves per workgroup, each wave a "group" of its own (group v walks rays v, v + groups, ...: which rays a partial sum covers,
// and hence the loss bits, do not depend on W).  W = 4: a quarter of the workgroups to dispatch for the same waves.
template <int W>
__global__ void __launch_bounds__(64 * W)
composite_loss_kernel(const float* __restrict__ color, const float* __restrict__ density, const float* __restrict__ deltas,
                      const int64_t* __restrict__ offsets, int64_t num_rays, int groups, Bg bg, const float* __restrict__ gt, int kind,
                      float inv_n, float* __restrict__ grad_color, float* __restrict__ grad_density, float* __restrict__ out_rgb,
                      float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * W + (threadIdx.x >> 6);
    if (v >= groups) return;
    float lacc = 0.0f;
    for (int64_t r = v; r < num_rays; r += groups) {
        const int64_t b = offsets[r], e = offsets[r + 1];
        // the ray's ground truth does not depend on anything computed below: ask for it now, not after the reductions
        const float gt0 = gt[r * 3], gt1 = gt[r * 3 + 1], gt2 = gt[r * 3 + 2];
        const bool single = e - b <= 64;
        float carry = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f;
        float dl = 0.0f, T = 0.0f, et = 0.0f, w = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;     // the single chunk's values
        for (int64_t k0 = b; k0 < e; k0 += 64) {
            const int64_t i = k0 + lane;
            const bool live = i < e;
            // every load of the chunk is issued before the scan: with the colours fetched behind it (where they are first used) a
            // ray paid one more memory round trip in its dependent chain
            dl = live ? deltas[i] : 0.0f;
            const float dn = live ? density[i] : 0.0f;
            c0 = live ? color[i * 3] : 0.0f; c1 = live ? color[i * 3 + 1] : 0.0f; c2 = live ? color[i * 3 + 2] : 0.0f;
            const float tau = live ? dn * dl : 0.0f;
            const float inc = wave_incl_scan_f(tau, lane);
            const float excl = carry + (inc - tau);
            carry += wave_last_f(inc);
            T = 0.0f; et = 0.0f; w = 0.0f;
            if (live) {
                T = expf(-excl); et = expf(-tau);
                w = T * (1.0f - et);
                sr += w * c0; sg += w * c1; sb += w * c2;
                sa += w;
            }
        }
        if (b < e) { sr = wave_sum_f(sr); sg = wave_sum_f(sg); sb = wave_sum_f(sb); sa = wave_sum_f(sa); }
        const float om = 1.0f - sa;
        const float rgb[3] = {bg.r * om + sr, bg.g * om + sg, bg.b * om + sb};
        const float gtc[3] = {gt0, gt1, gt2};
        float g[3], lsum[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = rgb[c] - gtc[c];
            float l, d;
            if (kind == 0) { const float a = fabsf(x); l = a < 1.0f ? 0.5f * x * x : a - 0.5f; d = fminf(fmaxf(x, -1.0f), 1.0f); }
            else if (kind == 1) { l = x * x; d = 2.0f * x; }
            else { l = fabsf(x); d = (x > 0.0f) ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
            lsum[c] = l;
            g[c] = d * inv_n;
        }
        lacc += (lsum[0] + lsum[1]) + lsum[2];
        if (out_rgb && lane == 0) { out_rgb[r * 3] = rgb[0]; out_rgb[r * 3 + 1] = rgb[1]; out_rgb[r * 3 + 2] = rgb[2]; }
        if (b == e) continue;
        const float gr = g[0], gg = g[1], gb = g[2];
        if (single) {
            const int64_t i = b + lane;
            const bool live = i < e;
            const float G = live ? gr * (c0 - bg.r) + gg * (c1 - bg.g) + gb * (c2 - bg.b) : 0.0f;
            const float gw = G * w;
            const float ginc = wave_incl_scan_f(gw, lane);
            const float tot = wave_last_f(ginc);
            const float suffix = tot - ginc;
            if (live) {
                grad_color[i * 3] = w * gr; grad_color[i * 3 + 1] = w * gg; grad_color[i * 3 + 2] = w * gb;
                grad_density[i] = (G * T * et - suffix) * dl;
            }
            continue;
        }
        // longer rays: as composite_bwd_kernel - the total of G w first, then the gradients with the suffix sums
        carry = 0.0f;
        float tot = 0.0f;
        for (int64_t k0 = b; k0 < e; k0 += 64) {
            const int64_t i = k0 + lane;
            const bool live = i < e;
            const float tau = live ? density[i] * deltas[i] : 0.0f;
            const float inc = wave_incl_scan_f(tau, lane);
            const float excl = carry + (inc - tau);
            carry += wave_last_f(inc);
            if (live) {
                const float ww = expf(-excl) * (1.0f - expf(-tau));
                const float G = gr * (color[i * 3] - bg.r) + gg * (color[i * 3 + 1] - bg.g) + gb * (color[i * 3 + 2] - bg.b);
                tot += G * ww;
            }
        }
        tot = wave_sum_f(tot);
        carry = 0.0f;
        float gcarry = 0.0f;
        for (int64_t k0 = b; k0 < e; k0 += 64) {
            const int64_t i = k0 + lane;
            const bool live = i < e;
            const float dd = live ? deltas[i] : 0.0f;
            const float tau = live ? density[i] * dd : 0.0f;
            const float inc = wave_incl_scan_f(tau, lane);
            const float excl = carry + (inc - tau);
            carry += wave_last_f(inc);
            float TT = 0.0f, ee = 0.0f, ww = 0.0f, G = 0.0f;
            if (live) {
                TT = expf(-excl); ee = expf(-tau); ww = TT * (1.0f - ee);
                G = gr * (color[i * 3] - bg.r) + gg * (color[i * 3 + 1] - bg.g) + gb * (color[i * 3 + 2] - bg.b);
            }
            const float gw = G * ww;
            const float ginc = wave_incl_scan_f(gw, lane);
            const float suffix = tot - (gcarry + ginc);
            gcarry += wave_last_f(ginc);
            if (live) {
                grad_color[i * 3] = ww * gr; grad_color[i * 3 + 1] = ww * gg; grad_color[i * 3 + 2] = ww * gb;
                grad_density[i] = (G * TT * ee - suffix) * dd;
            }
        }
    }
    // loss: one partial per workgroup (every lane holds the same sum); loss_sum_kernel adds them in index order.  (A last-
    // workgroup-finishes reduction inside this kernel - device-scope fence + ticket per workgroup - took the launch from 36 to
    // 238 us at 38 K rays: on this part a device-scope release / acquire writes back and invalidates the XCD's L2, 8192 times.)
    if (lane == 0) partial[v] = lacc;
}

// ---- the same pass with long rays split over the four waves of their workgroup ------------------------------------------
// composite_loss_kernel spends its launch in its longest ray: a ray of n > 64 samples walks ceil(n / 64) chunks three times, each
// round a dependent load -> scan -> exp chain (36 rounds for the 718-sample ray of a 2^18 batch, while 79 % of the rays are
// empty).  Here a workgroup still holds four consecutive rays, one per wave, and a wave whose ray has at most 64 samples (or
// more than 256 K samples) does what it does there; then the workgroup goes over its long rays one at a time, chunk c on wave c % 4,
// every chunk in registers (K per wave), every load of the ray issued at once:
//   1  load; tau, in-chunk scan, chunk total -> LDS                                                                 | barrier
//   2  carry = the chunk totals added in chunk order from 0 (the adds of `carry +=`); T, et, w; w and colour -> LDS | barrier
//   3  wave q adds sum q (r, g, b, alpha) per lane in chunk order, then over the lanes; -> LDS                      | barrier
//   4  every wave: rgb, loss terms, g (same inputs, same code: no broadcast); G of its chunks; scan of G w, totals -> LDS | barrier
//   5  every wave: total of G w per lane in chunk order; gcarry like carry; the gradients from registers
// Only workgroup barriers and LDS; every wave reaches each barrier once per long ray, and which rays are long is decided from the
// same four offset pairs by every wave, rays behind the last one count as empty.
// The results are those of composite_loss_kernel bit for bit: every sum keeps its order, and every product-sum is written out
// as that kernel's code object evaluates it (fmaf where it contracts, separate roundings where it does not - it contracts
// sr and sg but not sb, G differently in each of its three places, and the first step of the scan of G w with the product).
#define WISP_DPP_ADD(V, CTRL, RMASK)                                                                                  \
    V = V + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, V), CTRL, RMASK, 0xf, false))
// inclusive scan of a * b whose first step is fma(a, b, shr1(a * b))
static __device__ __forceinline__ float wave_incl_scan_prod_f(float a, float b) {
#pragma clang fp contract(off)
    const float p = a * b;
    float v = fmaf(a, b, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, p), 0x111, 0xf, 0xf, false)));
    WISP_DPP_ADD(v, 0x112, 0xf);
    WISP_DPP_ADD(v, 0x114, 0xf);
    WISP_DPP_ADD(v, 0x118, 0xf);
    WISP_DPP_ADD(v, 0x142, 0xa);
    WISP_DPP_ADD(v, 0x143, 0xc);
    return v;
}
#undef WISP_DPP_ADD

// rgb, d loss / d rgb and the ray's loss term from its four sums
static __device__ __forceinline__ float ray_loss_terms(float sr, float sg, float sb, float sa, const Bg& bg, float gt0, float gt1,
                                                       float gt2, int kind, float inv_n, float (&rgb)[3], float (&g)[3]) {
#pragma clang fp contract(off)
    const float om = 1.0f - sa;
    rgb[0] = fmaf(bg.r, om, sr); rgb[1] = fmaf(bg.g, om, sg); rgb[2] = fmaf(bg.b, om, sb);
    const float gtc[3] = {gt0, gt1, gt2};
    float lsum[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = rgb[c] - gtc[c];
        float l, d;
        if (kind == 0) { const float a = fabsf(x); const float h = 0.5f * x; l = a < 1.0f ? h * x : a - 0.5f; d = fminf(fmaxf(x, -1.0f), 1.0f); }
        else if (kind == 1) { l = x * x; d = 2.0f * x; }
        else { l = fabsf(x); d = (x > 0.0f) ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
        lsum[c] = l;
        g[c] = d * inv_n;
    }
    return (lsum[0] + lsum[1]) + lsum[2];
}

// one ray on one wave, as composite_loss_kernel does it: at most 64 samples out of registers, more in three passes
static __device__ __forceinline__ float composite_ray_serial(const float* __restrict__ color, const float* __restrict__ density,
                                                             const float* __restrict__ deltas, int64_t b, int64_t e, int64_t r,
                                                             int lane, const Bg& bg, const float* __restrict__ gt, int kind,
                                                             float inv_n, float* __restrict__ grad_color,
                                                             float* __restrict__ grad_density, float* __restrict__ out_rgb) {
#pragma clang fp contract(off)
    const float gt0 = gt[r * 3], gt1 = gt[r * 3 + 1], gt2 = gt[r * 3 + 2];
    const bool single = e - b <= 64;
    float carry = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f;
    float dl = 0.0f, T = 0.0f, et = 0.0f, w = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    for (int64_t k0 = b; k0 < e; k0 += 64) {
        const int64_t i = k0 + lane;
        const bool live = i < e;
        dl = live ? deltas[i] : 0.0f;
        const float dn = live ? density[i] : 0.0f;
        c0 = live ? color[i * 3] : 0.0f; c1 = live ? color[i * 3 + 1] : 0.0f; c2 = live ? color[i * 3 + 2] : 0.0f;
        const float tau = live ? dn * dl : 0.0f;
        const float inc = wave_incl_scan_f(tau, lane);
        const float excl = carry + (inc - tau);
        carry = carry + wave_last_f(inc);
        T = 0.0f; et = 0.0f; w = 0.0f;
        if (live) {
            T = expf(-excl); et = expf(-tau);
            w = (1.0f - et) * T;
            sr = fmaf(c0, w, sr); sg = fmaf(c1, w, sg);
            const float pb = c2 * w;
            sb = sb + pb;
            sa = sa + w;
        }
    }
    if (b < e) { sr = wave_sum_f(sr); sg = wave_sum_f(sg); sb = wave_sum_f(sb); sa = wave_sum_f(sa); }
    float rgb[3], g[3];
    const float term = ray_loss_terms(sr, sg, sb, sa, bg, gt0, gt1, gt2, kind, inv_n, rgb, g);
    if (out_rgb && lane == 0) { out_rgb[r * 3] = rgb[0]; out_rgb[r * 3 + 1] = rgb[1]; out_rgb[r * 3 + 2] = rgb[2]; }
    if (b == e) return term;
    const float gr = g[0], gg = g[1], gb = g[2];
    if (single) {
        const int64_t i = b + lane;
        const bool live = i < e;
        const float a0 = c0 - bg.r, a1 = c1 - bg.g, a2 = c2 - bg.b;
        const float G = live ? fmaf(a2, gb, fmaf(a0, gr, a1 * gg)) : 0.0f;
        const float ginc = wave_incl_scan_prod_f(w, G);
        const float tot = wave_last_f(ginc);
        const float suffix = tot - ginc;
        if (live) {
            grad_color[i * 3] = w * gr; grad_color[i * 3 + 1] = w * gg; grad_color[i * 3 + 2] = w * gb;
            const float tg = T * G;
            grad_density[i] = fmaf(et, tg, -suffix) * dl;
        }
        return term;
    }
    carry = 0.0f;
    float tot = 0.0f;
    for (int64_t k0 = b; k0 < e; k0 += 64) {
        const int64_t i = k0 + lane;
        const bool live = i < e;
        const float tau = live ? density[i] * deltas[i] : 0.0f;
        const float inc = wave_incl_scan_f(tau, lane);
        const float excl = carry + (inc - tau);
        carry = carry + wave_last_f(inc);
        if (live) {
            const float ww = (1.0f - expf(-tau)) * expf(-excl);
            const float p0 = gr * (color[i * 3] - bg.r), p1 = gg * (color[i * 3 + 1] - bg.g), p2 = gb * (color[i * 3 + 2] - bg.b);
            const float G = (p0 + p1) + p2;
            tot = fmaf(ww, G, tot);
        }
    }
    tot = wave_sum_f(tot);
    carry = 0.0f;
    float gcarry = 0.0f;
    for (int64_t k0 = b; k0 < e; k0 += 64) {
        const int64_t i = k0 + lane;
        const bool live = i < e;
        const float dd = live ? deltas[i] : 0.0f;
        const float tau = live ? density[i] * dd : 0.0f;
        const float inc = wave_incl_scan_f(tau, lane);
        const float excl = carry + (inc - tau);
        carry = carry + wave_last_f(inc);
        float TT = 0.0f, ee = 0.0f, ww = 0.0f, G = 0.0f;
        if (live) {
            TT = expf(-excl); ee = expf(-tau); ww = (1.0f - ee) * TT;
            const float p0 = gr * (color[i * 3] - bg.r), p2 = gb * (color[i * 3 + 2] - bg.b);
            G = fmaf(gg, color[i * 3 + 1] - bg.g, p0) + p2;
        }
        const float ginc = wave_incl_scan_prod_f(ww, G);
        const float suffix = tot - (gcarry + ginc);
        gcarry = gcarry + wave_last_f(ginc);
        if (live) {
            grad_color[i * 3] = ww * gr; grad_color[i * 3 + 1] = ww * gg; grad_color[i * 3 + 2] = ww * gb;
            const float tg = TT * G;
            grad_density[i] = fmaf(ee, tg, -suffix) * dd;
        }
    }
    return term;
}

// running sum of the chunk totals tot[0 .. nch) in chunk order; out[k] = the sum in front of chunk wv + 4 k.  Lane c fetches
// tot[c] once and the adds take their operand with v_readlane: a loop of LDS reads, each behind the add before it, cost 75 ns per
// chunk - more than everything else a long ray does here.  (Chunks behind the last add +0.0 to a sum nothing uses.)
template <int K>
static __device__ __forceinline__ void chunk_carries(const float* tot, int nch, int wv, int lane, float (&out)[K]) {
#pragma clang fp contract(off)
    const float mine = lane < nch ? tot[lane] : 0.0f;
    float run = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        out[k] = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q == wv) out[k] = run;
            run = run + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), 4 * k + q));
        }
    }
}

// per-lane accumulation over the chunks in chunk order, four chunks' LDS reads in flight:
// MODE 0  acc = fma(a, b, acc)     1  acc = acc + a * b     2  acc = acc + b
template <int MODE>
static __device__ __forceinline__ float chunk_accumulate(const float* sa, const float* sb, int nch, int lane) {
#pragma clang fp contract(off)
    float acc = 0.0f;
    for (int cb = 0; cb < nch; cb += 4) {                     // (nch <= 4 K: cb + 3 stays inside the arrays)
        float a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = MODE == 2 ? 0.0f : sa[(cb + q) * 64 + lane]; b[q] = sb[(cb + q) * 64 + lane]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (cb + q < nch) {                               // wave-uniform
                if (MODE == 0) acc = fmaf(a[q], b[q], acc);
                else if (MODE == 1) { const float p = a[q] * b[q]; acc = acc + p; }
                else acc = acc + b[q];
            }
        }
    }
    return acc;
}

template <int K>
// K chunks of a ray per wave in registers.  K = 4 (rays of up to 1 024 samples; the longest of a 2^18 batch has 718) compiles to
// 80 VGPRs, 16 KB of LDS and no scratch: six waves per SIMD, all workgroups of a 2^18 batch resident at once.  K = 8 (2 048 samples,
// 155 VGPRs, 32 KB, three waves per SIMD) was measured and is slower than the kernel this one replaces (25.9 against 18.9 us,
// profiles/long_rays_ab.txt): every long ray pays for the unrolled chunk slots it does not use.  A longer ray takes the three
// passes on its own wave.
__global__ void __launch_bounds__(256, 5)
composite_loss_split_kernel(const float* __restrict__ color, const float* __restrict__ density, const float* __restrict__ deltas,
                            const int64_t* __restrict__ offsets, int64_t num_rays, Bg bg, const float* __restrict__ gt, int kind,
                            float inv_n, float* __restrict__ grad_color, float* __restrict__ grad_density,
                            float* __restrict__ out_rgb, float* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NCH = 4 * K;                                // chunks of the longest ray of the split path
    __shared__ float s_w[NCH * 64];                           // [chunk][lane]: w
    __shared__ float s_c[3][NCH * 64];                        // [chunk][lane]: colour; behind barrier 3, s_c[0] = G of the total
    __shared__ float s_tot[NCH], s_gtot[NCH], s_sum[4];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 4;
    // the four offset pairs of the workgroup, read by every wave: the same values, the same decisions
    int64_t ob[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) ob[j] = offsets[r0 + j < num_rays ? r0 + j : num_rays];
    {
        const int64_t r = r0 + wv;
        if (r < num_rays) {                                   // (no barrier in here)
            const int64_t len = ob[wv + 1 < 5 ? wv + 1 : 4] - ob[wv];
            const int64_t b = wv == 0 ? ob[0] : wv == 1 ? ob[1] : wv == 2 ? ob[2] : ob[3];
            if (len <= 64 || len > 64 * NCH) {
                float lacc = 0.0f;
                lacc = lacc + composite_ray_serial(color, density, deltas, b, b + len, r, lane, bg, gt, kind, inv_n, grad_color,
                                                   grad_density, out_rgb);
                if (lane == 0) partial[r] = lacc;
            }
        }
    }
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const int64_t b = j == 0 ? ob[0] : j == 1 ? ob[1] : j == 2 ? ob[2] : ob[3];
        const int64_t e = j == 0 ? ob[1] : j == 1 ? ob[2] : j == 2 ? ob[3] : ob[4];
        const int64_t len = e - b;
        if (len <= 64 || len > 64 * NCH) continue;            // workgroup-uniform
        const int64_t r = r0 + j;                             // < num_rays: a ray behind the last one has length 0
        const int nch = (int)((len + 63) >> 6);
        const float gt0 = gt[r * 3], gt1 = gt[r * 3 + 1], gt2 = gt[r * 3 + 2];
        float dl[K], tau[K], inc[K], c0[K], c1[K], c2[K];
        // 1: every load of the wave's chunks first, then the scans
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t i = b + (int64_t)(wv + 4 * k) * 64 + lane;
            const bool live = i < e;
            dl[k] = live ? deltas[i] : 0.0f;
            tau[k] = live ? density[i] : 0.0f;
            c0[k] = live ? color[i * 3] : 0.0f; c1[k] = live ? color[i * 3 + 1] : 0.0f; c2[k] = live ? color[i * 3 + 2] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = wv + 4 * k;
            const bool live = b + (int64_t)c * 64 + lane < e;
            tau[k] = live ? tau[k] * dl[k] : 0.0f;
            inc[k] = wave_incl_scan_f(tau[k], lane);
            if (c < nch && lane == 0) s_tot[c] = wave_last_f(inc[k]);
        }
        __syncthreads();
        // 2
        float T[K], et[K], w[K];
        {
            float carry[K];
            chunk_carries<K>(s_tot, nch, wv, lane, carry);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int c = wv + 4 * k;
                const bool live = b + (int64_t)c * 64 + lane < e;
                const float excl = carry[k] + (inc[k] - tau[k]);
                T[k] = 0.0f; et[k] = 0.0f; w[k] = 0.0f;
                if (live) {
                    T[k] = expf(-excl); et[k] = expf(-tau[k]);
                    w[k] = (1.0f - et[k]) * T[k];
                }
                if (c < nch) {
                    s_w[c * 64 + lane] = w[k];
                    s_c[0][c * 64 + lane] = c0[k]; s_c[1][c * 64 + lane] = c1[k]; s_c[2][c * 64 + lane] = c2[k];
                }
            }
        }
        __syncthreads();
        // 3: wave 0 red, 1 green, 2 blue (not contracted), 3 alpha
        {
            float acc;
            if (wv == 0)      acc = chunk_accumulate<0>(s_c[0], s_w, nch, lane);
            else if (wv == 1) acc = chunk_accumulate<0>(s_c[1], s_w, nch, lane);
            else if (wv == 2) acc = chunk_accumulate<1>(s_c[2], s_w, nch, lane);
            else              acc = chunk_accumulate<2>(s_w, s_w, nch, lane);
            acc = wave_sum_f(acc);
            if (lane == 0) s_sum[wv] = acc;
        }
        __syncthreads();
        // 4
        float rgb[3], g[3];
        const float term = ray_loss_terms(s_sum[0], s_sum[1], s_sum[2], s_sum[3], bg, gt0, gt1, gt2, kind, inv_n, rgb, g);
        if (wv == 0 && lane == 0) {
            if (out_rgb) { out_rgb[r * 3] = rgb[0]; out_rgb[r * 3 + 1] = rgb[1]; out_rgb[r * 3 + 2] = rgb[2]; }
            float lacc = 0.0f;
            lacc = lacc + term;
            partial[r] = lacc;
        }
        const float gr = g[0], gg = g[1], gb = g[2];
        float G[K], ginc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = wv + 4 * k;
            const bool live = b + (int64_t)c * 64 + lane < e;
            const int at = (c < nch ? c : 0) * 64 + lane;                        // the wave's own colours, back from LDS
            const float a0 = s_c[0][at] - bg.r, a1 = s_c[1][at] - bg.g, a2 = s_c[2][at] - bg.b;
            const float p0 = gr * a0, p1 = gg * a1, p2 = gb * a2;
            const float Gt = live ? (p0 + p1) + p2 : 0.0f;                       // G as the pass of the total rounds it
            G[k] = live ? fmaf(gg, a1, p0) + p2 : 0.0f;                          // G as the pass of the gradients rounds it
            ginc[k] = wave_incl_scan_prod_f(w[k], G[k]);
            if (c < nch) {
                s_c[0][c * 64 + lane] = Gt;
                if (lane == 0) s_gtot[c] = wave_last_f(ginc[k]);
            }
        }
        __syncthreads();
        // 5
        const float tot = wave_sum_f(chunk_accumulate<0>(s_w, s_c[0], nch, lane));
        float gcarry[K];
        chunk_carries<K>(s_gtot, nch, wv, lane, gcarry);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t i = b + (int64_t)(wv + 4 * k) * 64 + lane;
            if (i < e) {
                const float suffix = tot - (gcarry[k] + ginc[k]);
                grad_color[i * 3] = w[k] * gr; grad_color[i * 3 + 1] = w[k] * gg; grad_color[i * 3 + 2] = w[k] * gb;
                const float tg = T[k] * G[k];
                grad_density[i] = fmaf(et[k], tg, -suffix) * dl[k];
            }
        }
        // (the next long ray writes s_tot in front of its first barrier, s_w / s_c / s_sum / s_gtot behind it: nothing this ray still reads)
    }
}

// the compositing launch only: workspace[0 .. *num_partials) holds the loss partials, loss = (their sum in index order) * *inv_n is
// the caller's to form - wisp_loss_sum, or the side workgroup of wisp_hashgrid_interpolate_bwd_adamw_tail
extern "C" int wisp_composite_loss_partials(const float* color, const float* density, const float* deltas, const int64_t* ray_offsets,
                                            int64_t num_rays, int64_t num_samples, const float* bg, const float* gt, int kind,
                                            float* grad_color, float* grad_density, float* out_rgb, float* workspace,
                                            int64_t workspace_floats, int* num_partials, float* inv_n_out, wisp_stream_t stream) {
    WISP_REQUIRE(num_rays > 0 && num_samples >= 0 && bg && gt && ray_offsets && workspace && workspace_floats >= 1 && num_partials && inv_n_out, "bad arguments");
    WISP_REQUIRE(kind >= 0 && kind <= 2, "kind: 0 huber, 1 l2, 2 l1");
    WISP_REQUIRE(num_samples == 0 || (color && density && deltas && grad_color && grad_density), "null pointer");
    const Bg b{bg[0], bg[1], bg[2]};
    // one ray per wave when the workspace has a partial-sum cell for every ray (rays differ a lot in length: handing a wave
    // several of them in a fixed order leaves the launch waiting for the unluckiest wave), else a grid-stride walk
    const int groups = (int)min64(num_rays, min64(workspace_floats, (int64_t)1 << 22));
    const float inv_n = 1.0f / (float)(num_rays * 3);
    static const int waves = [] { const char* e = getenv("WISP_COMPOSITE_WAVES"); const int w = e ? atoi(e) : 4; return (w == 1 || w == 2) ? w : 4; }();
    // WISP_COMPOSITE_SPLIT (read on every call: a test flips it between two calls): 0 = composite_loss_kernel for every ray
    const char* se = getenv("WISP_COMPOSITE_SPLIT");
    const bool split = waves == 4 && groups == num_rays && !(se && atoi(se) == 0);
    if (split)
        hipLaunchKernelGGL(composite_loss_split_kernel<4>, dim3((groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, color, density, deltas,
                           ray_offsets, num_rays, b, gt, kind, inv_n, grad_color, grad_density, out_rgb, workspace);
    else if (waves == 1)
        hipLaunchKernelGGL(composite_loss_kernel<1>, dim3(groups), dim3(64), 0, (hipStream_t)stream, color, density, deltas, ray_offsets,
                           num_rays, groups, b, gt, kind, inv_n, grad_color, grad_density, out_rgb, workspace);
    else if (waves == 2)
        hipLaunchKernelGGL(composite_loss_kernel<2>, dim3((groups + 1) / 2), dim3(128), 0, (hipStream_t)stream, color, density, deltas, ray_offsets,
                           num_rays, groups, b, gt, kind, inv_n, grad_color, grad_density, out_rgb, workspace);
    else
        hipLaunchKernelGGL(composite_loss_kernel<4>, dim3((groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, color, density, deltas, ray_offsets,
                           num_rays, groups, b, gt, kind, inv_n, grad_color, grad_density, out_rgb, workspace);
    *num_partials = groups;
    *inv_n_out = inv_n;
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_composite_loss(const float* color, const float* density, const float* deltas, const int64_t* ray_offsets,
                                   int64_t num_rays, int64_t num_samples, const float* bg, const float* gt, int kind,
                                   float* grad_color, float* grad_density, float* out_rgb, float* loss, float* workspace,
                                   int64_t workspace_floats, wisp_stream_t stream) {
    WISP_REQUIRE(loss, "bad arguments");
    int groups = 0;
    float inv_n = 0.0f;
    if (int rc = wisp_composite_loss_partials(color, density, deltas, ray_offsets, num_rays, num_samples, bg, gt, kind, grad_color, grad_density,
                                              out_rgb, workspace, workspace_floats, &groups, &inv_n, stream))
        return rc;
    return wisp_loss_sum(workspace, groups, inv_n, loss, stream);
}
