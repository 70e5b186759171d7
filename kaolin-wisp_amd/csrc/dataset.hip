// Multiview image bank -> training rays for gfx950.
//
// Replaces the resident per-ray tensors of NeRFSyntheticDataset (wisp/datasets/formats/nerf_standard_dataset.py:405-441: rays of
// every pixel of every view generated once and kept, colours blended once and kept - 37 bytes per pixel) and the per-step
// index_select launches of SampleRays over them (wisp/datasets/transforms/ray_sampler.py:25-35).  The bank stays what the files
// held - 8-bit RGBA, 4 bytes per pixel - and a ray is a pure function of (camera, pixel): one thread turns one pixel index into
// origin, direction, blended colour and mask.  Nothing per ray is read, 37 bytes per ray are written.
#include "wisp_common.h"
#include "raygen_dev.h"

struct BankGeom {
    int64_t view_stride;      // texels per view of the stored (full-size) bank: H * W
    int row_stride;           // texels per stored row: W
    int w, h;                 // mip-sized image: W >> mip, H >> mip
    int mip;
    int has_alpha;
    float bg[3];
};

// One texel -> four floats, each `float(u8) / 255.0f` (a division, as `img.float() / 255.0` of load_rgb, ops/image/io.py:83).
static __device__ __forceinline__ void texel_to_float(uint32_t t, float* __restrict__ c) {
    c[0] = (float)(t & 0xffu) / 255.0f;
    c[1] = (float)((t >> 8) & 0xffu) / 255.0f;
    c[2] = (float)((t >> 16) & 0xffu) / 255.0f;
    c[3] = (float)(t >> 24) / 255.0f;
}

// PER_RAY_VIEW = false: every ray belongs to view `view_index`, whose camera arrives by value.
// PER_RAY_VIEW = true : ray i belongs to view[i]; the lane reads that view's 64-byte record (R[9], t[3], 4 floats of padding)
//                       from `cameras` - a few hundred records, L2 resident.
template <bool PER_RAY_VIEW>
__global__ void __launch_bounds__(256)
multiview_sample_kernel(const uint32_t* __restrict__ bank, const float4* __restrict__ cameras, const int64_t* __restrict__ pix,
                        const int64_t* __restrict__ view, int64_t view_index, int64_t n, RayCam cam, BankGeom g,
                        float* __restrict__ origins, float* __restrict__ dirs, float* __restrict__ rgb,
                        uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t p = pix[i];
    if (p < 0) p += (int64_t)g.w * g.h;                                  // torch indexing semantics, as wisp_gather_rows
    const uint32_t pu = (uint32_t)p;                                     // h * w fits 31 bits (both are ints): a 32-bit divide
    const int row = (int)(pu / (uint32_t)g.w), col = (int)(pu - (uint32_t)row * (uint32_t)g.w);
    const int64_t v = PER_RAY_VIEW ? view[i] : view_index;
    if (origins || dirs) {
        if (PER_RAY_VIEW) {
            const float4 a = cameras[v * 4], b = cameras[v * 4 + 1], c = cameras[v * 4 + 2];
            cam.r[0] = a.x; cam.r[1] = a.y; cam.r[2] = a.z; cam.r[3] = a.w;
            cam.r[4] = b.x; cam.r[5] = b.y; cam.r[6] = b.z; cam.r[7] = b.w;
            cam.r[8] = c.x; cam.t[0] = c.y; cam.t[1] = c.z; cam.t[2] = c.w;
        }
        // pixel centre as generate_centered_pixel_coords forms it (raygen.py:22-30): index * 1.0 + 0.5
        float ow[3], dn[3];
        wisp_camera_ray<false>((float)col * 1.0f + 0.5f, (float)row * 1.0f + 0.5f, cam, ow, dn);
        if (origins) { origins[i * 3] = ow[0]; origins[i * 3 + 1] = ow[1]; origins[i * 3 + 2] = ow[2]; }
        if (dirs) { dirs[i * 3] = dn[0]; dirs[i * 3 + 1] = dn[1]; dirs[i * 3 + 2] = dn[2]; }
    }
    if (!rgb && !mask) return;
    // the 2^mip x 2^mip block of stored texels behind this pixel: each converted first, then summed in row-major order, then
    // scaled by 1 / 4^mip (a box mean; mip = 0: the texel itself, times 1)
    const int side = 1 << g.mip;
    const uint32_t* __restrict__ src = bank + v * g.view_stride + (int64_t)(row << g.mip) * g.row_stride + (col << g.mip);
    float acc[4];
    texel_to_float(src[0], acc);
    for (int dy = 0; dy < side; ++dy)
        for (int dx = (dy == 0 ? 1 : 0); dx < side; ++dx) {
            float c[4];
            texel_to_float(src[(int64_t)dy * g.row_stride + dx], c);
            acc[0] = acc[0] + c[0]; acc[1] = acc[1] + c[1]; acc[2] = acc[2] + c[2]; acc[3] = acc[3] + c[3];
        }
    if (g.mip > 0) {
        const float inv = 1.0f / (float)(1 << (2 * g.mip));
        acc[0] = acc[0] * inv; acc[1] = acc[1] * inv; acc[2] = acc[2] * inv; acc[3] = acc[3] * inv;
    }
    bool m = true;
    if (g.has_alpha) {                                                   // nerf_standard_dataset.py:437-439
        const float a = acc[3], om = 1.0f - a;
        m = a > 0.5f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float fg = acc[c] * a, back = om * g.bg[c];
            acc[c] = fminf(fmaxf(fg + back, 0.0f), 1.0f);
        }
    }
    if (rgb) { rgb[i * 3] = acc[0]; rgb[i * 3 + 1] = acc[1]; rgb[i * 3 + 2] = acc[2]; }
    if (mask) mask[i] = m ? 1 : 0;
}

extern "C" int wisp_multiview_sample(const uint8_t* images, const float* cameras, const float* camera_host, int64_t num_views,
                                     int height, int width, int mip, int has_alpha, const int64_t* pix, const int64_t* view,
                                     int64_t view_index, int64_t num_rays, float x0, float y0, float tan_half_fov_x,
                                     float tan_half_fov_y, const float* bg, float* origins, float* dirs, float* rgb,
                                     uint8_t* mask, wisp_stream_t stream) {
    WISP_REQUIRE(num_rays >= 0 && num_views >= 0, "negative count");
    WISP_REQUIRE(mip >= 0 && mip <= 5, "mip must be in 0..5");
    if (num_rays == 0) return WISP_OK;
    WISP_REQUIRE(num_views >= 1 && height >= 1 && width >= 1, "empty image bank");
    WISP_REQUIRE(height % (1 << mip) == 0 && width % (1 << mip) == 0, "image size must be a multiple of 2^mip");
    WISP_REQUIRE((int64_t)height * width < ((int64_t)1 << 31), "image too large");
    WISP_REQUIRE(pix, "null pixel index");
    WISP_REQUIRE(images || (!rgb && !mask), "colours / masks need the image bank");
    WISP_REQUIRE(bg || !rgb || !has_alpha, "null bg");
    WISP_REQUIRE(((uintptr_t)images & 3) == 0, "image bank must be 4-byte aligned");
    const bool want_rays = origins || dirs;
    RayCam cam{};
    cam.x0 = x0; cam.y0 = y0; cam.width = (float)(width >> mip); cam.height = (float)(height >> mip);
    cam.sx = tan_half_fov_x; cam.sy = tan_half_fov_y;
    BankGeom g{};
    g.view_stride = (int64_t)height * width; g.row_stride = width; g.w = width >> mip; g.h = height >> mip; g.mip = mip;
    g.has_alpha = has_alpha ? 1 : 0;
    for (int k = 0; k < 3; ++k) g.bg[k] = bg ? bg[k] : 0.0f;              // host array
    const dim3 grid((unsigned)ceil_div64(num_rays, 256));
    const uint32_t* bank = reinterpret_cast<const uint32_t*>(images);
    if (view) {
        WISP_REQUIRE(!want_rays || cameras, "per-ray views need the device camera table");
        WISP_REQUIRE(((uintptr_t)cameras & 15) == 0, "camera table must be 16-byte aligned");
        hipLaunchKernelGGL(multiview_sample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, bank,
                           reinterpret_cast<const float4*>(cameras), pix, view, (int64_t)0, num_rays, cam, g, origins, dirs, rgb, mask);
    } else {
        WISP_REQUIRE(view_index >= 0 && view_index < num_views, "view index out of range");
        WISP_REQUIRE(!want_rays || camera_host, "one-view mode needs the view's camera record (host)");
        if (camera_host) {
            for (int k = 0; k < 9; ++k) cam.r[k] = camera_host[k];
            for (int k = 0; k < 3; ++k) cam.t[k] = camera_host[9 + k];
        }
        hipLaunchKernelGGL(multiview_sample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, bank,
                           static_cast<const float4*>(nullptr), pix, view, view_index, num_rays, cam, g, origins, dirs, rgb, mask);
    }
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
