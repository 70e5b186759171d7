// The ray of one pixel of one camera, shared by wisp_generate_rays (render.hip) and wisp_multiview_sample (dataset.hip):
// both must produce the same bits for the same (camera, pixel), so the arithmetic is written once.
// generate_pinhole_rays / generate_ortho_rays (wisp/ops/raygen/raygen.py:40-119): pixel coordinates -> principal-point shift ->
// NDC -> camera-space ray -> world space (inverse of the view transform: R^T (p - t)) -> normalised direction.  Every step is a
// separately rounded fp32 operation, in the reference's order.
#pragma once
#include "wisp_common.h"

struct RayCam {
    float x0, y0, width, height;      // principal point offset (pixels from the image centre), image size
    float sx, sy;                     // pinhole: tan(fov_x / 2), tan(fov_y / 2); ortho: fov_distance * aspect, fov_distance
    float r[9];                       // view rotation R (row major), world -> camera
    float t[3];                       // view translation
};

template <bool ORTHO>
static __device__ __forceinline__ void wisp_camera_ray(float px, float py, const RayCam& cam, float* __restrict__ ow,
                                                       float* __restrict__ dn) {
#pragma clang fp contract(off)
    if (!ORTHO) { px = px - cam.x0; py = py + cam.y0; }                  // raygen.py:66-67
    px = 2.0f * (px / cam.width) - 1.0f;                                  // _to_ndc_coords, :34-37
    py = 2.0f * (py / cam.height) - 1.0f;
    float o[3], d[3];
    if (ORTHO) {                                                          // :100-107
        o[0] = px * cam.sx; o[1] = -(py * cam.sy); o[2] = 0.0f;
        d[0] = 0.0f; d[1] = 0.0f; d[2] = -1.0f;
    } else {                                                              // :72-77
        o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
        d[0] = px * cam.sx; d[1] = -py * cam.sy; d[2] = -1.0f;
    }
    // inv_transform_rays: origin' = R^T (o - t), dir' = R^T d  (sums accumulated left to right)
    const float q[3] = {o[0] - cam.t[0], o[1] - cam.t[1], o[2] - cam.t[2]};
    float dw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ow[c] = (cam.r[0 + c] * q[0] + cam.r[3 + c] * q[1]) + cam.r[6 + c] * q[2];
        dw[c] = (cam.r[0 + c] * d[0] + cam.r[3 + c] * d[1]) + cam.r[6 + c] * d[2];
    }
    const float nrm = sqrtf((dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2]);        // torch.linalg.norm
#pragma unroll
    for (int c = 0; c < 3; ++c) dn[c] = dw[c] / nrm;
}
