// Surface colour of a textured mesh at the closest point of a chosen triangle (replaces the torch chain behind
// wisp/ops/mesh/closest_tex.py:43-64: closest_point_on_triangle, closest_point.py:17-107, with its [N,3,3] fp64 temporaries;
// barycentric_coordinates.py:31-45; the UV gather + weighted sum; sample_tex.py:27-56 with one grid_sample and two host
// read-backs per material).  The nearest triangle comes from wisp_mesh_to_sdf_triangle (mesh_sdf.hip); everything behind it is
// one launch, one thread per point.  Every step is written as separately rounded IEEE operations (the compiler's own contraction
// is off), so tests/mesh_tex_ref.py can restate it operation for operation; include/wisp_hip.h spells the arithmetic out.
#include "wisp_common.h"
#include "grid_sample_dev.h"

namespace {

constexpr int MT_BLOCK = 256;

struct MtBank {
    const float* texels;
    int64_t num_texels;
    const wisp_tex_material* mats;
    int num_mats;
};

__host__ __device__ __forceinline__ double mt_dot(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    return (ax * bx + ay * by) + az * bz;
}

// sample_tex.py:41-56 for one point: Kd of a material without a map, otherwise the bilinear lookup of its map under reflection
// padding; zero for no material / no record / a record that does not fit the bank.
__host__ __device__ __forceinline__ void mt_colour(const MtBank& bank, float u, float v, int64_t material, float& r, float& g, float& b) {
#pragma clang fp contract(off)
    r = g = b = 0.0f;
    if (material < 0 || material >= (int64_t)bank.num_mats) return;
    const wisp_tex_material m = bank.mats[material];
    if (!m.has_map) {
        r = m.kd[0];
        g = m.kd[1];
        b = m.kd[2];
        return;
    }
    if (m.height < 1 || m.width < 1 || m.offset < 0 || m.offset + (int64_t)m.height * m.width > bank.num_texels) return;
    const float gx = u * 2.0f - 1.0f;
    const float gy = -(v * 2.0f - 1.0f);                      // images are stored top row first
    const float ix = wisp_reflect_source_index(gx, m.width), iy = wisp_reflect_source_index(gy, m.height);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
    const float w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
    const bool vx1 = x1 < m.width, vy1 = y1 < m.height;       // grid_sample drops out-of-bounds corners (their weight is 0 here)
    const float* t = bank.texels + m.offset * 3;
    const float* p00 = t + ((int64_t)y0 * m.width + x0) * 3;
    const float* p01 = p00 + 3;
    const float* p10 = p00 + (int64_t)m.width * 3;
    const float* p11 = p10 + 3;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float acc = p00[k] * w00;
        if (vx1) acc = acc + p01[k] * w01;
        if (vy1) acc = acc + p10[k] * w10;
        if (vx1 && vy1) acc = acc + p11[k] * w11;
        c[k] = acc;
    }
    r = c[0];
    g = c[1];
    b = c[2];
}

// Everything wisp_mesh_closest_tex does for point i, given its triangle t (host-callable: a CPU program can run it).
__host__ __device__ __forceinline__ void mt_closest_point(int64_t i, int64_t t, const double* __restrict__ pts,
                                                          const double* __restrict__ mesh, int64_t f, const float* __restrict__ texv,
                                                          int64_t tv, const int64_t* __restrict__ texf, const MtBank& bank,
                                                          double* __restrict__ hit, float* __restrict__ rgb) {
#pragma clang fp contract(off)
    const bool have = t >= 0 && t < f;
    const double* T = mesh + (have ? t : 0) * 9;              // no triangle: the hit is taken on triangle 0 (closest_point)
    const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    const double ax = T[0], ay = T[1], az = T[2], bx = T[3], by = T[4], bz = T[5], cx = T[6], cy = T[7], cz = T[8];
    const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;

    // 1. closest point: Voronoi region from six dot products, vertex regions first, then edges, then the face
    const double d1 = mt_dot(abx, aby, abz, px - ax, py - ay, pz - az), d2 = mt_dot(acx, acy, acz, px - ax, py - ay, pz - az);
    const double d3 = mt_dot(abx, aby, abz, px - bx, py - by, pz - bz), d4 = mt_dot(acx, acy, acz, px - bx, py - by, pz - bz);
    const double d5 = mt_dot(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = mt_dot(acx, acy, acz, px - cx, py - cy, pz - cz);
    const double va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
    double hx, hy, hz;
    if (d1 <= 0.0 && d2 <= 0.0) {
        hx = ax; hy = ay; hz = az;
    } else if (d3 >= 0.0 && d4 <= d3) {
        hx = bx; hy = by; hz = bz;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double w = d1 / (d1 - d3);
        hx = ax + w * abx; hy = ay + w * aby; hz = az + w * abz;
    } else if (d6 >= 0.0 && d5 <= d6) {
        hx = cx; hy = cy; hz = cz;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
        hx = ax + w * acx; hy = ay + w * acy; hz = az + w * acz;
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        hx = bx + w * (cx - bx); hy = by + w * (cy - by); hz = bz + w * (cz - bz);
    } else {
        const double inv = 1.0 / ((va + vb) + vc);
        const double wb = vb * inv, wc = vc * inv;
        hx = (ax + abx * wb) + acx * wc; hy = (ay + aby * wb) + acy * wc; hz = (az + abz * wb) + acz * wc;
    }
    hit[3 * i] = hx;
    hit[3 * i + 1] = hy;
    hit[3 * i + 2] = hz;

    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (have) {
        const int64_t material = texf[4 * t + 3];
        if (material >= 0 && material < (int64_t)bank.num_mats) {
            float u = 0.0f, v = 0.0f;
            bool uv_ok = true;
            if (bank.mats[material].has_map) {
                // 2. barycentric coordinates of the hit: L1, L2 in fp64, clipped, rounded to fp32; L0 from them in fp32
                const double rx = hx - ax, ry = hy - ay, rz = hz - az;
                const double d00 = mt_dot(abx, aby, abz, abx, aby, abz), d01 = mt_dot(abx, aby, abz, acx, acy, acz);
                const double d11 = mt_dot(acx, acy, acz, acx, acy, acz);
                const double d20 = mt_dot(rx, ry, rz, abx, aby, abz), d21 = mt_dot(rx, ry, rz, acx, acy, acz);
                const double denom = d00 * d11 - d01 * d01;
                const float l1 = (float)fmin(fmax((d11 * d20 - d01 * d21) / denom, 0.0), 1.0);
                const float l2 = (float)fmin(fmax((d00 * d21 - d01 * d20) / denom, 0.0), 1.0);
                const float l0 = fminf(fmaxf(1.0f - (l1 + l2), 0.0f), 1.0f);
                // 3. UV
                const int64_t k0 = texf[4 * t], k1 = texf[4 * t + 1], k2 = texf[4 * t + 2];
                uv_ok = k0 >= 0 && k0 < tv && k1 >= 0 && k1 < tv && k2 >= 0 && k2 < tv;
                if (uv_ok) {
                    u = (texv[2 * k0] * l0 + texv[2 * k1] * l1) + texv[2 * k2] * l2;
                    v = (texv[2 * k0 + 1] * l0 + texv[2 * k1 + 1] * l1) + texv[2 * k2 + 1] * l2;
                }
            }
            // 4. colour
            if (uv_ok) mt_colour(bank, u, v, material, r, g, b);
        }
    }
    rgb[3 * i] = r;
    rgb[3 * i + 1] = g;
    rgb[3 * i + 2] = b;
}

template <bool TIDX_I64>
__global__ __launch_bounds__(MT_BLOCK) void mesh_tex_closest_kernel(const double* __restrict__ pts, int64_t n,
                                                                    const double* __restrict__ mesh, int64_t f,
                                                                    const void* __restrict__ tidx, const float* __restrict__ texv,
                                                                    int64_t tv, const int64_t* __restrict__ texf, MtBank bank,
                                                                    double* __restrict__ hit, float* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= n) return;
    int64_t t;
    if (TIDX_I64) {
        t = ((const int64_t*)tidx)[i];
    } else {
        const double td = ((const double*)tidx)[i];
        t = (td >= 0.0 && td < 9.0e15) ? (int64_t)td : -1;
    }
    mt_closest_point(i, t, pts, mesh, f, texv, tv, texf, bank, hit, rgb);
}

__global__ __launch_bounds__(MT_BLOCK) void mesh_tex_sample_kernel(const float* __restrict__ uv, const int64_t* __restrict__ material,
                                                                   int64_t n, MtBank bank, float* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= n) return;
    float r, g, b;
    mt_colour(bank, uv[2 * i], uv[2 * i + 1], material[i], r, g, b);
    rgb[3 * i] = r;
    rgb[3 * i + 1] = g;
    rgb[3 * i + 2] = b;
}

int check_bank(const char* fn, const float* texels, int64_t num_texels, const wisp_tex_material* materials, int num_materials) {
    if (num_texels < 0 || num_materials < 0) return wisp_fail(WISP_ERR_INVALID, fn, "negative bank size");
    if ((num_texels > 0 && !texels) || (num_materials > 0 && !materials)) return wisp_fail(WISP_ERR_INVALID, fn, "null bank pointer");
    return WISP_OK;
}

}  // namespace

extern "C" int wisp_mesh_closest_tex(const double* points, int64_t n, const double* mesh, int64_t f, const void* tidx,
                                     int tidx_is_i64, const float* texv, int64_t tv, const int64_t* texf, const float* texels,
                                     int64_t num_texels, const wisp_tex_material* materials, int num_materials, double* hit,
                                     float* rgb, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0 && f >= 1 && tv >= 0, "bad sizes");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(n <= (int64_t)0x7fffffff * MT_BLOCK, "too many points for one launch");
    WISP_REQUIRE(points && mesh && tidx && texf && hit && rgb, "null pointer");
    WISP_REQUIRE(tv == 0 || texv, "null texv");
    if (int rc = check_bank(__func__, texels, num_texels, materials, num_materials)) return rc;
    const MtBank bank{texels, num_texels, materials, num_materials};
    const unsigned blocks = (unsigned)ceil_div64(n, MT_BLOCK);
    if (tidx_is_i64)
        mesh_tex_closest_kernel<true><<<blocks, MT_BLOCK, 0, (hipStream_t)stream>>>(points, n, mesh, f, tidx, texv, tv, texf, bank, hit, rgb);
    else
        mesh_tex_closest_kernel<false><<<blocks, MT_BLOCK, 0, (hipStream_t)stream>>>(points, n, mesh, f, tidx, texv, tv, texf, bank, hit, rgb);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

extern "C" int wisp_mesh_sample_tex(const float* uv, const int64_t* material, int64_t n, const float* texels, int64_t num_texels,
                                    const wisp_tex_material* materials, int num_materials, float* rgb, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 0, "bad sizes");
    if (n == 0) return WISP_OK;
    WISP_REQUIRE(n <= (int64_t)0x7fffffff * MT_BLOCK, "too many points for one launch");
    WISP_REQUIRE(uv && material && rgb, "null pointer");
    if (int rc = check_bank(__func__, texels, num_texels, materials, num_materials)) return rc;
    const MtBank bank{texels, num_texels, materials, num_materials};
    mesh_tex_sample_kernel<<<(unsigned)ceil_div64(n, MT_BLOCK), MT_BLOCK, 0, (hipStream_t)stream>>>(uv, material, n, bank, rgb);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}
