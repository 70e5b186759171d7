// Brute-force mesh -> signed distance (replaces wisp._C.external.mesh_to_sdf_cuda / mesh_to_sdf_triangle_cuda:
// wisp/csrc/external/mesh_to_sdf.cpp:23-43, kernels wisp/csrc/external/mesh2sdf_kernel.cu:334-583 (distance + stabbing tests),
// :585-840 (+ nearest triangle), :844-970 (split aggregation), host code :1230-1330).
//
// Same rule as the reference (DESIGN.md section 7 lists every float rounding it keeps), different organisation:
//   * mesh_sdf_prep_kernel writes ONE record per triangle with everything that does not depend on the point (edges, normal,
//     edge x normal, the float-rounded reciprocals, the 13 stabbing directions' pvec = d x e2, 1/det and skip bits).  The
//     reference recomputes all of it for every (point, triangle) pair.
//   * mesh_sdf_main_kernel is a 2-D grid: x tiles the points (MS_PTS per thread, so every record read serves several pairs),
//     y splits the triangle list into ranges.  Every lane of a wave reads the same record at the same time (wave-uniform
//     scalar loads, or an LDS-staged chunk read as a broadcast with WISP_MESH_SDF_STAGE=lds; DESIGN.md section 4 has the A/B).  The inner
//     loop has no branches: the 13 tests fold into a 26-bit mask (bit d = hit at t >= 0, bit 13 + d = hit at t < 0).
//   * Ranges combine order-free: atomicOr of the mask, atomicMin of the float bits of distsq (non-negative floats order like
//     their bits) or, with the triangle index, of (bits << 32 | index).  The result is bitwise the same for every split.
#include <utility>

#include "wisp_common.h"

namespace {

constexpr int MS_BLOCK = 256;
constexpr int MS_PTS = 2;                       // points per thread
constexpr int MS_TILE = MS_BLOCK * MS_PTS;      // points per workgroup
constexpr int MS_REC = 88;                      // doubles per triangle record (87 used)
constexpr int MS_CHUNK = 16;                    // triangles per LDS round (WISP_MESH_SDF_STAGE=lds)
constexpr int64_t MS_MAX_PAIRS = int64_t(1) << 34;   // pairs per launch: no multi-second kernel on a shared GPU

// record layout (doubles)
constexpr int R_A = 0, R_B = 3, R_C = 6, R_E10 = 9, R_E21 = 12, R_E02 = 15, R_N = 18, R_CN10 = 21, R_CN21 = 24, R_CN02 = 27,
              R_R10 = 30, R_R21 = 31, R_R02 = 32, R_RN = 33, R_INVDET = 34, R_PVEC = 47, R_FLAGS = 86;
constexpr uint32_t FLAG_DEGENERATE = 1u << 13;   // flags: bits 0..12 = direction d is tested (|det_d| >= 1e-8)

// The 13 stabbing directions (mesh2sdf_kernel.cu:368-380): float literals promoted to double.
#define MS_C2 ((double)0.707106781f)
#define MS_C3 ((double)0.577350269f)
__device__ __forceinline__ void ms_dir(int d, double& x, double& y, double& z) {
    const double c2 = MS_C2, c3 = MS_C3;
    switch (d) {
        case 0: x = 1; y = 0; z = 0; break;
        case 1: x = 0; y = 1; z = 0; break;
        case 2: x = 0; y = 0; z = 1; break;
        case 3: x = 0; y = c2; z = c2; break;
        case 4: x = c2; y = 0; z = c2; break;
        case 5: x = c2; y = c2; z = 0; break;
        case 6: x = 0; y = c2; z = -c2; break;
        case 7: x = c2; y = 0; z = -c2; break;
        case 8: x = c2; y = -c2; z = 0; break;
        case 9: x = c3; y = c3; z = c3; break;
        case 10: x = -c3; y = c3; z = c3; break;
        case 11: x = c3; y = -c3; z = c3; break;
        default: x = c3; y = c3; z = -c3; break;
    }
}

// d . q with the zero components of d left out (d is a compile-time constant in the unrolled loop).
template <int D>
__device__ __forceinline__ double ms_dir_dot(double qx, double qy, double qz) {
    const double c2 = MS_C2, c3 = MS_C3;
    if constexpr (D == 0) return qx;
    else if constexpr (D == 1) return qy;
    else if constexpr (D == 2) return qz;
    else if constexpr (D == 3) return c2 * qy + c2 * qz;
    else if constexpr (D == 4) return c2 * qx + c2 * qz;
    else if constexpr (D == 5) return c2 * qx + c2 * qy;
    else if constexpr (D == 6) return c2 * qy - c2 * qz;
    else if constexpr (D == 7) return c2 * qx - c2 * qz;
    else if constexpr (D == 8) return c2 * qx - c2 * qy;
    else if constexpr (D == 9) return c3 * qx + c3 * qy + c3 * qz;
    else if constexpr (D == 10) return -c3 * qx + c3 * qy + c3 * qz;
    else if constexpr (D == 11) return c3 * qx - c3 * qy + c3 * qz;
    else return c3 * qx + c3 * qy - c3 * qz;
}

// __frcp_rn(float(x)): the reciprocal correctly rounded to float.  Dividing in double and rounding once to float gives the same
// float (53 >= 2 * 24 + 2: double rounding is innocuous for a quotient).
__device__ __forceinline__ double ms_frcp(double x) { return (double)(float)(1.0 / (double)(float)x); }

__device__ __forceinline__ double ms_dot(const double* a, double x, double y, double z) { return a[0] * x + a[1] * y + a[2] * z; }

// One record per triangle; the same launch also sets the per-point combine words to their identities.
__global__ __launch_bounds__(MS_BLOCK) void mesh_sdf_prep_kernel(const double* __restrict__ tris, int64_t f, double* __restrict__ rec,
                                                                 int64_t n, uint32_t* __restrict__ dist_bits,
                                                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ masks) {
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i < n) {
        masks[i] = 0u;
        if (keys) keys[i] = (uint64_t(0x7f800000u) << 32) | 0xffffffffull;     // (+inf, no triangle)
        else dist_bits[i] = 0x7f800000u;
    }
    if (i >= f) return;
    const double* T = tris + i * 9;
    double* R = rec + i * MS_REC;
    double a[3], b[3], c[3], e10[3], e21[3], e02[3], nn[3];
    for (int k = 0; k < 3; ++k) { a[k] = T[k]; b[k] = T[3 + k]; c[k] = T[6 + k]; }
    for (int k = 0; k < 3; ++k) { e10[k] = b[k] - a[k]; e21[k] = c[k] - b[k]; e02[k] = a[k] - c[k]; }
    nn[0] = e10[1] * e02[2] - e10[2] * e02[1];           // n = e10 x e02
    nn[1] = e10[2] * e02[0] - e10[0] * e02[2];
    nn[2] = e10[0] * e02[1] - e10[1] * e02[0];
    for (int k = 0; k < 3; ++k) { R[R_A + k] = a[k]; R[R_B + k] = b[k]; R[R_C + k] = c[k]; }
    for (int k = 0; k < 3; ++k) { R[R_E10 + k] = e10[k]; R[R_E21 + k] = e21[k]; R[R_E02 + k] = e02[k]; R[R_N + k] = nn[k]; }
    const double* edges[3] = {e10, e21, e02};
    for (int e = 0; e < 3; ++e) {                        // e_k x n
        const double* v = edges[e];
        R[R_CN10 + 3 * e + 0] = v[1] * nn[2] - v[2] * nn[1];
        R[R_CN10 + 3 * e + 1] = v[2] * nn[0] - v[0] * nn[2];
        R[R_CN10 + 3 * e + 2] = v[0] * nn[1] - v[1] * nn[0];
        R[R_R10 + e] = ms_frcp(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    }
    R[R_RN] = ms_frcp(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
    uint32_t flags = (nn[0] != 0.0 || nn[1] != 0.0 || nn[2] != 0.0) ? 0u : FLAG_DEGENERATE;
    const double e2[3] = {-e02[0], -e02[1], -e02[2]};    // e2 = c - a, as the reference negates e02
    for (int d = 0; d < 13; ++d) {
        double dx, dy, dz;
        ms_dir(d, dx, dy, dz);
        const double px = dy * e2[2] - dz * e2[1], py = dz * e2[0] - dx * e2[2], pz = dx * e2[1] - dy * e2[0];
        const double det = e10[0] * px + e10[1] * py + e10[2] * pz;
        const bool tested = !(det > -1e-8 && det < 1e-8);
        R[R_PVEC + 3 * d + 0] = px;
        R[R_PVEC + 3 * d + 1] = py;
        R[R_PVEC + 3 * d + 2] = pz;
        R[R_INVDET + d] = tested ? 1.0 / det : 0.0;
        flags |= tested ? (1u << d) : 0u;
    }
    R[R_FLAGS] = __longlong_as_double((long long)flags);
}

struct MsPoint {
    double x, y, z;
};

template <int D>
__device__ __forceinline__ uint32_t ms_stab(const double* __restrict__ R, double tx, double ty, double tz, double qx, double qy,
                                            double qz, double e2q) {
    const double inv = R[R_INVDET + D];
    const double u = (tx * R[R_PVEC + 3 * D] + ty * R[R_PVEC + 3 * D + 1] + tz * R[R_PVEC + 3 * D + 2]) * inv;
    const double v = ms_dir_dot<D>(qx, qy, qz) * inv;
    const double t = e2q * inv;
    const bool hit = (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0);
    return hit ? (t >= 0.0 ? (1u << D) : (1u << (13 + D))) : 0u;
}

template <int... D>
__device__ __forceinline__ uint32_t ms_stab_all(const double* __restrict__ R, double tx, double ty, double tz, double qx,
                                                double qy, double qz, double e2q, std::integer_sequence<int, D...>) {
    return (ms_stab<D>(R, tx, ty, tz, qx, qy, qz, e2q) | ...);
}

__device__ __forceinline__ float ms_edge(const double* __restrict__ R, int e, int r, double px, double py, double pz) {
    const double ex = R[e], ey = R[e + 1], ez = R[e + 2];
    const float cf = fmaxf(0.0f, fminf((float)((ex * px + ey * py + ez * pz) * R[r]), 1.0f));   // clamp in float (fminf / fmaxf)
    const double c = (double)cf;
    const double t0 = ex * c - px, t1 = ey * c - py, t2 = ez * c - pz;
    return (float)(t0 * t0 + t1 * t1 + t2 * t2);
}

// distsq of one (point, triangle) pair rounded to float, as float bits (0xffffffff for a degenerate triangle), and its sign mask.
__device__ __forceinline__ void ms_pair(const double* __restrict__ R, const MsPoint& p, uint32_t& bits, uint32_t& mask) {
    const uint32_t flags = (uint32_t)__double_as_longlong(R[R_FLAGS]);
    const double p0x = p.x - R[R_A], p0y = p.y - R[R_A + 1], p0z = p.z - R[R_A + 2];
    const double p1x = p.x - R[R_B], p1y = p.y - R[R_B + 1], p1z = p.z - R[R_B + 2];
    const double p2x = p.x - R[R_C], p2y = p.y - R[R_C + 1], p2z = p.z - R[R_C + 2];
    const double s1 = ms_dot(R + R_CN10, p0x, p0y, p0z), s2 = ms_dot(R + R_CN21, p1x, p1y, p1z), s3 = ms_dot(R + R_CN02, p2x, p2y, p2z);
    const bool face = !(signbit(s1) || signbit(s2) || signbit(s3));      // copysign(1, s1) + ... >= 2 <=> no sign bit set
    const float ed = fminf(ms_edge(R, R_E10, R_R10, p0x, p0y, p0z),
                           fminf(ms_edge(R, R_E21, R_R21, p1x, p1y, p1z), ms_edge(R, R_E02, R_R02, p2x, p2y, p2z)));
    const double dn = ms_dot(R + R_N, p0x, p0y, p0z);
    float fd = face ? (float)(dn * dn * R[R_RN]) : ed;
    fd = fd < 0.0f ? 0.0f : fd;
    bits = (flags & FLAG_DEGENERATE) ? 0xffffffffu : __float_as_uint(fd);
    // stabbing tests: tvec = p0, q = tvec x e1, t numerator = e2 . q = -(e02 . q)
    const double e1x = R[R_E10], e1y = R[R_E10 + 1], e1z = R[R_E10 + 2];
    const double qx = p0y * e1z - p0z * e1y, qy = p0z * e1x - p0x * e1z, qz = p0x * e1y - p0y * e1x;
    const double e2q = -ms_dot(R + R_E02, qx, qy, qz);
    const uint32_t hits = ms_stab_all(R, p0x, p0y, p0z, qx, qy, qz, e2q, std::make_integer_sequence<int, 13>{});
    const uint32_t tested = flags & 0x1fffu;
    mask = hits & (tested | (tested << 13));
}

template <bool TRI, bool LDS>
__global__ __launch_bounds__(MS_BLOCK) void mesh_sdf_main_kernel(const double* __restrict__ pts, int64_t n,
                                                                 const double* __restrict__ rec, int64_t f_begin, int64_t f_end,
                                                                 int64_t per_range, uint32_t* __restrict__ dist_bits,
                                                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ masks) {
    const int64_t base = (int64_t)blockIdx.x * MS_TILE + threadIdx.x;
    MsPoint p[MS_PTS];
    uint64_t best[MS_PTS];
    uint32_t acc[MS_PTS];
#pragma unroll
    for (int k = 0; k < MS_PTS; ++k) {
        const int64_t i = min(base + k * MS_BLOCK, n - 1);          // tail lanes evaluate the last point and do not combine
        p[k].x = pts[3 * i];
        p[k].y = pts[3 * i + 1];
        p[k].z = pts[3 * i + 2];
        best[k] = ~0ull;
        acc[k] = 0u;
    }
    const int64_t t0 = f_begin + (int64_t)blockIdx.y * per_range;
    const int64_t t1 = min(t0 + per_range, f_end);

    auto eval = [&](const double* __restrict__ R, int64_t t) {
#pragma unroll
        for (int k = 0; k < MS_PTS; ++k) {
            uint32_t bits, mask;
            ms_pair(R, p[k], bits, mask);
            const uint64_t key = TRI ? ((uint64_t(bits) << 32) | (uint64_t)t) : (uint64_t)bits;
            best[k] = key < best[k] ? key : best[k];                 // ties keep the lower (earlier) index
            acc[k] |= mask;
        }
    };
    if constexpr (LDS) {
        __shared__ double sh[MS_CHUNK * MS_REC];
        for (int64_t c0 = t0; c0 < t1; c0 += MS_CHUNK) {
            const int cnt = (int)min((int64_t)MS_CHUNK, t1 - c0);
            __syncthreads();
            for (int j = threadIdx.x; j < cnt * MS_REC; j += MS_BLOCK) sh[j] = rec[c0 * MS_REC + j];
            __syncthreads();
            for (int k = 0; k < cnt; ++k) eval(sh + k * MS_REC, c0 + k);
        }
    } else {
        for (int64_t t = t0; t < t1; ++t) eval(rec + t * MS_REC, t);    // wave-uniform address: scalar loads
    }
#pragma unroll
    for (int k = 0; k < MS_PTS; ++k) {
        const int64_t i = base + k * MS_BLOCK;
        if (i >= n) continue;
        if (acc[k]) atomicOr(masks + i, acc[k]);
        if (TRI) {
            if (best[k] != ~0ull) atomicMin((unsigned long long*)(keys + i), (unsigned long long)best[k]);
        } else {
            if ((uint32_t)best[k] < 0x7f800000u) atomicMin(dist_bits + i, (uint32_t)best[k]);
        }
    }
}

// sdf = +-sqrtf(min distsq) (negative iff every direction was hit on both sides); the triangle variant also writes the index as
// a double (-1 when every triangle is degenerate), after the N distances (mesh_to_sdf.cpp:36-43 layout).
template <bool TRI>
__global__ __launch_bounds__(MS_BLOCK) void mesh_sdf_finalize_kernel(int64_t n, const uint32_t* __restrict__ dist_bits,
                                                                     const uint64_t* __restrict__ keys,
                                                                     const uint32_t* __restrict__ masks, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t bits = TRI ? (uint32_t)(keys[i] >> 32) : dist_bits[i];
    const float dsq = __uint_as_float(bits);
    const double d = (double)(float)sqrt((double)dsq);             // sqrtf, correctly rounded (double rounding is innocuous)
    const bool inside = masks[i] == 0x3ffffffu;
    out[i] = inside ? -d : d;
    if (TRI) {
        const uint32_t idx = (uint32_t)(keys[i] & 0xffffffffull);
        out[n + i] = idx == 0xffffffffu ? -1.0 : (double)idx;
    }
}

int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

bool stage_lds() {
    static const int v = [] {
        const char* s = getenv("WISP_MESH_SDF_STAGE");
        return (s && s[0] == 'l') ? 1 : 0;
    }();
    return v != 0;
}

template <bool TRI, bool LDS>
void launch_main(dim3 grid, hipStream_t st, const double* points, int64_t n, const double* rec, int64_t f0, int64_t f1,
                 int64_t per_range, uint32_t* dist_bits, uint64_t* keys, uint32_t* masks) {
    mesh_sdf_main_kernel<TRI, LDS><<<grid, MS_BLOCK, 0, st>>>(points, n, rec, f0, f1, per_range, dist_bits, keys, masks);
}

int mesh_sdf_run(const char* fn, bool tri, const double* points, int64_t n, const double* mesh, int64_t f, int triangle_ranges,
                 int64_t max_pairs_per_launch, double* out, void* workspace, int64_t workspace_bytes, wisp_stream_t stream) {
    if (!points || !mesh || !out || !workspace) return wisp_fail(WISP_ERR_INVALID, fn, "null pointer");
    if (n < 1 || f < 1) return wisp_fail(WISP_ERR_INVALID, fn, "need at least one point and one triangle");
    if (f >= 0xffffffffll || n > (int64_t(1) << 40)) return wisp_fail(WISP_ERR_INVALID, fn, "too many triangles or points");
    if (workspace_bytes < wisp_mesh_sdf_workspace_bytes(n, f)) return wisp_fail(WISP_ERR_INVALID, fn, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* rec = (double*)ws;
    char* tail = ws + align256(f * MS_REC * (int64_t)sizeof(double));
    uint64_t* keys = tri ? (uint64_t*)tail : nullptr;
    uint32_t* dist_bits = tri ? nullptr : (uint32_t*)tail;
    uint32_t* masks = (uint32_t*)(tail + align256(n * 8));

    const int64_t prep_n = n > f ? n : f;
    mesh_sdf_prep_kernel<<<(unsigned)ceil_div64(prep_n, MS_BLOCK), MS_BLOCK, 0, st>>>(mesh, f, rec, n, dist_bits, keys, masks);
    WISP_CHECK_LAUNCH();

    const int64_t pblocks = ceil_div64(n, MS_TILE);
    const int64_t cap = max_pairs_per_launch > 0 ? max_pairs_per_launch : MS_MAX_PAIRS;
    int64_t per_launch = cap / (pblocks * MS_TILE);
    if (per_launch < 1) per_launch = 1;
    const bool lds = stage_lds();
    for (int64_t f0 = 0; f0 < f; f0 += per_launch) {
        const int64_t fl = min64(per_launch, f - f0);
        int64_t ranges;
        if (triangle_ranges > 0) {
            ranges = triangle_ranges;
        } else {                                                     // about 8 workgroups per CU, >= 16 triangles per range
            ranges = ceil_div64(2048, pblocks);
            ranges = min64(ranges, ceil_div64(fl, 16));
        }
        ranges = min64(min64(ranges, fl), 65535);
        if (ranges < 1) ranges = 1;
        const int64_t per_range = ceil_div64(fl, ranges);
        ranges = ceil_div64(fl, per_range);
        const dim3 grid((unsigned)pblocks, (unsigned)ranges);
        if (tri) {
            if (lds) launch_main<true, true>(grid, st, points, n, rec, f0, f0 + fl, per_range, dist_bits, keys, masks);
            else launch_main<true, false>(grid, st, points, n, rec, f0, f0 + fl, per_range, dist_bits, keys, masks);
        } else {
            if (lds) launch_main<false, true>(grid, st, points, n, rec, f0, f0 + fl, per_range, dist_bits, keys, masks);
            else launch_main<false, false>(grid, st, points, n, rec, f0, f0 + fl, per_range, dist_bits, keys, masks);
        }
        WISP_CHECK_LAUNCH();
    }
    const unsigned fin = (unsigned)ceil_div64(n, MS_BLOCK);
    if (tri) mesh_sdf_finalize_kernel<true><<<fin, MS_BLOCK, 0, st>>>(n, dist_bits, keys, masks, out);
    else mesh_sdf_finalize_kernel<false><<<fin, MS_BLOCK, 0, st>>>(n, dist_bits, keys, masks, out);
    WISP_CHECK_LAUNCH();
    return WISP_OK;
}

}  // namespace

extern "C" int64_t wisp_mesh_sdf_workspace_bytes(int64_t n, int64_t f) {
    if (n < 0 || f < 0) return 0;
    return align256(f * MS_REC * (int64_t)sizeof(double)) + align256(n * 8) + align256(n * 4);
}

extern "C" int wisp_mesh_to_sdf(const double* points, int64_t n, const double* mesh, int64_t f, int triangle_ranges,
                                int64_t max_pairs_per_launch, double* sdf, void* workspace, int64_t workspace_bytes,
                                wisp_stream_t stream) {
    return mesh_sdf_run(__func__, false, points, n, mesh, f, triangle_ranges, max_pairs_per_launch, sdf, workspace,
                        workspace_bytes, stream);
}

extern "C" int wisp_mesh_to_sdf_triangle(const double* points, int64_t n, const double* mesh, int64_t f, int triangle_ranges,
                                         int64_t max_pairs_per_launch, double* out, void* workspace, int64_t workspace_bytes,
                                         wisp_stream_t stream) {
    return mesh_sdf_run(__func__, true, points, n, mesh, f, triangle_ranges, max_pairs_per_launch, out, workspace,
                        workspace_bytes, stream);
}
