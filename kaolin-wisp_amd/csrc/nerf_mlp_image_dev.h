// The hidden-64 bf16 decoder's operands as ONE image in global memory: the LDS layout of nerf_mlp_bf16.hip's kernels (the permuted,
// row-padded bf16 weight images and the fp32 bias vectors), built once per training step from the packed fp32 parameters and copied
// into LDS by every workgroup of the image kernels - instead of every one of ~770 workgroups fetching the same 42 KB of fp32
// parameters and converting them element by element.  Shared by nerf_mlp_bf16.hip (the kernels, the stand-alone builder) and
// raymarch.hip (trailing workgroups of the coded emit launch build the image of a training step).
#pragma once
#include "nerf_mlp_bf16_dev.h"

namespace wisp_mlp_dev {

// forward operands  [out row][K slots], row stride = K + 8 elements
constexpr int LD1 = 40, LD2 = 72, LD3 = 56, LD4 = 72, LD5 = 72;
constexpr int L_W1 = 0;                     // [64][32]  natural K (the grid features come straight from HBM)
constexpr int L_W2 = L_W1 + 64 * LD1;       // [16][64]  chained K
constexpr int L_W3 = L_W2 + 16 * LD2;       // [64][48]  block 0 chained (density-MLP outputs), blocks 1-2 view encoding
constexpr int L_W4 = L_W3 + 64 * LD3;       // [64][64]  chained
constexpr int L_W5 = L_W4 + 64 * LD4;       // [ 4][64]  chained (3 real rows)
constexpr int L_FWD_END = L_W5 + 4 * LD5;
// backward operands [in row][out-neuron slots]
constexpr int LT5 = 24, LT4 = 72, LT3 = 72, LT2 = 24, LT1 = 72;
constexpr int L_W5T = L_FWD_END;            // [64][16]  slot p < 3 <-> colour channel p
constexpr int L_W4T = L_W5T + 64 * LT5;     // [64][64]
constexpr int L_W3T = L_W4T + 64 * LT4;     // [16][64]  row m <-> density-MLP output m (row 0 unused)
constexpr int L_W2T = L_W3T + 16 * LT3;     // [64][16]
constexpr int L_W1T = L_W2T + 64 * LT2;     // [32][64]
constexpr int L_BWD_END = L_W1T + 32 * LT1;

constexpr int BIASV_FLOATS = 2 * 2 * 2 * 16;            // hidden biases in accumulator layout [layer][t][g][16]

// Image (bytes): [forward operands][bias vectors][small biases: b2[16], b5[3], 0 ...] pad | [backward operands] pad.  Both parts end
// on a 1 KB boundary; the forward kernel copies the first part, the backward kernel everything.  Row paddings and pads hold zeros.
constexpr int IMG_OFF_BIASV = L_FWD_END * 2;
constexpr int IMG_OFF_SMALL = IMG_OFF_BIASV + BIASV_FLOATS * 4;
constexpr int IMG_SMALL_FLOATS = 32;
constexpr int IMG_FWD_BYTES = (IMG_OFF_SMALL + IMG_SMALL_FLOATS * 4 + 1023) / 1024 * 1024;
constexpr int IMG_OFF_BWD = IMG_FWD_BYTES;               // element e >= L_FWD_END of the LDS layout sits at IMG_OFF_BWD + 2 (e - L_FWD_END)
constexpr int IMG_BYTES = (IMG_OFF_BWD + (L_BWD_END - L_FWD_END) * 2 + 1023) / 1024 * 1024;
constexpr int IMG_UNITS = IMG_BYTES / 16;                // 16-byte units, the builder's and the copy's granule
static_assert(IMG_OFF_BIASV % 16 == 0 && (L_BWD_END - L_FWD_END) % 8 == 0, "image parts are whole 16-byte units");

// element e of the LDS layout above (what stage_weights<true> of nerf_mlp_bf16.hip writes there; 0 in the row paddings)
DEV float image_weight(const float* __restrict__ P, int in_dim, int e) {
    auto W = [&](int canonical) { return packed_param(P, canonical, in_dim); };
    if (e < L_W2) { const int r = e / LD1, c = e % LD1; return c < IN ? W(OW1 + r * IN + c) : 0.0f; }
    if (e < L_W3) { e -= L_W2; const int r = e / LD2, s = e % LD2; return s < H ? W(OW2 + r * H + phi(s)) : 0.0f; }
    if (e < L_W4) {
        e -= L_W3;
        const int r = e / LD3, s = e % LD3;
        if (s < 16) { const int m = phi16(s); return m ? W(OW3 + r * X2 + m - 1) : 0.0f; }
        if (s < ONES_SLOT) return W(OW3 + r * X2 + s - 1);
        return s == ONES_SLOT ? W(OB3 + r) : 0.0f;
    }
    if (e < L_W5) { e -= L_W4; const int r = e / LD4, s = e % LD4; return s < H ? W(OW4 + r * H + phi(s)) : 0.0f; }
    if (e < L_FWD_END) { e -= L_W5; const int r = e / LD5, s = e % LD5; return (r < 3 && s < H) ? W(OW5 + r * H + phi(s)) : 0.0f; }
    if (e < L_W4T) { e -= L_W5T; const int k = e / LT5, p = e % LT5; return p < 3 ? W(OW5 + p * H + k) : 0.0f; }
    if (e < L_W3T) { e -= L_W4T; const int k = e / LT4, s = e % LT4; return s < H ? W(OW4 + phi(s) * H + k) : 0.0f; }
    if (e < L_W2T) { e -= L_W3T; const int m = e / LT3, s = e % LT3; return (m && s < H) ? W(OW3 + phi(s) * X2 + m - 1) : 0.0f; }
    if (e < L_W1T) { e -= L_W2T; const int k = e / LT2, p = e % LT2; return p < 16 ? W(OW2 + phi16(p) * H + k) : 0.0f; }
    e -= L_W1T;
    const int k = e / LT1, s = e % LT1;
    return s < H ? W(OW1 + phi(s) * IN + k) : 0.0f;
}

// 16-byte unit u of the image (u < IMG_UNITS): computed from the parameters and stored with one 16-byte store
DEV void build_image_unit(const float* __restrict__ P, int in_dim, unsigned char* __restrict__ image, int u) {
    const int byte = u * 16;
    auto W = [&](int canonical) { return packed_param(P, canonical, in_dim); };
    if (byte >= IMG_OFF_BIASV && byte < IMG_OFF_BWD) {
        float4 v = {0.f, 0.f, 0.f, 0.f};
        float* o = &v.x;
        if (byte < IMG_OFF_SMALL) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = (byte - IMG_OFF_BIASV) / 4 + j;
                const int r = e & 15, g = (e >> 4) & 1, t = (e >> 5) & 1, layer = e >> 6;
                o[j] = W((layer ? OB4 : OB1) + 32 * t + acc_row(r, g));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = (byte - IMG_OFF_SMALL) / 4 + j;
                o[j] = e < 16 ? W(OB2 + e) : (e < 19 ? W(OB5 + e - 16) : 0.0f);
            }
        }
        *reinterpret_cast<float4*>(image + byte) = v;
        return;
    }
    const int e0 = byte < IMG_OFF_BIASV ? byte / 2 : L_FWD_END + (byte - IMG_OFF_BWD) / 2;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = e0 + j < L_BWD_END ? image_weight(P, in_dim, e0 + j) : 0.0f;
    bf16x8 w;
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (__bf16)v[j];
    *reinterpret_cast<bf16x8*>(image + byte) = w;
}

// prologue of the image kernels: the first BYTES of the image into LDS, every load in flight before the first LDS write
template <int THREADS, int BYTES>
DEV void copy_image(unsigned char* lds, const unsigned char* __restrict__ image, int tid) {
    constexpr int UNITS = BYTES / 16, FULL = UNITS / THREADS, REM = UNITS % THREADS;
    const uint4* src = reinterpret_cast<const uint4*>(image);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    uint4 v[FULL], tail = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < FULL; ++k) v[k] = src[tid + k * THREADS];
    if (REM > 0 && tid < REM) tail = src[tid + FULL * THREADS];
#pragma unroll
    for (int k = 0; k < FULL; ++k) dst[tid + k * THREADS] = v[k];
    if (REM > 0 && tid < REM) dst[tid + FULL * THREADS] = tail;
}

}  // namespace wisp_mlp_dev
