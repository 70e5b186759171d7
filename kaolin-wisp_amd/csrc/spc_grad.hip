// Backward of the dual-octree trilinear lookups (OctreeGrid / CodebookOctreeGrid) for gfx950 - order-free by construction.
//
// What it replaces: the backward of kaolin.ops.spc.unbatched_interpolate_trilinear as autograd runs it under
// OctreeGrid._interpolate / interpolate (wisp/models/grids/octree_grid.py:130-219: one lookup per active level, then cat or
// sum) and of CodebookOctreeGrid._index_features + _interpolate (wisp/models/grids/codebook_grid.py:103-172: straight-through
// softmax one-hot over 2^bw dictionary rows per corner).  The reference scatters with float atomics (free order).
//
// Here every corner gradient is a sum of fixed-point integers, which is associative: whatever order the memory-side atomic
// units retire the adds in, the bits of the result are the same.  One call = all levels:
//   1. spc_grad_absmax      M = max |w_corner * g| over every (sample, level, corner, channel) - evaluated with the very float
//                           operations of pass 2, via max_j |w_j| * max_c |g_c| (rounding is monotone) - as an integer max of
//                           float bit patterns (a NaN / inf gradient gives an all-ones exponent and selects the float path)
//   2. spc_grad_scatter     per sample and level: w_j * g_c in float (the reference's products), consecutive samples of one
//                           cell merged in the wave by a fixed-shape segmented scan, run totals converted to
//                           round(v * 2^s) (s from M and the sample count: 8 n 2^s M < 2^62, so no sum can overflow) and added
//                           with 64-bit integer atomics into the accumulator rows of the workspace; touched rows are flagged
//   3. spc_grad_finalize /  every flagged row once: accumulator -> float -> ADDED to the gradient tensor (one writer per
//      codebook_finalize    element), accumulator and flag cleared.  The codebook variant turns the row's G = sum w g into the
//                           logits gradient  p_k (D_k . G - sum_m p_m D_m . G)  and adds scale * G to the dictionary row's
//                           own fixed-point accumulator (LDS, then workspace), which
//   4. codebook_dict_flush  converts (one small launch).
// The workspace (caller-owned, ZERO before its first use) is all zero again when the call returns - except its 64-byte header,
// which every call resets itself.
#include "wisp_common.h"

#define SG_MAX_LODS 16
#define SG_THREADS 128
#ifndef SG_LINK_TAILS
#define SG_LINK_TAILS 8            // a wave links corners across tails when it has more tails than this (see spc_grad_scatter_merge_kernel)
#endif
#define CB_MAX_K 256
#define CB_MAX_F 16

struct SgLods {
    float* grad[SG_MAX_LODS];            // per-level gradient tensor ([rows_l, C] features or [rows_l, K] logits)
    const float* logits[SG_MAX_LODS];    // codebook only
    const float* dict[SG_MAX_LODS];      // codebook only
    float* grad_dict[SG_MAX_LODS];       // codebook only
    int64_t base[SG_MAX_LODS + 1];       // first accumulator row of every level
    int32_t level[SG_MAX_LODS];
};

struct SgHeader { uint32_t absmax_bits; uint32_t pad[15]; };

static inline int sg_stride(int channels) {
    if (channels <= 8) { int s = 1; while (s < channels) s <<= 1; return s; }
    return (channels + 7) / 8 * 8;
}
static inline int64_t sg_round64(int64_t v) { return (v + 63) / 64 * 64; }

// ---- fixed-point scale: values are bounded by M < 2^(E+1); `adds` contributions per accumulator at most
struct SgScale { double to_fix, to_float; int finite; int zero; };
static __device__ __forceinline__ SgScale sg_scale(uint32_t absmax_bits, int clog) {
    SgScale s;
    const int e = (int)(absmax_bits >> 23);
    s.finite = e < 0xf8;                  // (a sum of 64 such values must stay finite as a float too)
    s.zero = absmax_bits == 0;
    const int E = (e < 1 ? 1 : e) - 127;
    const int sh = 60 - clog - E;                                       // 2^clog adds of < 2^(E+1) each stay below 2^61
    s.to_fix = __longlong_as_double((long long)(sh + 1023) << 52);
    s.to_float = __longlong_as_double((long long)(1023 - sh) << 52);
    return s;
}

static __device__ __forceinline__ void sg_coeffs(const float* __restrict__ c, const int16_t* __restrict__ pt, int level,
                                                 float (&w)[8]) {
    // (the statements of trilinear_coeffs in spc_interp.hip: forward and backward must see the same weights)
    const float res = (float)(1 << level);
    float f[3], g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        f[a] = res * (0.5f * c[a] + 0.5f) - (float)pt[a];
        g[a] = 1.0f - f[a];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = ((j & 4) ? f[0] : g[0]) * ((j & 2) ? f[1] : g[1]) * ((j & 1) ? f[2] : g[2]);
}

template <int CTRL> static __device__ __forceinline__ float sg_dpp(float v) {      // v of the lane the DPP control names
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

template <int CTRL> static __device__ __forceinline__ int sg_dpp_i(int v, int fill) {   // lanes without a source lane get `fill`
    return __builtin_amdgcn_update_dpp(fill, v, CTRL, 0xf, 0xf, false);
}

static __device__ __forceinline__ uint32_t sg_wave_umax(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------- pass 1: magnitude bound
template <typename I>
__global__ void __launch_bounds__(256)
spc_grad_absmax_kernel(const float* __restrict__ coords, const I* __restrict__ cells, int64_t cell_stride, int spv,
                       const int16_t* __restrict__ points, SgLods ml, const float* __restrict__ grad_out, int64_t n,
                       int num_lods, int channels, int sum, SgHeader* __restrict__ hdr) {
    const int out_row = sum ? channels : num_lods * channels;
    uint32_t best = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float* g = grad_out + i * out_row;
        uint32_t gsum = 0;
        if (sum)
            for (int c = 0; c < channels; ++c) { const uint32_t b = __float_as_uint(g[c]) & 0x7fffffffu; gsum = b > gsum ? b : gsum; }
        const I* ch = cells + (spv == 1 ? i : i / spv) * cell_stride;
        for (int l = 0; l < num_lods; ++l) {
            const int64_t p = (int64_t)ch[l];
            if (p < 0) continue;
            uint32_t gm = gsum;
            if (!sum) {
                gm = 0;
                for (int c = 0; c < channels; ++c) {
                    const uint32_t b = __float_as_uint(g[l * channels + c]) & 0x7fffffffu;
                    gm = b > gm ? b : gm;
                }
            }
            const float res = (float)(1 << ml.level[l]);
            float wm = 1.0f;
            bool first = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float f = res * (0.5f * coords[i * 3 + a] + 0.5f) - (float)points[p * 3 + a];
                const float m = fmaxf(fabsf(f), fabsf(1.0f - f));
                wm = first ? m : wm * m;                                // (a * b) * c, as the weights are formed
                first = false;
            }
            // |w_j g_c| <= fl(max_j |w_j| * max_c |g_c|): both factors are attained and float rounding is monotone
            const uint32_t b = __float_as_uint(wm * __uint_as_float(gm)) & 0x7fffffffu;
            const uint32_t nb = (gm >= 0x7f800000u || !(wm == wm)) ? 0x7fc00000u : b;       // non-finite anywhere: say so
            best = nb > best ? nb : best;
        }
    }
    best = sg_wave_umax(best);
    // (32 k waves hammering one address cost 0.17 ms; a wave whose maximum is already covered has nothing to say - the plain read
    //  may be stale, which only costs an atomic that changes nothing)
    if ((threadIdx.x & 63) == 0 && best > __atomic_load_n(&hdr->absmax_bits, __ATOMIC_RELAXED)) atomicMax(&hdr->absmax_bits, best);
}

// ---------------------------------------------------------------------------------------------- pass 2: scatter
// Small channel counts (<= 8: nerf_octree / nerf_codebook have 5): one thread owns one sample and keeps its 8 x F products
// in registers.  Consecutive samples of a ray share the cell (16 per cell in the 'voxel' march, long runs on the coarse levels
// of any march), so the wave first adds up each run with a segmented scan - same lanes, same shape, same float adds every
// time - and only the run tails go to memory: all lanes walk the (tail, corner, channel) items, channel fastest, so that the
// F adds of a row sit in neighbouring lanes of one atomic instruction.
template <int F, typename I>
__global__ void __launch_bounds__(SG_THREADS)
spc_grad_scatter_merge_kernel(const float* __restrict__ coords, const I* __restrict__ cells, int64_t cell_stride, int spv,
                              const int16_t* __restrict__ points, const int32_t* __restrict__ trinkets, SgLods ml,
                              const float* __restrict__ grad_out, int64_t n, int num_lods, int sum, int clog, int stride,
                              int direct_stride, const SgHeader* __restrict__ hdr, uint8_t* __restrict__ flags,
                              long long* __restrict__ acc) {
    __shared__ float s_val[SG_THREADS / 64][64][8 * F];
    __shared__ int32_t s_row[SG_THREADS / 64][64][8];
    __shared__ int32_t s_info[SG_THREADS / 64][64];
    __shared__ int8_t s_fwd[SG_THREADS / 64][64 * 8];    // (bytes: the slice must not cost the kernel a workgroup per CU)
    __shared__ int8_t s_bwd[SG_THREADS / 64][64 * 8];
    const SgScale sc = sg_scale(hdr->absmax_bits, clog);
    if (sc.zero) return;                                                 // every product is zero: nothing to add
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool in = i < n;
    const int out_row = sum ? F : num_lods * F;
    float c[3] = {0.0f, 0.0f, 0.0f}, g[F];
#pragma unroll
    for (int f = 0; f < F; ++f) g[f] = 0.0f;
    if (in) {
        c[0] = coords[i * 3]; c[1] = coords[i * 3 + 1]; c[2] = coords[i * 3 + 2];
        if (sum)
#pragma unroll
            for (int f = 0; f < F; ++f) g[f] = grad_out[i * out_row + f];
    }
    const I* ch = cells + (in ? (spv == 1 ? i : i / spv) * cell_stride : 0);
    for (int l = 0; l < num_lods; ++l) {
        const int64_t p = in ? (int64_t)ch[l] : -1;
        float v[8][F];
        if (p >= 0) {
            float w[8];
            sg_coeffs(c, points + p * 3, ml.level[l], w);
            if (!sum)
#pragma unroll
                for (int f = 0; f < F; ++f) g[f] = grad_out[i * out_row + l * F + f];
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int f = 0; f < F; ++f) v[j][f] = w[j] * g[f];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int f = 0; f < F; ++f) v[j][f] = 0.0f;
        }
        // Runs of consecutive samples in one cell (16 per cell in the 'voxel' march, a few in the 'ray' march, long ones on the
        // coarse levels) are added up before anything goes to memory.  Inside every 16-lane row: a segmented inclusive scan with
        // DPP row shifts - no LDS traffic; per step one predicate for all 8 F values, applied as a 0 / 1 factor (x + t * 1 rounds
        // once, like the add; x + t * 0 is x).  A run that continues across a row boundary leaves a partial total at lane 15;
        // it is added to the run's final total when the totals are written out (the corner links below).  Same lanes, same
        // order of adds every time: the float part of the sum is repeatable, the rest is integer.
        const int lane16 = lane & 15;
        const int key = p >= 0 ? (int)p : -1 - lane;                      // (invalid lanes are their own run)
        const int prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
        const bool joins = lane > 0 && prev == key;                       // continues the run of the lane before
        int head = (lane16 == 0 || !joins) ? 1 : 0;
#pragma unroll
        for (int step = 0; step < 4; ++step) {
            const float m = head ? 0.0f : 1.0f;
            int hp;
            if (step == 0) hp = sg_dpp_i<0x111>(head, 1); else if (step == 1) hp = sg_dpp_i<0x112>(head, 1);
            else if (step == 2) hp = sg_dpp_i<0x114>(head, 1); else hp = sg_dpp_i<0x118>(head, 1);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    float t;
                    if (step == 0) t = sg_dpp<0x111>(v[j][f]); else if (step == 1) t = sg_dpp<0x112>(v[j][f]);      // row_shr:1, :2
                    else if (step == 2) t = sg_dpp<0x114>(v[j][f]); else t = sg_dpp<0x118>(v[j][f]);                // row_shr:4, :8
                    v[j][f] = __builtin_fmaf(t, m, v[j][f]);
                }
            head |= hp;
        }
#ifdef SG_EXP_FEWTAILS
        const bool tail = p >= 0 && lane == 63;
#else
        const bool tail = p >= 0 && (lane16 == 15 || next != key);
#endif
        const uint64_t tmask = __ballot(tail);
        if (tmask == 0) continue;                                         // (wave-uniform)
        float (*sv)[8 * F] = s_val[wv];
        int32_t (*sr)[8] = s_row[wv];
        int8_t* fwd = s_fwd[wv];
        int8_t* bwd = s_bwd[wv];
        const int ntails = __popcll(tmask);
        // Consecutive tails often name the same table row: the two halves of a run cut by a row boundary (all eight corners: `carry`
        // / `dropped`, always honoured) and neighbouring cells of a ray, which share a face (four corners).  A corner whose row
        // reappears in the NEXT tail can hand its total on instead of going to memory, and the last tail of such a chain adds the
        // chain up, in order: a third fewer atomic requests - which is what bounds this kernel when runs are short ('ray' march,
        // 5.7 samples per run: 460 -> 383 us), and costs more than it saves when a wave has a handful of tails ('voxel' march, 16
        // samples per cell: 222 -> 264 us).  The wave decides by its tail count.
        const bool links = ntails > SG_LINK_TAILS;
        const uint64_t cont = __ballot(joins && lane16 == 0);            // bit 16 r: row r starts inside the run row r-1 ended with
        if (tail) {
            const int rank = __popcll(tmask & ((1ull << lane) - 1ull));
            const int row0 = lane & ~15;
            const bool first_in_row = ((tmask >> row0) & ((1ull << lane16) - 1ull)) == 0;
            const bool carry = first_in_row && ((cont >> row0) & 1ull);                       // add the total parked by the tail before
            const bool dropped = lane16 == 15 && lane < 63 && ((cont >> (row0 + 16)) & 1ull);  // a partial total: parked, not written out
            s_info[wv][rank] = (carry ? 1 : 0) | (dropped ? 2 : 0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sr[rank][j] = trinkets[p * 8 + j];
#pragma unroll
                for (int f = 0; f < F; ++f) sv[rank][j * F + f] = v[j][f];
            }
        }
        if (links)
            for (int e = lane; e < ntails * 8; e += 64) { fwd[e] = -1; bwd[e] = -1; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (links) {
            for (int e = lane; e < (ntails - 1) * 8; e += 64) {
                const int t = e >> 3;
                const int32_t r = sr[t][e & 7];
                int hit = -1;
#pragma unroll
                for (int q = 0; q < 8; ++q) hit = sr[t + 1][q] == r ? q : hit;       // (the rows of one cell are distinct)
                fwd[e] = (int8_t)hit;
                if (hit >= 0) bwd[(t + 1) * 8 + hit] = (int8_t)(e & 7);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        // all lanes walk the (tail, corner, channel) items, channel fastest: the F adds of a row sit in neighbouring lanes of ONE
        // atomic instruction (the memory side takes them as one request per 64-byte line)
        const int items = ntails * 8 * F;
        const int64_t base = ml.base[l];
        float* gd = ml.grad[l];
        for (int it = lane; it < items; it += 64) {
            const int t = it / (8 * F), rem = it - t * (8 * F);
            const int j = rem / F, f = rem - j * F;
            float total = sv[t][rem];
            if (links) {
                if (fwd[t * 8 + j] >= 0) continue;                        // handed on to the next tail
                for (int k = t, jj = j; k > 0;) {
                    const int b = bwd[k * 8 + jj];
                    if (b < 0) break;
                    --k; jj = b;
                    total += sv[k][jj * F + f];
                }
            } else {
                int info = s_info[wv][t];
                if (info & 2) continue;
                for (int k = t; info & 1;) { --k; total += sv[k][rem]; info = s_info[wv][k]; }
            }
            const int32_t crow = sr[t][j];
            if (sc.finite) {
                const int64_t row = base + crow;
                const long long q = __double2ll_rn((double)total * sc.to_fix);
#ifdef SG_EXP_NOATOMIC
                if (q == 0x7fffffffffffffffll) acc[row * stride + f] = q;
#else
                atomicAdd(reinterpret_cast<unsigned long long*>(acc + row * stride + f), (unsigned long long)q);
#endif
                if (flags && f == 0) flags[row] = 1;
            } else {
                // a non-finite (or nearly overflowing) gradient: plain float atomics straight into the gradient tensor, so that
                // inf / NaN arrive where the reference's atomics would put them (the optimizer step is skipped anyway; the 0 / 1
                // factors of the scan may have turned further lanes into NaN, which changes nothing about that)
                atomicAdd(gd + (int64_t)crow * direct_stride + f, total);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                                  // the slice is rewritten by the next level
    }
}

// Any channel count (NGLOD: 16): consecutive lanes own consecutive channels of one sample, one 64-bit add per product.
template <typename I>
__global__ void __launch_bounds__(256)
spc_grad_scatter_wide_kernel(const float* __restrict__ coords, const I* __restrict__ cells, int64_t cell_stride, int spv,
                             const int16_t* __restrict__ points, const int32_t* __restrict__ trinkets, SgLods ml,
                             const float* __restrict__ grad_out, int64_t n, int num_lods, int channels, int sum, int clog,
                             int stride, int direct_stride, const SgHeader* __restrict__ hdr, uint8_t* __restrict__ flags,
                             long long* __restrict__ acc, int split_lods) {
    const SgScale sc = sg_scale(hdr->absmax_bits, clog);
    if (sc.zero) return;
    const int cpt = channels <= 64 ? channels : 64;
    const int rows_per_block = blockDim.x / cpt;
    const int ch0 = threadIdx.x % cpt;
    if ((int)threadIdx.x / cpt >= rows_per_block) return;
    const int64_t step = (int64_t)gridDim.x * rows_per_block;
    const int out_row = sum ? channels : num_lods * channels;
    const int64_t units = split_lods ? n * num_lods : n;                 // split_lods: one (sample, level) per lane group
    for (int64_t u = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / cpt; u < units; u += step) {
        const int64_t i = split_lods ? u / num_lods : u;
        const int l0 = split_lods ? (int)(u - i * num_lods) : 0, l1 = split_lods ? l0 + 1 : num_lods;
        const I* ch = cells + (spv == 1 ? i : i / spv) * cell_stride;
        for (int l = l0; l < l1; ++l) {
            const int64_t p = (int64_t)ch[l];
            if (p < 0) continue;
            float w[8];
            sg_coeffs(coords + i * 3, points + p * 3, ml.level[l], w);
            const int32_t* tr = trinkets + p * 8;
            for (int c = ch0; c < channels; c += cpt) {
                const float g = grad_out[i * out_row + (sum ? 0 : l * channels) + c];
                if (sc.finite) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int64_t row = ml.base[l] + tr[j];
                        const long long q = __double2ll_rn((double)(g * w[j]) * sc.to_fix);
                        atomicAdd(reinterpret_cast<unsigned long long*>(acc + row * stride + c), (unsigned long long)q);
                        if (flags && c == 0) flags[row] = 1;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) atomicAdd(ml.grad[l] + (int64_t)tr[j] * direct_stride + c, g * w[j]);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- pass 3: accumulators -> gradients
static __device__ __forceinline__ int sg_level_of(const SgLods& ml, int num_lods, int64_t row) {
    int l = 0;
    while (l + 1 < num_lods && row >= ml.base[l + 1]) ++l;
    return l;
}

__global__ void __launch_bounds__(256)
spc_grad_finalize_kernel(SgLods ml, int num_lods, int channels, int stride, int lpr /* lanes per row: power of two <= 64 */,
                         int clog, const SgHeader* __restrict__ hdr, uint8_t* __restrict__ flags, long long* __restrict__ acc) {
    const SgScale sc = sg_scale(hdr->absmax_bits, clog);
    const int64_t total = ml.base[num_lods];
    const int rpb = blockDim.x / lpr, lane = threadIdx.x % lpr;
    for (int64_t row = (int64_t)blockIdx.x * rpb + threadIdx.x / lpr; row < total; row += (int64_t)gridDim.x * rpb) {
        if (flags && !flags[row]) continue;                              // (all lanes of a row sit in one wave: read before the clear)
        const int l = sg_level_of(ml, num_lods, row);
        float* gd = ml.grad[l] + (row - ml.base[l]) * channels;
        long long* a = acc + row * stride;
        for (int c = lane; c < channels; c += lpr) {
            const long long q = a[c];
            if (q != 0) { gd[c] += (float)((double)q * sc.to_float); a[c] = 0; }
        }
        if (flags && lane == 0) flags[row] = 0;
    }
}

// Codebook: one thread per logits row.  d logits[row, k] = p_k (D_k . G - sum_m p_m D_m . G); d dictionary[argmax] += scale G
// with scale = (1 - p) + p, the forward value of the straight-through key (codebook_grid.py:117-125).
template <int KR>
__global__ void __launch_bounds__(256)
codebook_grad_finalize_kernel(SgLods ml, int lod_begin, int lod_end, int K, int F, int stride, int clog,
                              const SgHeader* __restrict__ hdr, uint8_t* __restrict__ flags, long long* __restrict__ acc,
                              long long* __restrict__ dict_acc) {
    extern __shared__ __align__(16) unsigned char s_raw[];
    const int nl = lod_end - lod_begin;
    long long* s_gdict = reinterpret_cast<long long*>(s_raw);            // [nl * K * F] fixed-point dictionary gradient
    float* s_dict = reinterpret_cast<float*>(s_gdict + (size_t)nl * K * F);   // [nl * K * F] dictionaries
    for (int e = threadIdx.x; e < nl * K * F; e += blockDim.x) {
        s_gdict[e] = 0;
        s_dict[e] = ml.dict[lod_begin + e / (K * F)][e % (K * F)];
    }
    __syncthreads();
    const SgScale sc = sg_scale(hdr->absmax_bits, clog);
    const int64_t first = ml.base[lod_begin], last = ml.base[lod_end];
    for (int64_t row = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < last; row += (int64_t)gridDim.x * blockDim.x) {
        long long* a = acc + row * stride;
        if (flags) {
            if (!flags[row]) continue;
            flags[row] = 0;
        } else {
            bool any = false;
#pragma unroll
            for (int f = 0; f < CB_MAX_F; ++f) if (f < F) any |= a[f] != 0;
            if (!any) continue;                                          // untouched (or cancelled to exactly zero: nothing to add)
        }
        int l = lod_begin;
        while (l + 1 < lod_end && row >= ml.base[l + 1]) ++l;
        const int64_t r = row - ml.base[l];
        long long q[CB_MAX_F];                                           // (constant trip counts + guards: these stay in registers)
        float G[CB_MAX_F];
#pragma unroll
        for (int f = 0; f < CB_MAX_F; ++f) {
            q[f] = 0; G[f] = 0.0f;
            if (f < F) { q[f] = a[f]; a[f] = 0; G[f] = (float)((double)q[f] * sc.to_float); }
        }
        const float* lrow = ml.logits[l] + r * K;
        float* grow = ml.grad[l] + r * K;
        const float* D = s_dict + (size_t)(l - lod_begin) * K * F;
        int best = 0;
        float inv;
        if (KR > 0) {
            // the row in registers (K <= KR, a multiple of four: 16-byte loads), every exponential and dictionary product once
            float x[KR > 0 ? KR : 1], e[KR > 0 ? KR : 1];
#pragma unroll
            for (int k4 = 0; k4 < KR; k4 += 4)
                if (k4 < K) {
                    const float4 t = *reinterpret_cast<const float4*>(lrow + k4);
                    x[k4] = t.x; x[k4 + 1] = t.y; x[k4 + 2] = t.z; x[k4 + 3] = t.w;
                }
            float mx = x[0];
#pragma unroll
            for (int k = 1; k < KR; ++k) if (k < K && x[k] > mx) { mx = x[k]; best = k; }    // first max wins (torch.max)
            float denom = 0.0f;
#pragma unroll
            for (int k = 0; k < KR; ++k) if (k < K) { e[k] = expf(x[k] - mx); denom += e[k]; }
            inv = 1.0f / denom;
            // argmax of the softmax VALUES, first index on ties (codebook_softmax_pick, wisp_common.h), on the registers at hand
#pragma unroll
            for (int k = KR - 1; k >= 0; --k) if (k < best && e[k] * inv == inv) best = k;
            float dot = 0.0f;
#pragma unroll
            for (int k = 0; k < KR; ++k)
                if (k < K) {
                    float dk = 0.0f;
#pragma unroll
                    for (int f = 0; f < CB_MAX_F; ++f) if (f < F) dk += D[k * F + f] * G[f];
                    x[k] = dk;
                    dot += e[k] * inv * dk;
                }
#pragma unroll
            for (int k4 = 0; k4 < KR; k4 += 4)
                if (k4 < K) {
                    float4 t = *reinterpret_cast<float4*>(grow + k4);
                    t.x += e[k4] * inv * (x[k4] - dot); t.y += e[k4 + 1] * inv * (x[k4 + 1] - dot);
                    t.z += e[k4 + 2] * inv * (x[k4 + 2] - dot); t.w += e[k4 + 3] * inv * (x[k4 + 3] - dot);
                    *reinterpret_cast<float4*>(grow + k4) = t;
                }
        } else {
            float mx = lrow[0];
            for (int k = 1; k < K; ++k) { const float x = lrow[k]; if (x > mx) { mx = x; best = k; } }   // first max wins (torch.max)
            float denom = 0.0f;
            for (int k = 0; k < K; ++k) denom += expf(lrow[k] - mx);
            inv = 1.0f / denom;
            best = codebook_softmax_pick(lrow, best, mx, inv);
            float dot = 0.0f;
            for (int k = 0; k < K; ++k) {
                float dk = 0.0f;
#pragma unroll
                for (int f = 0; f < CB_MAX_F; ++f) if (f < F) dk += D[k * F + f] * G[f];
                dot += expf(lrow[k] - mx) * inv * dk;
            }
            for (int k = 0; k < K; ++k) {
                float dk = 0.0f;
#pragma unroll
                for (int f = 0; f < CB_MAX_F; ++f) if (f < F) dk += D[k * F + f] * G[f];
                grow[k] += expf(lrow[k] - mx) * inv * (dk - dot);
            }
        }
        const double scale = (double)((1.0f - inv) + inv);
        long long* sg = s_gdict + ((size_t)(l - lod_begin) * K + best) * F;
#pragma unroll
        for (int f = 0; f < CB_MAX_F; ++f)
            if (f < F && q[f] != 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(sg + f), (unsigned long long)__double2ll_rn((double)q[f] * scale));
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nl * K * F; e += blockDim.x) {
        const long long x = s_gdict[e];
        if (x != 0) atomicAdd(reinterpret_cast<unsigned long long*>(dict_acc + (size_t)lod_begin * K * F + e), (unsigned long long)x);
    }
}

__global__ void __launch_bounds__(256)
codebook_dict_flush_kernel(SgLods ml, int num_lods, int KF, int clog, const SgHeader* __restrict__ hdr,
                           long long* __restrict__ dict_acc) {
    const SgScale sc = sg_scale(hdr->absmax_bits, clog);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < num_lods * KF; e += gridDim.x * blockDim.x) {
        const long long q = dict_acc[e];
        if (q == 0) continue;
        dict_acc[e] = 0;
        ml.grad_dict[e / KF][e % KF] += (float)((double)q * sc.to_float);
    }
}

// ---------------------------------------------------------------------------------------------- host side
struct SgPlan { int64_t total_rows, dict_elems, off_dict, off_flags, off_acc, bytes; int stride; };

static SgPlan sg_plan(int64_t total_rows, int channels, int64_t dict_elems) {
    SgPlan p;
    p.total_rows = total_rows; p.dict_elems = dict_elems; p.stride = sg_stride(channels);
    p.off_dict = (int64_t)sizeof(SgHeader);
    p.off_flags = p.off_dict + sg_round64(dict_elems * 8);
    p.off_acc = p.off_flags + sg_round64(total_rows);
    p.bytes = p.off_acc + total_rows * p.stride * 8;
    return p;
}

extern "C" int64_t wisp_spc_bwd_workspace_bytes(int64_t total_rows, int channels, int64_t dict_elems) {
    if (total_rows < 0 || channels < 1 || dict_elems < 0) return -1;
    return sg_plan(total_rows, channels, dict_elems).bytes;
}

static int sg_clog(int64_t n) {                                           // ceil(log2(8 n)): adds one accumulator can receive
    int c = 3;
    while (((int64_t)1 << (c - 3)) < n) ++c;
    return c;
}

struct SgCall {
    const float* coords; const void* cells; int cells_is_i64; int64_t cell_stride; int spv;
    const int16_t* points; const int32_t* trinkets; const float* grad_out; int64_t n; int num_lods; int channels; int sum;
    int direct_stride;                                                    // row stride of the gradient tensors (non-finite path)
};

// Touched-row flags (one byte store per scattered row, one byte read per table row in pass 3) pay off when a launch reaches a
// small part of a big table - NGLOD's 512 coordinates in a million rows; when most rows are touched anyway (a 2 M-sample NeRF
// batch over 0.2 M rows) pass 3 reads the accumulators themselves and pass 2 saves its 2.5 M scattered byte stores.
static bool sg_use_flags(const SgCall& c, const SgPlan& pl) { return c.n * 8 * c.num_lods < pl.total_rows; }

// few samples (an NGLOD step has 512): the levels of a sample go to different lane groups, or a handful of workgroups would walk
// all levels one after the other with the rest of the chip idle
static int sg_split_lods(const SgCall& c) { return c.num_lods > 1 && c.n * (c.channels <= 64 ? c.channels : 64) < (int64_t)256 * 1024; }

// passes 1 and 2; have_absmax: the caller has zeroed the header and a kernel of its own leaves the magnitude bound there (pass 1)
static int sg_scatter(const SgCall& c, const SgLods& ml, const SgPlan& pl, unsigned char* ws, hipStream_t s, bool have_absmax = false) {
    SgHeader* hdr = reinterpret_cast<SgHeader*>(ws);
    uint8_t* flags = sg_use_flags(c, pl) ? ws + pl.off_flags : nullptr;
    long long* acc = reinterpret_cast<long long*>(ws + pl.off_acc);
    const int clog = sg_clog(c.n);
    if (!have_absmax) {
        if (hipMemsetAsync(hdr, 0, sizeof(SgHeader), s) != hipSuccess) return -1;
        const unsigned g1 = (unsigned)min64(ceil_div64(c.n, 256), 4096);
#define SG_ABSMAX(I) hipLaunchKernelGGL((spc_grad_absmax_kernel<I>), dim3(g1), dim3(256), 0, s, c.coords, (const I*)c.cells,   \
                                        c.cell_stride, c.spv, c.points, ml, c.grad_out, c.n, c.num_lods, c.channels, c.sum, hdr)
        if (c.cells_is_i64) SG_ABSMAX(int64_t); else SG_ABSMAX(int32_t);
#undef SG_ABSMAX
    }
    if (c.channels <= 8) {
        const dim3 grid((unsigned)ceil_div64(c.n, SG_THREADS)), block(SG_THREADS);
#define SG_MERGE(FF, I) hipLaunchKernelGGL((spc_grad_scatter_merge_kernel<FF, I>), grid, block, 0, s, c.coords, (const I*)c.cells, \
                                           c.cell_stride, c.spv, c.points, c.trinkets, ml, c.grad_out, c.n, c.num_lods, c.sum, \
                                           clog, pl.stride, c.direct_stride, hdr, flags, acc)
#define SG_CASE(FF) case FF: if (c.cells_is_i64) SG_MERGE(FF, int64_t); else SG_MERGE(FF, int32_t); break;
        switch (c.channels) { SG_CASE(1) SG_CASE(2) SG_CASE(3) SG_CASE(4) SG_CASE(5) SG_CASE(6) SG_CASE(7) SG_CASE(8) }
#undef SG_CASE
#undef SG_MERGE
    } else {
        const int cpt = c.channels <= 64 ? c.channels : 64;
        const int split = sg_split_lods(c);
        const dim3 grid((unsigned)min64(ceil_div64(c.n * (split ? c.num_lods : 1), 256 / cpt), 16384)), block(256);
#define SG_WIDE(I) hipLaunchKernelGGL((spc_grad_scatter_wide_kernel<I>), grid, block, 0, s, c.coords, (const I*)c.cells,         \
                                      c.cell_stride, c.spv, c.points, c.trinkets, ml, c.grad_out, c.n, c.num_lods, c.channels,  \
                                      c.sum, clog, pl.stride, c.direct_stride, hdr, flags, acc, split)
        if (c.cells_is_i64) SG_WIDE(int64_t); else SG_WIDE(int32_t);
#undef SG_WIDE
    }
    return 0;
}

static int sg_fill(SgLods& ml, const int32_t* levels, const int64_t* rows, int num_lods) {
    for (int l = 0; l < SG_MAX_LODS; ++l) {
        ml.grad[l] = nullptr; ml.logits[l] = nullptr; ml.dict[l] = nullptr; ml.grad_dict[l] = nullptr; ml.level[l] = 0; ml.base[l] = 0;
    }
    ml.base[SG_MAX_LODS] = 0;
    int64_t b = 0;
    for (int l = 0; l < num_lods; ++l) {
        if (levels[l] < 0 || levels[l] > 15 || rows[l] < 0) return -1;
        ml.level[l] = levels[l];
        ml.base[l] = b;
        b += rows[l];
    }
    for (int l = num_lods; l <= SG_MAX_LODS; ++l) ml.base[l] = b;
    return 0;
}

// pass 3 of the feature tables
static void sg_finalize(const SgCall& c, const SgLods& ml, const SgPlan& pl, unsigned char* ws, hipStream_t s) {
    int lpr = 1;
    while (lpr < c.channels && lpr < 64) lpr <<= 1;
    const unsigned g3 = (unsigned)min64(ceil_div64(pl.total_rows, 256 / lpr), 8192);
    if (pl.total_rows > 0)
        hipLaunchKernelGGL(spc_grad_finalize_kernel, dim3(g3), dim3(256), 0, s, ml, c.num_lods, c.channels, pl.stride, lpr,
                           sg_clog(c.n), reinterpret_cast<const SgHeader*>(ws), sg_use_flags(c, pl) ? ws + pl.off_flags : nullptr,
                           reinterpret_cast<long long*>(ws + pl.off_acc));
}

static int spc_bwd_impl(const SgCall& c, const int32_t* levels, const int64_t* rows, float* const* grad_feats, void* workspace,
                        int64_t workspace_bytes, hipStream_t s) {
    SgLods ml;
    if (sg_fill(ml, levels, rows, c.num_lods) != 0) return wisp_fail(WISP_ERR_INVALID, __func__, "bad level or row count");
    for (int l = 0; l < c.num_lods; ++l) {
        if (!grad_feats[l]) return wisp_fail(WISP_ERR_INVALID, __func__, "null gradient pointer");
        ml.grad[l] = grad_feats[l];
    }
    const SgPlan pl = sg_plan(ml.base[c.num_lods], c.channels, 0);
    if (!workspace || workspace_bytes < pl.bytes) return wisp_fail(WISP_ERR_INVALID, __func__, "workspace missing or too small (wisp_spc_bwd_workspace_bytes)");
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    if (sg_scatter(c, ml, pl, ws, s) != 0) return wisp_fail(WISP_ERR_LAUNCH, __func__, "hipMemsetAsync failed");
    sg_finalize(c, ml, pl, ws, s);
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, __func__, hipGetErrorString(e_));
    return WISP_OK;
}

extern "C" int wisp_spc_trilinear_bwd(const float* coords, const void* pidx, int pidx_is_i64, const int16_t* points,
                                      const int32_t* trinkets, const float* grad_out, int64_t num_voxels,
                                      int samples_per_voxel, int channels, int level, int64_t num_rows, float* grad_feats,
                                      void* workspace, int64_t workspace_bytes, wisp_stream_t stream) {
    WISP_REQUIRE(num_voxels >= 0 && samples_per_voxel >= 1 && channels >= 1 && level >= 0 && level <= 15 && num_rows >= 0, "bad sizes");
    if (num_voxels == 0) return WISP_OK;
    WISP_REQUIRE(coords && pidx && points && trinkets && grad_out && grad_feats, "null pointer");
    WISP_REQUIRE(num_voxels * samples_per_voxel < ((int64_t)1 << 40), "too many samples for one launch");
    SgCall c{coords, pidx, pidx_is_i64, 1, samples_per_voxel, points, trinkets, grad_out, num_voxels * samples_per_voxel, 1,
             channels, 1, channels};
    const int32_t lv[1] = {level};
    const int64_t rw[1] = {num_rows};
    float* const gp[1] = {grad_feats};
    return spc_bwd_impl(c, lv, rw, gp, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int wisp_spc_trilinear_multi_bwd(const float* coords, const int64_t* chain, int64_t chain_stride,
                                            const int16_t* points, const int32_t* trinkets, const float* grad_out,
                                            int64_t num_samples, int num_lods, const int32_t* levels, const int64_t* rows,
                                            int channels, int sum, float* const* grad_feats, void* workspace,
                                            int64_t workspace_bytes, wisp_stream_t stream) {
    WISP_REQUIRE(num_samples >= 0 && num_lods >= 1 && num_lods <= SG_MAX_LODS && channels >= 1 && chain_stride >= num_lods, "bad sizes");
    if (num_samples == 0) return WISP_OK;
    WISP_REQUIRE(coords && chain && points && trinkets && grad_out && levels && rows && grad_feats, "null pointer");
    WISP_REQUIRE(num_samples < ((int64_t)1 << 40), "too many samples for one launch");
    SgCall c{coords, chain, 1, chain_stride, 1, points, trinkets, grad_out, num_samples, num_lods, channels, sum, channels};
    return spc_bwd_impl(c, levels, rows, grad_feats, workspace, workspace_bytes, (hipStream_t)stream);
}

static int codebook_bwd_impl(const SgCall& c, const int32_t* levels, const int64_t* rows, const float* const* logits,
                             const float* const* dictionaries, int dict_size, float* const* grad_logits,
                             float* const* grad_dictionaries, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    const int K = dict_size, F = c.channels;
    SgLods ml;
    if (sg_fill(ml, levels, rows, c.num_lods) != 0) return wisp_fail(WISP_ERR_INVALID, __func__, "bad level or row count");
    for (int l = 0; l < c.num_lods; ++l) {
        if (!logits[l] || !dictionaries[l] || !grad_logits[l] || !grad_dictionaries[l])
            return wisp_fail(WISP_ERR_INVALID, __func__, "null table pointer");
        ml.grad[l] = grad_logits[l]; ml.logits[l] = logits[l]; ml.dict[l] = dictionaries[l]; ml.grad_dict[l] = grad_dictionaries[l];
    }
    const int64_t dict_elems = (int64_t)c.num_lods * K * F;
    const SgPlan pl = sg_plan(ml.base[c.num_lods], F, dict_elems);
    if (!workspace || workspace_bytes < pl.bytes) return wisp_fail(WISP_ERR_INVALID, __func__, "workspace missing or too small (wisp_spc_bwd_workspace_bytes)");
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    // (non-finite path: G cannot be scattered into the logits gradient rows - they are K wide - so it goes to the first F
    //  columns, which is where a non-finite value has to show up for the found-inf check; see the header)
    if (sg_scatter(c, ml, pl, ws, s) != 0) return wisp_fail(WISP_ERR_LAUNCH, __func__, "hipMemsetAsync failed");
    const SgHeader* hdr = reinterpret_cast<const SgHeader*>(ws);
    uint8_t* flags = sg_use_flags(c, pl) ? ws + pl.off_flags : nullptr;
    long long* acc = reinterpret_cast<long long*>(ws + pl.off_acc);
    long long* dict_acc = reinterpret_cast<long long*>(ws + pl.off_dict);
    const int clog = sg_clog(c.n);
    // all levels in one launch while their dictionaries (+ fixed-point gradients) fit the default LDS window, else level groups
    const size_t per_level = (size_t)K * F * 12;
    int group = (int)(48 * 1024 / per_level);
    if (group < 1) group = 1;
    bool rows16 = true;                                                   // 16-byte loads of the logits rows need aligned tensors
    for (int l = 0; l < c.num_lods; ++l)
        rows16 = rows16 && ((reinterpret_cast<uintptr_t>(logits[l]) | reinterpret_cast<uintptr_t>(grad_logits[l])) & 15) == 0;
    for (int lb = 0; lb < c.num_lods; lb += group) {
        const int le = lb + group < c.num_lods ? lb + group : c.num_lods;
        const int64_t nrows = ml.base[le] - ml.base[lb];
        if (nrows == 0) continue;
        const unsigned g3 = (unsigned)min64(ceil_div64(nrows, 256), 2048);
        if (K % 4 == 0 && K <= 16 && rows16)
            hipLaunchKernelGGL(codebook_grad_finalize_kernel<16>, dim3(g3), dim3(256), (size_t)(le - lb) * per_level, s, ml, lb, le, K, F,
                               pl.stride, clog, hdr, flags, acc, dict_acc);
        else
            hipLaunchKernelGGL(codebook_grad_finalize_kernel<0>, dim3(g3), dim3(256), (size_t)(le - lb) * per_level, s, ml, lb, le, K, F,
                               pl.stride, clog, hdr, flags, acc, dict_acc);
    }
    hipLaunchKernelGGL(codebook_dict_flush_kernel, dim3((unsigned)min64(ceil_div64(dict_elems, 256), 64)), dim3(256), 0, s, ml,
                       c.num_lods, K * F, clog, hdr, dict_acc);
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, __func__, hipGetErrorString(e_));
    return WISP_OK;
}

extern "C" int wisp_codebook_trilinear_bwd(const float* coords, const void* pidx, int pidx_is_i64, const int16_t* points,
                                           const int32_t* trinkets, const float* logits, const float* dictionary,
                                           const float* grad_out, int64_t num_voxels, int samples_per_voxel, int dict_size,
                                           int feature_dim, int level, int64_t num_logit_rows, float* grad_logits,
                                           float* grad_dictionary, void* workspace, int64_t workspace_bytes,
                                           wisp_stream_t stream) {
    WISP_REQUIRE(num_voxels >= 0 && samples_per_voxel >= 1 && level >= 0 && level <= 15 && num_logit_rows >= 0, "bad sizes");
    WISP_REQUIRE(dict_size >= 1 && dict_size <= CB_MAX_K && feature_dim >= 1 && feature_dim <= CB_MAX_F && feature_dim <= dict_size,
                 "dictionary shape outside the fused kernels (dict_size <= 256, feature_dim <= min(16, dict_size))");
    if (num_voxels == 0) return WISP_OK;
    WISP_REQUIRE(coords && pidx && points && trinkets && logits && dictionary && grad_out && grad_logits && grad_dictionary, "null pointer");
    SgCall c{coords, pidx, pidx_is_i64, 1, samples_per_voxel, points, trinkets, grad_out, num_voxels * samples_per_voxel, 1,
             feature_dim, 1, dict_size};
    const int32_t lv[1] = {level};
    const int64_t rw[1] = {num_logit_rows};
    const float* const lg[1] = {logits};
    const float* const dc[1] = {dictionary};
    float* const gl[1] = {grad_logits};
    float* const gd[1] = {grad_dictionary};
    return codebook_bwd_impl(c, lv, rw, lg, dc, dict_size, gl, gd, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int wisp_codebook_trilinear_multi_bwd(const float* coords, const int64_t* chain, int64_t chain_stride,
                                                 const int16_t* points, const int32_t* trinkets, const float* const* logits,
                                                 const float* const* dictionaries, const float* grad_out, int64_t num_samples,
                                                 int num_lods, const int32_t* levels, const int64_t* rows, int dict_size,
                                                 int feature_dim, int sum, float* const* grad_logits,
                                                 float* const* grad_dictionaries, void* workspace, int64_t workspace_bytes,
                                                 wisp_stream_t stream) {
    WISP_REQUIRE(num_samples >= 0 && num_lods >= 1 && num_lods <= SG_MAX_LODS && chain_stride >= num_lods, "bad sizes");
    WISP_REQUIRE(dict_size >= 1 && dict_size <= CB_MAX_K && feature_dim >= 1 && feature_dim <= CB_MAX_F && feature_dim <= dict_size,
                 "dictionary shape outside the fused kernels (dict_size <= 256, feature_dim <= min(16, dict_size))");
    if (num_samples == 0) return WISP_OK;
    WISP_REQUIRE(coords && chain && points && trinkets && logits && dictionaries && grad_out && levels && rows && grad_logits
                 && grad_dictionaries, "null pointer");
    SgCall c{coords, chain, 1, chain_stride, 1, points, trinkets, grad_out, num_samples, num_lods, feature_dim, sum, dict_size};
    return codebook_bwd_impl(c, levels, rows, logits, dictionaries, dict_size, grad_logits, grad_dictionaries, workspace,
                             workspace_bytes, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- fused SDF regression step
// One optimisation step of the reference's SDFTrainer (wisp/trainers/sdf_trainer.py:65-124, only_last) over an OctreeGrid, for
// both of its fields.  A NeuralSDF (wisp/models/nefs/neural_sdf.py:102-155; nglod_octree.yaml: 16 'sum' features on 6 levels,
// [position, features] -> Linear(19, 128) -> relu -> Linear(128, 1), 512 coordinates per step) has one decoder output:
//     pred = decoder([x, sum_l trilinear_l(x)]) ;  loss = sum (pred - gt)^2 / B ;  backward
// A NeuralSDFTex (neural_sdf_tex.py:95-123, sample_tex) has four, rgb = sigmoid(y[0:3]), sdf = y[3], the position is optional:
//     in = pos_input ? [x, f] : f ;  loss = (sum (rgb - rgb_gt)^2 + sum (sdf - gt)^2) / B
// The reference issues ~60 kernels for the step (a query, six trilinear lookups, two GEMMs with their elementwise companions,
// the loss, and all of that again backwards); the modular path of this package 20.  At 512 coordinates every one of them is
// launch latency.  Here:
//   sdf_train_kernel<NOUT>  one kernel for NOUT = 1 or 4 decoder outputs; only the loss head is written per field.
//                        Phase 1 (st_lookup): 16 lanes per (sample, level) walk the octree to the level's cell and blend its
//                        corners (all levels of a sample at once, so the dependent loads of the walk cost the deepest level's,
//                        not the sum; inference has the same statements in sdf_eval_point, sdf_eval_dev.h).  Phase 2: 16 lanes
//                        per sample run the decoder forward, d loss / d y (g = 2 diff / B; through the sigmoid, g_o = 2 diff_o
//                        c_o (1 - c_o) / B) and the decoder backward: lane c keeps hidden units c, c + 16, ..., d
//                        pre-activation[h] = (a_h > 0) sum_o W2[o][h] g_o in ascending o, the gradient of the decoder input
//                        is a column sum over LDS.  Phase 3: the weight gradients and squared errors of the workgroup are
//                        summed by the thread that owns the entry, in sample order, and stored as one partial row - no
//                        atomics.  The sample's feature gradient [16] and cell chain go to scratch; the workgroup's largest
//                        |w g| goes to the header of the order-free scatter, which therefore needs no magnitude pass.
//   sdf_train_reduce_kernel  adds the partial rows up in workgroup order, ADDS the sums to the decoder's gradient tensors, writes
//                        the loss: loss[0] = sum / B for one output, loss[3] = {total / B, distance sum, colour sum} for four.
//   spc_grad_scatter_wide + spc_grad_finalize   the corner sums of all levels (64-bit fixed point, above).
// Every sum has a fixed order or is an integer sum: the step is bitwise repeatable.  The two instantiations round apart in two
// places only, kept on purpose and marked "rounding" below: with inert colour rows (W2[0:3] = 0, b2[0:3] = 0, colour target
// 0.5: g_0..2 = 0 exactly) every sum that reaches dW1, db1 and the feature tables is the one-output instantiation's, term by
// term in the same order, and those gradients are bitwise equal.
#define ST_GROUP 16
#define ST_GROUPS 16                       // samples per workgroup pass
#define ST_MAX_HIDDEN 256

struct StField {
    const float* feats[SG_MAX_LODS];
    int32_t level[SG_MAX_LODS];
    int num_lods, channels, half_round, hidden, max_level, pos_input;
    const float *w1, *b1, *w2, *b2;          // [hidden][in_dim], [hidden], [n_out][hidden], [n_out]
};

// squared errors a sample leaves behind: its distance error and, with colour outputs, its colour error
static __host__ __device__ constexpr int st_n_sq(int n_out) { return n_out == 1 ? 1 : 2; }

// Every size of the step, from (hidden, in_dim, n_out), for the scratch sizes, the host body and both kernels.
//   a workgroup's partial row = the entries of the reduce kernel: dW1 [H][in_dim] at 0, db1 [H] at e_b1, dW2 [n_out][H] at e_w2,
//   db2 [n_out] at e_b2, the squared-error sums at e_sq and, where there are two of them, their total; `entries` in all,
//   rows row_stride apart
//   the dynamic LDS of sdf_train_kernel, as offsets in floats; `floats` = its size
struct StLayout { int e_b1, e_w2, e_b2, e_sq, entries, row_stride, w1, b1, w2, in, ga, r, g, sq, lev, wm, own, floats; };
static __host__ __device__ inline StLayout st_layout(int hidden, int in_dim, int n_out) {
    StLayout s;
    s.e_b1 = hidden * in_dim;
    s.e_w2 = s.e_b1 + hidden;
    s.e_b2 = s.e_w2 + n_out * hidden;
    s.e_sq = s.e_b2 + n_out;
    s.entries = s.e_sq + st_n_sq(n_out) + (st_n_sq(n_out) > 1);
    s.row_stride = (s.entries + 15) / 16 * 16;
    s.w1 = 0;                                           // [H][in_dim | 1]      odd row stride: the lanes of a group read different rows
    s.b1 = s.w1 + hidden * (in_dim | 1);                // [H]
    s.w2 = s.b1 + hidden;                               // [n_out][H]
    s.in = s.w2 + n_out * hidden;                       // [spb][in_dim]        decoder inputs of the pass
    s.ga = s.in + ST_GROUPS * in_dim;                   // [spb][H]             d loss / d pre-activation
    s.r = s.ga + ST_GROUPS * hidden;                    // [spb][H]             relu output (one output: times d loss / d pred)
    s.g = s.r + ST_GROUPS * hidden;                     // [spb][n_out]         d loss / d y
    s.sq = s.g + ST_GROUPS * n_out;                     // [spb][n_sq]          squared distance error (, squared colour error)
    s.lev = s.sq + ST_GROUPS * st_n_sq(n_out);          // [groups][C]          one level's lookup of one sample
    s.wm = s.lev + ST_GROUPS * ST_GROUP;                // [groups]             its largest corner weight
    s.own = s.wm + ST_GROUPS;                           // [entries]            this workgroup's partial row
    s.floats = s.own + s.entries;
    return s;
}
static inline int st_grid(int64_t n, int num_lods) { return (int)min64(ceil_div64(n, ST_GROUPS / num_lods), 1024); }
static inline int64_t st_scratch_bytes(int64_t n, int num_lods, int channels, int hidden, int in_dim, int n_out) {
    return (int64_t)st_grid(n, num_lods) * st_layout(hidden, in_dim, n_out).row_stride * 4 + sg_round64(n * channels * 4) + n * num_lods * 8;
}

// Phase 1 for one (sample, level) pair, all 16 lanes of its group together: walk to the cell of sample s on level fld.level[li]
// (node = -1 outside the cube or in an unoccupied cell), blend feature channel c of its corners (acc; it and wm come in as 0) and
// return the largest corner weight (wm); lane 0 records the node at node_out.  The blend is an fmaf chain over the corners in
// corner order from +0, as sdf_eval_point spells it (the other products are by powers of two: exact, fused or not).
static __device__ __forceinline__ void st_lookup(const StField& fld, const float* __restrict__ coords, const uint8_t* __restrict__ octree,
                                                 const int32_t* __restrict__ exsum, const int16_t* __restrict__ points,
                                                 const int32_t* __restrict__ trinkets, int64_t s, int li, int c,
                                                 int64_t* __restrict__ node_out, float& acc, float& wm) {
#pragma clang fp contract(off)
    const int C = fld.channels, L = fld.max_level;
    const float px = coords[s * 3], py = coords[s * 3 + 1], pz = coords[s * 3 + 2];
    const bool inside = (fabsf(px) <= 1.0f) && (fabsf(py) <= 1.0f) && (fabsf(pz) <= 1.0f);
    const float res = (float)(1 << L);
    const int top = (1 << L) - 1;
    const int qx = min((int)floorf(res * (0.5f * px + 0.5f)), top);
    const int qy = min((int)floorf(res * (0.5f * py + 0.5f)), top);
    const int qz = min((int)floorf(res * (0.5f * pz + 0.5f)), top);
    const float pos[3] = {px, py, pz};
    const int lv = fld.level[li];
    int64_t node = inside ? 0 : -1;
    for (int l = 0; l < lv && node >= 0; ++l) {                           // (spc_query_kernel's walk)
        const int sh = L - 1 - l, cs = (((qx >> sh) & 1) << 2) | (((qy >> sh) & 1) << 1) | ((qz >> sh) & 1);
        const uint32_t bits = octree[node];                               // both loads of a level go out together: one round
        const int64_t first = (int64_t)exsum[node];                       // trip per level, not two
        const int64_t child = first + __popc(bits & ((2u << cs) - 1u));
        node = ((bits >> cs) & 1u) ? child : -1;
    }
    if (c == 0) *node_out = node;                                         // (now: the node need not live through the blend)
    if (node >= 0) {
        float w[8];
        sg_coeffs(pos, points + node * 3, lv, w);
#pragma unroll
        for (int j = 0; j < 8; ++j) wm = fmaxf(wm, fabsf(w[j]));
        const int32_t* tr = trinkets + node * 8;
        const float* f = fld.feats[li];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float fv = f[(int64_t)tr[j] * C + c];
            if (fld.half_round) fv = __half2float(__float2half_rn(fv));
            acc = __builtin_fmaf(fv, w[j], acc);
        }
        if (fld.half_round) acc = __half2float(__float2half_rn(acc));
    }
}

template <int NOUT>
__global__ void __launch_bounds__(ST_GROUP * ST_GROUPS)
sdf_train_kernel(const float* __restrict__ coords, const float* __restrict__ gts, const float* __restrict__ rgb_gts /* NOUT == 4 */,
                 int64_t n, const uint8_t* __restrict__ octree, const int32_t* __restrict__ exsum, const int16_t* __restrict__ points,
                 const int32_t* __restrict__ trinkets, StField fld, float inv_batch, float* __restrict__ partials /* [grid][row] */,
                 float* __restrict__ dfeat /* [n][channels] */, int64_t* __restrict__ chain /* [n][num_lods] */, SgHeader* __restrict__ hdr) {
    // Every fused multiply-add is written as one, here and in st_lookup, and the compiler's own contraction is off: left to it,
    // one source fused the corner blend and the colour error in one way as a kernel of its own and in another as an instantiation
#pragma clang fp contract(off)
    static_assert(NOUT == 1 || NOUT == 4, "one output (distance) or four (colour, distance)");
    constexpr int NSQ = st_n_sq(NOUT);
    extern __shared__ float s_st[];
    const int C = fld.channels, H = fld.hidden, NL = fld.num_lods;
    const int fo = fld.pos_input ? 3 : 0;               // first feature column of the decoder input
    const int in_dim = fo + C;
    const int in_pad = in_dim | 1;
    const int spb = ST_GROUPS / NL;                     // samples per workgroup pass: one lane group per (sample, level)
    const StLayout lay = st_layout(H, in_dim, NOUT);
    float *s_w1 = s_st + lay.w1, *s_b1 = s_st + lay.b1, *s_w2 = s_st + lay.w2, *s_in = s_st + lay.in, *s_ga = s_st + lay.ga;
    float *s_r = s_st + lay.r, *s_g = s_st + lay.g, *s_sq = s_st + lay.sq, *s_lev = s_st + lay.lev, *s_wm = s_st + lay.wm;
    float* s_own = s_st + lay.own;                      // every entry of the partial row has one owner
    for (int e = threadIdx.x; e < H * in_dim; e += blockDim.x) s_w1[(e / in_dim) * in_pad + e % in_dim] = fld.w1[e];
    for (int e = threadIdx.x; e < H; e += blockDim.x) s_b1[e] = fld.b1[e];
    for (int e = threadIdx.x; e < NOUT * H; e += blockDim.x) s_w2[e] = fld.w2[e];
    for (int e = threadIdx.x; e < lay.entries; e += blockDim.x) s_own[e] = 0.0f;
    const int c = threadIdx.x & (ST_GROUP - 1);
    const int grp = threadIdx.x / ST_GROUP;
    float b2[NOUT];
    for (int o = 0; o < NOUT; ++o) b2[o] = fld.b2[o];
    uint32_t mbits = 0;
    const int my_si = grp / NL, my_li = grp - my_si * NL;                 // phase 1: this group's (sample of the pass, level)
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * spb; base < n; base += (int64_t)gridDim.x * spb) {
        // ---- phase 1: every (sample, level) pair on its own lane group: six groups walking at once cost the deepest one's time
        {
            const int64_t s = base + my_si;
            float acc = 0.0f, wm = 0.0f;
            if (my_si < spb && s < n) st_lookup(fld, coords, octree, exsum, points, trinkets, s, my_li, c, chain + s * NL + my_li, acc, wm);
            s_lev[grp * ST_GROUP + c] = acc;
            if (c == 0) s_wm[grp] = wm;
        }
        __syncthreads();
        // ---- phase 2: group si owns sample si of the pass: decoder forward, d loss / d y, decoder backward
        const int64_t s = base + grp;
        const bool live = grp < spb && s < n;
        float* gin = s_in + grp * in_dim;
        float* ga = s_ga + grp * H;
        float* gr = s_r + grp * H;
        float wmax = 0.0f;
        if (live) {
            float feat = 0.0f;                                            // channel c, summed over the levels in order
            for (int li = 0; li < NL; ++li) {
                feat += s_lev[(grp * NL + li) * ST_GROUP + c];
                wmax = fmaxf(wmax, s_wm[grp * NL + li]);
            }
            if (c < fo) gin[c] = coords[s * 3 + c];
            gin[fo + c] = feat;
        }
        __builtin_amdgcn_wave_barrier();                 // a group's lanes are in one wave: LDS order suffices
        if (live) {
            // decoder forward: in = [position, features] (the modules put the embedded position first) or the features alone
            float out[NOUT] = {};
            for (int hh = c; hh < H; hh += ST_GROUP) {
                const float* wr = s_w1 + hh * in_pad;
                float a = s_b1[hh];
                for (int i = 0; i < in_dim; ++i) a = __builtin_fmaf(wr[i], gin[i], a);
                const float r = fmaxf(a, 0.0f);
                for (int o = 0; o < NOUT; ++o) out[o] = __builtin_fmaf(s_w2[o * H + hh], r, out[o]);
                ga[hh] = a > 0.0f ? 1.0f : 0.0f;        // the relu mask; finished below, once d loss / d y is known
                gr[hh] = r;
            }
#pragma unroll
            for (int d = ST_GROUP / 2; d >= 1; d >>= 1)
                for (int o = 0; o < NOUT; ++o) out[o] += __shfl_xor(out[o], d, ST_GROUP);
            // ---- the loss head, the one part that differs by field: g = d loss / d y, sq = the sample's squared errors.  The
            //      distance is the last output; the colours before it go through a sigmoid
            float g[NOUT], sq[NSQ];
            const float dd = (out[NOUT - 1] + b2[NOUT - 1]) - gts[s];
            g[NOUT - 1] = 2.0f * dd * inv_batch;         // d [sum (sdf - gt)^2 / B] / d sdf
            sq[0] = dd * dd;
            if constexpr (NOUT == 4) {
                float d[3];
                for (int o = 0; o < 3; ++o) {
                    const float co = 1.0f / (1.0f + expf(-(out[o] + b2[o])));
                    d[o] = co - rgb_gts[s * 3 + o];
                    g[o] = 2.0f * d[o] * (co * (1.0f - co)) * inv_batch;      // d loss / d y_o through the sigmoid
                }
                sq[1] = __builtin_fmaf(d[1], d[1], d[0] * d[0]) + d[2] * d[2];
            }
            // ---- end of the loss head
            for (int hh = c; hh < H; hh += ST_GROUP) {
                // rounding: one output forms the plain product; four form an fmaf chain from +0, which differs from it where the
                // first product is -0 - each keeps its own
                float t = NOUT == 1 ? s_w2[hh] * g[0] : __builtin_fmaf(s_w2[hh], g[0], 0.0f);
                for (int o = 1; o < NOUT; ++o) t = __builtin_fmaf(s_w2[o * H + hh], g[o], t);
                // the relu's backward SELECTS: a unit that is off passes 0 on, also for a non-finite g, where a product with the
                // mask would be 0 * inf = NaN
                ga[hh] = ga[hh] != 0.0f ? t : 0.0f;
                if constexpr (NOUT == 1) gr[hh] *= g[0];                      // rounding: see d W2 in phase 3
            }
            if (c == 0) {
                for (int o = 0; o < NOUT; ++o) s_g[grp * NOUT + o] = g[o];
                for (int k = 0; k < NSQ; ++k) s_sq[grp * NSQ + k] = sq[k];
            }
        } else if (grp < spb) {
            for (int hh = c; hh < H; hh += ST_GROUP) { ga[hh] = 0.0f; gr[hh] = 0.0f; }
            if (c < fo) gin[c] = 0.0f;
            gin[fo + c] = 0.0f;
            if (c < NOUT) s_g[grp * NOUT + c] = 0.0f;
            if (c < NSQ) s_sq[grp * NSQ + c] = 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
        if (live) {
            // gradient of the decoder input, feature columns only (nothing consumes d / d position)
            float dx = 0.0f;
            for (int hh = 0; hh < H; ++hh) dx = __builtin_fmaf(ga[hh], s_w1[hh * in_pad + fo + c], dx);
            dfeat[s * C + c] = dx;
            const uint32_t b = __float_as_uint(wmax * fabsf(dx)) & 0x7fffffffu;
            const uint32_t nb = (!(dx == dx) || !(wmax == wmax)) ? 0x7fc00000u : b;
            mbits = nb > mbits ? nb : mbits;
        }
        __syncthreads();
        // ---- phase 3: weight gradients of this pass: the thread that owns an entry adds the samples up in order
        for (int e = threadIdx.x; e < lay.entries; e += blockDim.x) {
            float acc = 0.0f;
            if (e < lay.e_b1) {
                const int hh = e / in_dim, i = e - hh * in_dim;
                for (int q = 0; q < spb; ++q) acc = __builtin_fmaf(s_ga[q * H + hh], s_in[q * in_dim + i], acc);
            } else if (e < lay.e_w2) {
                const int hh = e - lay.e_b1;
                for (int q = 0; q < spb; ++q) acc += s_ga[q * H + hh];
            } else if (e < lay.e_b2) {
                // rounding: d W2 of one output adds the products r * g that phase 2 stored (a rounded product, then a plain add);
                // four outputs keep r and fuse, fmaf(g, r, acc).  The two differ in the last bit, and each keeps its own.
                const int o = NOUT == 1 ? 0 : (e - lay.e_w2) / H, hh = (e - lay.e_w2) - o * H;
                for (int q = 0; q < spb; ++q)
                    acc = NOUT == 1 ? acc + s_r[q * H + hh] : __builtin_fmaf(s_g[q * NOUT + o], s_r[q * H + hh], acc);
            } else if (e < lay.e_sq) {
                for (int q = 0; q < spb; ++q) acc += s_g[q * NOUT + (e - lay.e_b2)];
            } else if (e < lay.e_sq + NSQ) {
                for (int q = 0; q < spb; ++q) acc += s_sq[q * NSQ + (e - lay.e_sq)];
            } else if constexpr (NSQ == 2) {                                  // the total: colour + distance, in that order
                for (int q = 0; q < spb; ++q) acc += s_sq[q * 2 + 1] + s_sq[q * 2];
            }
            s_own[e] += acc;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < lay.entries; e += blockDim.x) partials[(int64_t)blockIdx.x * lay.row_stride + e] = s_own[e];
    mbits = sg_wave_umax(mbits);
    if ((threadIdx.x & 63) == 0 && mbits > __atomic_load_n(&hdr->absmax_bits, __ATOMIC_RELAXED)) atomicMax(&hdr->absmax_bits, mbits);
}

__global__ void __launch_bounds__(256)
sdf_train_reduce_kernel(const float* __restrict__ partials, int rows, int H, int in_dim, int n_out,
                        float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2,
                        float* __restrict__ loss, float inv_batch) {
    // 16 lanes per entry: lane r adds rows r, r + 16, ... in order, then a fixed butterfly over the 16 lanes
    const StLayout lay = st_layout(H, in_dim, n_out);
    const int r0 = threadIdx.x & 15;
    for (int e = blockIdx.x * 16 + (threadIdx.x >> 4); e < lay.entries + 15; e += gridDim.x * 16) {          // (whole groups stay together)
        const bool in = e < lay.entries;
        float acc = 0.0f;
        if (in)
            for (int r = r0; r < rows; r += 16) acc += partials[(int64_t)r * lay.row_stride + e];
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 16);
        if (!in || r0 != 0) continue;
        if (e < lay.e_b1) gw1[e] += acc;
        else if (e < lay.e_w2) gb1[e - lay.e_b1] += acc;
        else if (e < lay.e_b2) gw2[e - lay.e_w2] += acc;
        else if (e < lay.e_sq) gb2[e - lay.e_b2] += acc;
        else if (e == lay.entries - 1) loss[0] = acc * inv_batch;                 // the last entry is the whole squared error
        else loss[1 + (e - lay.e_sq)] = acc;          // un-normalised: what the tracker adds up as l2_loss, then as rgb_loss
    }
}

// The body of both entry points, after their own argument checks; who = the entry point, for its error messages
template <int NOUT>
static int st_step(const char* who, const float* coords, const float* gts, const float* rgb_gts, int64_t n, const uint8_t* octree,
                   const int32_t* exsum, const int16_t* points, const int32_t* trinkets, const float* const* feats,
                   const int32_t* levels, const int64_t* rows, int num_lods, int channels, int half_round, int pos_input,
                   const float* w1, const float* b1, const float* w2, const float* b2, int hidden, float* const* grad_feats,
                   float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, float* loss, void* scratch, void* workspace,
                   int64_t workspace_bytes, hipStream_t s) {
    StField fld;
    SgLods ml;
    if (sg_fill(ml, levels, rows, num_lods) != 0) return wisp_fail(WISP_ERR_INVALID, who, "bad level or row count");
    for (int l = 0; l < num_lods; ++l) {
        if (!(feats[l] && grad_feats[l] && (l == 0 || levels[l] > levels[l - 1]))) return wisp_fail(WISP_ERR_INVALID, who, "bad level list");
        fld.feats[l] = feats[l]; fld.level[l] = levels[l]; ml.grad[l] = grad_feats[l];
    }
    fld.num_lods = num_lods; fld.channels = channels; fld.half_round = half_round; fld.hidden = hidden;
    fld.max_level = levels[num_lods - 1]; fld.pos_input = pos_input;
    fld.w1 = w1; fld.b1 = b1; fld.w2 = w2; fld.b2 = b2;
    const SgPlan pl = sg_plan(ml.base[num_lods], channels, 0);
    if (workspace_bytes < pl.bytes) return wisp_fail(WISP_ERR_INVALID, who, "workspace too small (wisp_spc_bwd_workspace_bytes)");
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    SgHeader* hdr = reinterpret_cast<SgHeader*>(ws);
    const int in_dim = (pos_input ? 3 : 0) + channels;
    const int grid = st_grid(n, num_lods);
    const StLayout lay = st_layout(hidden, in_dim, NOUT);
    float* partials = static_cast<float*>(scratch);
    float* dfeat = partials + (size_t)grid * lay.row_stride;
    int64_t* chain = reinterpret_cast<int64_t*>(reinterpret_cast<unsigned char*>(dfeat) + sg_round64(n * channels * 4));
    const size_t lds = (size_t)lay.floats * sizeof(float);
    const float inv_batch = 1.0f / (float)n;
    if (hipMemsetAsync(hdr, 0, sizeof(SgHeader), s) != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, who, "hipMemsetAsync failed");
    if (const hipError_t e = WISP_ALLOW_LDS(sdf_train_kernel<NOUT>, lds)) return wisp_fail(WISP_ERR_LAUNCH, who, hipGetErrorString(e));
    hipLaunchKernelGGL(sdf_train_kernel<NOUT>, dim3(grid), dim3(ST_GROUP * ST_GROUPS), lds, s, coords, gts, rgb_gts, n, octree, exsum,
                       points, trinkets, fld, inv_batch, partials, dfeat, chain, hdr);
    hipLaunchKernelGGL(sdf_train_reduce_kernel, dim3((lay.entries + 15) / 16), dim3(256), 0, s, partials, grid, hidden, in_dim, NOUT,
                       grad_w1, grad_b1, grad_w2, grad_b2, loss, inv_batch);
    // the corner sums: the magnitude bound is in the header already (sdf_train_kernel), so only scatter + row pass
    const SgCall c{coords, chain, 1, num_lods, 1, points, trinkets, dfeat, n, num_lods, channels, 1, channels};
    sg_scatter(c, ml, pl, ws, s, true);                                   // (without its memset nothing in it can fail)
    sg_finalize(c, ml, pl, ws, s);
    if (const hipError_t e = hipGetLastError()) return wisp_fail(WISP_ERR_LAUNCH, who, hipGetErrorString(e));
    return WISP_OK;
}

extern "C" int64_t wisp_sdf_train_scratch_bytes(int64_t n, int num_lods, int channels, int hidden) {
    if (n < 0 || num_lods < 1 || num_lods > SG_MAX_LODS || channels < 1 || hidden < 1) return -1;
    return st_scratch_bytes(n, num_lods, channels, hidden, 3 + channels, 1);
}

extern "C" int wisp_sdf_train_step(const float* coords, const float* gts, int64_t n, const uint8_t* octree, const int32_t* exsum,
                                   const int16_t* points, const int32_t* trinkets, const float* const* feats,
                                   const int32_t* levels, const int64_t* rows, int num_lods, int channels, int half_round,
                                   const float* w1, const float* b1, const float* w2, const float* b2, int hidden,
                                   float* const* grad_feats, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2,
                                   float* loss, void* scratch, int64_t scratch_bytes, void* workspace, int64_t workspace_bytes,
                                   wisp_stream_t stream) {
    WISP_REQUIRE(n >= 1 && num_lods >= 1 && num_lods <= SG_MAX_LODS, "bad sizes");
    WISP_REQUIRE(channels == ST_GROUP, "the fused SDF step is built for 16 feature channels (nglod_octree.yaml)");
    WISP_REQUIRE(hidden >= 1 && hidden <= ST_MAX_HIDDEN, "hidden width out of range");
    WISP_REQUIRE(coords && gts && octree && exsum && points && trinkets && feats && levels && rows && w1 && b1 && w2 && b2 &&
                 grad_feats && grad_w1 && grad_b1 && grad_w2 && grad_b2 && loss && scratch && workspace, "null pointer");
    WISP_REQUIRE(scratch_bytes >= wisp_sdf_train_scratch_bytes(n, num_lods, channels, hidden), "scratch too small (wisp_sdf_train_scratch_bytes)");
    return st_step<1>(__func__, coords, gts, nullptr, n, octree, exsum, points, trinkets, feats, levels, rows, num_lods, channels,
                      half_round, 1, w1, b1, w2, b2, hidden, grad_feats, grad_w1, grad_b1, grad_w2, grad_b2, loss, scratch, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

extern "C" int64_t wisp_sdf_tex_train_scratch_bytes(int64_t n, int num_lods, int channels, int hidden, int pos_input) {
    if (n < 0 || num_lods < 1 || num_lods > SG_MAX_LODS || channels != ST_GROUP || hidden < 1 || hidden > ST_MAX_HIDDEN ||
        (pos_input != 0 && pos_input != 1))
        return -1;
    return st_scratch_bytes(n, num_lods, channels, hidden, (pos_input ? 3 : 0) + channels, 4);
}

extern "C" int wisp_sdf_tex_train_step(const float* coords, const float* gts, const float* rgb_gts, int64_t n, const uint8_t* octree,
                                       const int32_t* exsum, const int16_t* points, const int32_t* trinkets,
                                       const float* const* feats, const int32_t* levels, const int64_t* rows, int num_lods,
                                       int channels, int half_round, int pos_input, const float* w1, const float* b1,
                                       const float* w2, const float* b2, int hidden, float* const* grad_feats, float* grad_w1,
                                       float* grad_b1, float* grad_w2, float* grad_b2, float* loss, void* scratch,
                                       int64_t scratch_bytes, void* workspace, int64_t workspace_bytes, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 1 && num_lods >= 1 && num_lods <= SG_MAX_LODS, "bad sizes");
    WISP_REQUIRE(channels == ST_GROUP, "the fused textured SDF step is built for 16 feature channels");
    WISP_REQUIRE(hidden >= 1 && hidden <= ST_MAX_HIDDEN, "hidden width out of range");
    WISP_REQUIRE(pos_input == 0 || pos_input == 1, "pos_input must be 0 or 1");
    WISP_REQUIRE(coords && gts && rgb_gts && octree && exsum && points && trinkets && feats && levels && rows && w1 && b1 && w2 &&
                 b2 && grad_feats && grad_w1 && grad_b1 && grad_w2 && grad_b2 && loss && scratch && workspace, "null pointer");
    WISP_REQUIRE(scratch_bytes >= wisp_sdf_tex_train_scratch_bytes(n, num_lods, channels, hidden, pos_input),
                 "scratch too small (wisp_sdf_tex_train_scratch_bytes)");
    return st_step<4>(__func__, coords, gts, rgb_gts, n, octree, exsum, points, trinkets, feats, levels, rows, num_lods, channels,
                      half_round, pos_input, w1, b1, w2, b2, hidden, grad_feats, grad_w1, grad_b1, grad_w2, grad_b2, loss, scratch,
                      workspace, workspace_bytes, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- fused all-LOD SDF regression step
// The same step with the loss taken over EVERY level of detail (sdf_trainer.py:80-123 without only_last), for the same two fields:
//     x_k = [position,] sum_{l <= k} blend_l  (the running sum in level order: what the one-LOD step forms on the first k + 1 levels)
//     y_k = decoder(x_k) ;  S_k = sum_s (sdf_k - gt)^2 ;  R_k = sum_s |rgb_k - rgb_gt|^2
//     loss = (sum_k w_sdf[k] S_k + sum_k w_rgb[k] R_k) / B
// sdf_train_kernel gives one 16-lane group to each (sample, level) pair for the lookup and leaves all but 16 / L of them idle
// through the decoder.  Here the group that looked level k up goes on to run LOD k:
//   sdf_lods_train_kernel<NOUT>
//     Phase 1: st_lookup, unchanged.
//     Phase 2: group (si, k) = row q = si L + k adds the blends 0..k of its sample up in level order from +0, then runs the
//              statements of sdf_train_kernel's phase 2 on its own rows of the LDS arrays; the loss head scales the constant:
//              g = (2 w[k]) diff ... / B (w = 1 leaves the one-LOD statements and their rounding as they are).  Lane 0 leaves
//              S, (R,) and the row's share of the total, T = w_sdf[k] S (one output) or w_rgb[k] R + w_sdf[k] S (four: two rounded
//              products, one add).  d loss / d x_k, feature columns, goes to LDS.
//     Phase 3: the owner of an entry adds the rows up in ascending q = si L + k - sample-major, LOD-minor - with the statements of
//              sdf_train_kernel; S_k and R_k add the rows of LOD k in sample order, the total adds T in ascending q.
//              Group (si, l) forms the gradient of level l's blend, sum_{k >= l} d loss / d x_k, starting from k = l and adding
//              in ascending k, and stores it as column block l of dfeat [n][L 16]; the header's magnitude bound is that SUM times
//              level l's largest corner weight.  The scatter takes the blocks as 'cat' columns (sum = 0).
//   sdf_lods_train_reduce_kernel   sdf_train_reduce_kernel's sums (lane r adds rows r, r + 16, ... in order, then a fixed
//              butterfly); loss[0] = total / B, loss[1 + k] = S_k, loss[1 + L + k] = R_k.
// Every float sum has one of these orders; the table sums are the 64-bit fixed-point ones.  With L = 1 and weights 1 every
// statement that reaches a result is sdf_train_kernel's, in its order: the results are bitwise equal.
struct StLodW { float sdf[SG_MAX_LODS], rgb[SG_MAX_LODS]; };

// st_layout's sibling: the partial row has S_k [L] (, R_k [L]) at e_sq and the total at e_tot; the LDS rows of s_sq hold
// {S, (R,) T}; df [groups][C] is d loss / d x_k of the pass, wt [2][SG_MAX_LODS] the weights
struct StLodsLayout { int e_b1, e_w2, e_b2, e_sq, e_tot, entries, row_stride, w1, b1, w2, in, ga, r, g, sq, lev, df, wt, own, floats; };
static __host__ __device__ inline StLodsLayout st_lods_layout(int hidden, int in_dim, int n_out, int num_lods) {
    StLodsLayout s;
    s.e_b1 = hidden * in_dim;
    s.e_w2 = s.e_b1 + hidden;
    s.e_b2 = s.e_w2 + n_out * hidden;
    s.e_sq = s.e_b2 + n_out;
    s.e_tot = s.e_sq + st_n_sq(n_out) * num_lods;
    s.entries = s.e_tot + 1;
    s.row_stride = (s.entries + 15) / 16 * 16;
    s.w1 = 0;
    s.b1 = s.w1 + hidden * (in_dim | 1);
    s.w2 = s.b1 + hidden;
    s.in = s.w2 + n_out * hidden;
    s.ga = s.in + ST_GROUPS * in_dim;
    s.r = s.ga + ST_GROUPS * hidden;
    s.g = s.r + ST_GROUPS * hidden;
    s.sq = s.g + ST_GROUPS * n_out;
    s.lev = s.sq + ST_GROUPS * (st_n_sq(n_out) + 1);
    s.df = s.lev + ST_GROUPS * ST_GROUP;
    s.wt = s.df + ST_GROUPS * ST_GROUP;
    s.own = s.wt + 2 * SG_MAX_LODS;
    s.floats = s.own + s.entries;
    return s;
}
static inline int64_t st_lods_scratch_bytes(int64_t n, int num_lods, int channels, int hidden, int in_dim, int n_out) {
    return (int64_t)st_grid(n, num_lods) * st_lods_layout(hidden, in_dim, n_out, num_lods).row_stride * 4 +
           sg_round64(n * num_lods * channels * 4) + n * num_lods * 8;
}

template <int NOUT>
__global__ void __launch_bounds__(ST_GROUP * ST_GROUPS)
sdf_lods_train_kernel(const float* __restrict__ coords, const float* __restrict__ gts, const float* __restrict__ rgb_gts /* NOUT == 4 */,
                      int64_t n, const uint8_t* __restrict__ octree, const int32_t* __restrict__ exsum,
                      const int16_t* __restrict__ points, const int32_t* __restrict__ trinkets, StField fld, StLodW wt, float inv_batch,
                      float* __restrict__ partials /* [grid][row] */, float* __restrict__ dfeat /* [n][num_lods][channels] */,
                      int64_t* __restrict__ chain /* [n][num_lods] */, SgHeader* __restrict__ hdr) {
#pragma clang fp contract(off)                          // (as in sdf_train_kernel: every fused multiply-add is written as one)
    static_assert(NOUT == 1 || NOUT == 4, "one output (distance) or four (colour, distance)");
    constexpr int NSQ = st_n_sq(NOUT), NSQ1 = NSQ + 1;
    extern __shared__ float s_st[];
    const int C = fld.channels, H = fld.hidden, NL = fld.num_lods;
    const int fo = fld.pos_input ? 3 : 0;
    const int in_dim = fo + C;
    const int in_pad = in_dim | 1;
    const int spb = ST_GROUPS / NL;                     // samples per workgroup pass
    const int nrows = spb * NL;                         // (sample, LOD) rows of a pass; the groups behind them idle
    const StLodsLayout lay = st_lods_layout(H, in_dim, NOUT, NL);
    float *s_w1 = s_st + lay.w1, *s_b1 = s_st + lay.b1, *s_w2 = s_st + lay.w2, *s_in = s_st + lay.in, *s_ga = s_st + lay.ga;
    float *s_r = s_st + lay.r, *s_g = s_st + lay.g, *s_sq = s_st + lay.sq, *s_lev = s_st + lay.lev;
    float *s_df = s_st + lay.df, *s_wt = s_st + lay.wt, *s_own = s_st + lay.own;
    for (int e = threadIdx.x; e < H * in_dim; e += blockDim.x) s_w1[(e / in_dim) * in_pad + e % in_dim] = fld.w1[e];
    for (int e = threadIdx.x; e < H; e += blockDim.x) s_b1[e] = fld.b1[e];
    for (int e = threadIdx.x; e < NOUT * H; e += blockDim.x) s_w2[e] = fld.w2[e];
    for (int e = threadIdx.x; e < lay.entries; e += blockDim.x) s_own[e] = 0.0f;
    if (threadIdx.x < SG_MAX_LODS) { s_wt[threadIdx.x] = wt.sdf[threadIdx.x]; s_wt[SG_MAX_LODS + threadIdx.x] = wt.rgb[threadIdx.x]; }
    const int c = threadIdx.x & (ST_GROUP - 1);
    const int grp = threadIdx.x / ST_GROUP;
    float b2[NOUT];
    for (int o = 0; o < NOUT; ++o) b2[o] = fld.b2[o];
    uint32_t mbits = 0;
    const int my_si = grp / NL, my_li = grp - my_si * NL;                 // this group's (sample of the pass, level = LOD), both phases
    float* gin = s_in + grp * in_dim;
    float* ga = s_ga + grp * H;
    float* gr = s_r + grp * H;
    __syncthreads();
    const float two_ws = 2.0f * s_wt[my_li];                              // (2 w) first: exact, and 2 itself for w = 1
    for (int64_t base = (int64_t)blockIdx.x * spb; base < n; base += (int64_t)gridDim.x * spb) {
        const int64_t s = base + my_si;
        const bool live = my_si < spb && s < n;
        // ---- phase 1: every (sample, level) pair on its own lane group
        float wm1 = 0.0f;
        {
            float acc = 0.0f;
            if (live) st_lookup(fld, coords, octree, exsum, points, trinkets, s, my_li, c, chain + s * NL + my_li, acc, wm1);
            s_lev[grp * ST_GROUP + c] = acc;
        }
        __syncthreads();
        // ---- phase 2: the same group runs LOD my_li of its sample on row grp: decoder forward, d loss / d y, decoder backward
        if (live) {
            float feat = 0.0f;                                            // channel c, summed over the levels 0..k in order
            for (int li = 0; li <= my_li; ++li) feat += s_lev[(grp - my_li + li) * ST_GROUP + c];
            if (c < fo) gin[c] = coords[s * 3 + c];
            gin[fo + c] = feat;
        }
        __builtin_amdgcn_wave_barrier();                 // a group's lanes are in one wave: LDS order suffices
        if (live) {
            float out[NOUT] = {};
            for (int hh = c; hh < H; hh += ST_GROUP) {
                const float* wr = s_w1 + hh * in_pad;
                float a = s_b1[hh];
                for (int i = 0; i < in_dim; ++i) a = __builtin_fmaf(wr[i], gin[i], a);
                const float r = fmaxf(a, 0.0f);
                for (int o = 0; o < NOUT; ++o) out[o] = __builtin_fmaf(s_w2[o * H + hh], r, out[o]);
                ga[hh] = a > 0.0f ? 1.0f : 0.0f;        // the relu mask; finished below
                gr[hh] = r;
            }
#pragma unroll
            for (int d = ST_GROUP / 2; d >= 1; d >>= 1)
                for (int o = 0; o < NOUT; ++o) out[o] += __shfl_xor(out[o], d, ST_GROUP);
            // ---- the loss head of sdf_train_kernel with the LOD's weights
            float g[NOUT], sq[NSQ1];
            const float dd = (out[NOUT - 1] + b2[NOUT - 1]) - gts[s];
            g[NOUT - 1] = two_ws * dd * inv_batch;
            sq[0] = dd * dd;
            if constexpr (NOUT == 4) {
                const float two_wc = 2.0f * s_wt[SG_MAX_LODS + my_li];
                float d[3];
                for (int o = 0; o < 3; ++o) {
                    const float co = 1.0f / (1.0f + expf(-(out[o] + b2[o])));
                    d[o] = co - rgb_gts[s * 3 + o];
                    g[o] = two_wc * d[o] * (co * (1.0f - co)) * inv_batch;
                }
                sq[1] = __builtin_fmaf(d[1], d[1], d[0] * d[0]) + d[2] * d[2];
                sq[2] = s_wt[SG_MAX_LODS + my_li] * sq[1] + s_wt[my_li] * sq[0];      // colour + distance, in that order
            } else {
                sq[1] = s_wt[my_li] * sq[0];
            }
            // ---- end of the loss head
            for (int hh = c; hh < H; hh += ST_GROUP) {
                float t = NOUT == 1 ? s_w2[hh] * g[0] : __builtin_fmaf(s_w2[hh], g[0], 0.0f);         // rounding: as sdf_train_kernel
                for (int o = 1; o < NOUT; ++o) t = __builtin_fmaf(s_w2[o * H + hh], g[o], t);
                ga[hh] = ga[hh] != 0.0f ? t : 0.0f;     // the relu's backward selects
                if constexpr (NOUT == 1) gr[hh] *= g[0];
            }
            if (c == 0) {
                for (int o = 0; o < NOUT; ++o) s_g[grp * NOUT + o] = g[o];
                for (int k = 0; k < NSQ1; ++k) s_sq[grp * NSQ1 + k] = sq[k];
            }
        } else if (grp < nrows) {
            for (int hh = c; hh < H; hh += ST_GROUP) { ga[hh] = 0.0f; gr[hh] = 0.0f; }
            if (c < fo) gin[c] = 0.0f;
            gin[fo + c] = 0.0f;
            if (c < NOUT) s_g[grp * NOUT + c] = 0.0f;
            if (c < NSQ1) s_sq[grp * NSQ1 + c] = 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
        if (live) {
            float dx = 0.0f;                                              // d loss / d x_k, feature columns only
            for (int hh = 0; hh < H; ++hh) dx = __builtin_fmaf(ga[hh], s_w1[hh * in_pad + fo + c], dx);
            s_df[grp * ST_GROUP + c] = dx;
        }
        __syncthreads();
        // ---- the gradient of level l's blend: every LOD from l on saw it; from k = l, ascending k
        if (live) {
            float suf = s_df[grp * ST_GROUP + c];
            for (int k = my_li + 1; k < NL; ++k) suf += s_df[(grp - my_li + k) * ST_GROUP + c];
            dfeat[(s * NL + my_li) * C + c] = suf;
            const uint32_t b = __float_as_uint(wm1 * fabsf(suf)) & 0x7fffffffu;
            const uint32_t nb = (!(suf == suf) || !(wm1 == wm1)) ? 0x7fc00000u : b;
            mbits = nb > mbits ? nb : mbits;
        }
        // ---- phase 3: the thread that owns an entry adds the rows up in ascending q = si L + k
        for (int e = threadIdx.x; e < lay.entries; e += blockDim.x) {
            float acc = 0.0f;
            if (e < lay.e_b1) {
                const int hh = e / in_dim, i = e - hh * in_dim;
                for (int q = 0; q < nrows; ++q) acc = __builtin_fmaf(s_ga[q * H + hh], s_in[q * in_dim + i], acc);
            } else if (e < lay.e_w2) {
                const int hh = e - lay.e_b1;
                for (int q = 0; q < nrows; ++q) acc += s_ga[q * H + hh];
            } else if (e < lay.e_b2) {
                const int o = NOUT == 1 ? 0 : (e - lay.e_w2) / H, hh = (e - lay.e_w2) - o * H;        // rounding: as sdf_train_kernel
                for (int q = 0; q < nrows; ++q)
                    acc = NOUT == 1 ? acc + s_r[q * H + hh] : __builtin_fmaf(s_g[q * NOUT + o], s_r[q * H + hh], acc);
            } else if (e < lay.e_sq) {
                for (int q = 0; q < nrows; ++q) acc += s_g[q * NOUT + (e - lay.e_b2)];
            } else if (e < lay.e_tot) {                                   // S_k, then R_k: the rows of LOD k in sample order
                const int j = (e - lay.e_sq) / NL, k = (e - lay.e_sq) - j * NL;
                for (int si = 0; si < spb; ++si) acc += s_sq[(si * NL + k) * NSQ1 + j];
            } else {
                for (int q = 0; q < nrows; ++q) acc += s_sq[q * NSQ1 + NSQ];
            }
            s_own[e] += acc;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < lay.entries; e += blockDim.x) partials[(int64_t)blockIdx.x * lay.row_stride + e] = s_own[e];
    mbits = sg_wave_umax(mbits);
    if ((threadIdx.x & 63) == 0 && mbits > __atomic_load_n(&hdr->absmax_bits, __ATOMIC_RELAXED)) atomicMax(&hdr->absmax_bits, mbits);
}

__global__ void __launch_bounds__(256)
sdf_lods_train_reduce_kernel(const float* __restrict__ partials, int rows, int H, int in_dim, int n_out, int num_lods,
                             float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2,
                             float* __restrict__ loss, float inv_batch) {
    // sdf_train_reduce_kernel over the all-LOD row: 16 lanes per entry, lane r adds rows r, r + 16, ... in order, then a butterfly
    const StLodsLayout lay = st_lods_layout(H, in_dim, n_out, num_lods);
    const int r0 = threadIdx.x & 15;
    for (int e = blockIdx.x * 16 + (threadIdx.x >> 4); e < lay.entries + 15; e += gridDim.x * 16) {
        const bool in = e < lay.entries;
        float acc = 0.0f;
        if (in)
            for (int r = r0; r < rows; r += 16) acc += partials[(int64_t)r * lay.row_stride + e];
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 16);
        if (!in || r0 != 0) continue;
        if (e < lay.e_b1) gw1[e] += acc;
        else if (e < lay.e_w2) gb1[e - lay.e_b1] += acc;
        else if (e < lay.e_b2) gw2[e - lay.e_w2] += acc;
        else if (e < lay.e_sq) gb2[e - lay.e_b2] += acc;
        else if (e == lay.e_tot) loss[0] = acc * inv_batch;
        else loss[1 + (e - lay.e_sq)] = acc;            // S_k at 1 + k, R_k at 1 + L + k, un-normalised
    }
}

template <int NOUT>
static int st_lods_step(const char* who, const float* coords, const float* gts, const float* rgb_gts, int64_t n, const uint8_t* octree,
                        const int32_t* exsum, const int16_t* points, const int32_t* trinkets, const float* const* feats,
                        const int32_t* levels, const int64_t* rows, int num_lods, int channels, int half_round, int pos_input,
                        const float* w_sdf, const float* w_rgb, const float* w1, const float* b1, const float* w2, const float* b2,
                        int hidden, float* const* grad_feats, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2,
                        float* loss, void* scratch, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    StField fld;
    StLodW wt;
    SgLods ml;
    if (sg_fill(ml, levels, rows, num_lods) != 0) return wisp_fail(WISP_ERR_INVALID, who, "bad level or row count");
    for (int l = 0; l < SG_MAX_LODS; ++l) { wt.sdf[l] = 1.0f; wt.rgb[l] = 1.0f; }
    for (int l = 0; l < num_lods; ++l) {
        if (!(feats[l] && grad_feats[l] && (l == 0 || levels[l] > levels[l - 1]))) return wisp_fail(WISP_ERR_INVALID, who, "bad level list");
        fld.feats[l] = feats[l]; fld.level[l] = levels[l]; ml.grad[l] = grad_feats[l];
        wt.sdf[l] = w_sdf[l];
        if (NOUT == 4) wt.rgb[l] = w_rgb[l];
        if (!(std::isfinite(wt.sdf[l]) && wt.sdf[l] > 0.0f && std::isfinite(wt.rgb[l]) && wt.rgb[l] > 0.0f))
            return wisp_fail(WISP_ERR_INVALID, who, "the LOD weights must be finite and > 0");
    }
    fld.num_lods = num_lods; fld.channels = channels; fld.half_round = half_round; fld.hidden = hidden;
    fld.max_level = levels[num_lods - 1]; fld.pos_input = pos_input;
    fld.w1 = w1; fld.b1 = b1; fld.w2 = w2; fld.b2 = b2;
    const SgPlan pl = sg_plan(ml.base[num_lods], channels, 0);
    if (workspace_bytes < pl.bytes) return wisp_fail(WISP_ERR_INVALID, who, "workspace too small (wisp_spc_bwd_workspace_bytes)");
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    SgHeader* hdr = reinterpret_cast<SgHeader*>(ws);
    const int in_dim = (pos_input ? 3 : 0) + channels;
    const int grid = st_grid(n, num_lods);
    const StLodsLayout lay = st_lods_layout(hidden, in_dim, NOUT, num_lods);
    float* partials = static_cast<float*>(scratch);
    float* dfeat = partials + (size_t)grid * lay.row_stride;
    int64_t* chain = reinterpret_cast<int64_t*>(reinterpret_cast<unsigned char*>(dfeat) + sg_round64(n * num_lods * channels * 4));
    const size_t lds = (size_t)lay.floats * sizeof(float);
    const float inv_batch = 1.0f / (float)n;
    if (hipMemsetAsync(hdr, 0, sizeof(SgHeader), s) != hipSuccess) return wisp_fail(WISP_ERR_LAUNCH, who, "hipMemsetAsync failed");
    if (const hipError_t e = WISP_ALLOW_LDS(sdf_lods_train_kernel<NOUT>, lds)) return wisp_fail(WISP_ERR_LAUNCH, who, hipGetErrorString(e));
    hipLaunchKernelGGL(sdf_lods_train_kernel<NOUT>, dim3(grid), dim3(ST_GROUP * ST_GROUPS), lds, s, coords, gts, rgb_gts, n, octree,
                       exsum, points, trinkets, fld, wt, inv_batch, partials, dfeat, chain, hdr);
    hipLaunchKernelGGL(sdf_lods_train_reduce_kernel, dim3((lay.entries + 15) / 16), dim3(256), 0, s, partials, grid, hidden, in_dim,
                       NOUT, num_lods, grad_w1, grad_b1, grad_w2, grad_b2, loss, inv_batch);
    // the corner sums: one column block per level ('cat' columns, sum = 0); the magnitude bound is in the header already
    const SgCall c{coords, chain, 1, num_lods, 1, points, trinkets, dfeat, n, num_lods, channels, 0, channels};
    sg_scatter(c, ml, pl, ws, s, true);
    sg_finalize(c, ml, pl, ws, s);
    if (const hipError_t e = hipGetLastError()) return wisp_fail(WISP_ERR_LAUNCH, who, hipGetErrorString(e));
    return WISP_OK;
}

extern "C" int64_t wisp_sdf_lods_train_scratch_bytes(int64_t n, int num_lods, int channels, int hidden, int n_out, int pos_input) {
    if (n < 0 || num_lods < 1 || num_lods > SG_MAX_LODS || channels != ST_GROUP || hidden < 1 || hidden > ST_MAX_HIDDEN ||
        (n_out != 1 && n_out != 4) || (pos_input != 0 && pos_input != 1) || (n_out == 1 && pos_input != 1))
        return -1;
    return st_lods_scratch_bytes(n, num_lods, channels, hidden, (pos_input ? 3 : 0) + channels, n_out);
}

extern "C" int wisp_sdf_lods_train_step(const float* coords, const float* gts, const float* rgb_gts, int64_t n, const uint8_t* octree,
                                        const int32_t* exsum, const int16_t* points, const int32_t* trinkets,
                                        const float* const* feats, const int32_t* levels, const int64_t* rows, int num_lods,
                                        int channels, int half_round, int n_out, int pos_input, const float* w_sdf,
                                        const float* w_rgb, const float* w1, const float* b1, const float* w2, const float* b2,
                                        int hidden, float* const* grad_feats, float* grad_w1, float* grad_b1, float* grad_w2,
                                        float* grad_b2, float* loss, void* scratch, int64_t scratch_bytes, void* workspace,
                                        int64_t workspace_bytes, wisp_stream_t stream) {
    WISP_REQUIRE(n >= 1 && num_lods >= 1 && num_lods <= SG_MAX_LODS, "bad sizes");
    WISP_REQUIRE(channels == ST_GROUP, "the fused all-LOD SDF step is built for 16 feature channels (nglod_octree.yaml)");
    WISP_REQUIRE(hidden >= 1 && hidden <= ST_MAX_HIDDEN, "hidden width out of range");
    WISP_REQUIRE(n_out == 1 || n_out == 4, "n_out must be 1 or 4");
    WISP_REQUIRE(pos_input == 0 || pos_input == 1, "pos_input must be 0 or 1");
    WISP_REQUIRE(n_out == 4 || pos_input == 1, "a one-output field takes the position (pos_input must be 1)");
    WISP_REQUIRE(coords && gts && octree && exsum && points && trinkets && feats && levels && rows && w_sdf && w1 && b1 && w2 && b2 &&
                 grad_feats && grad_w1 && grad_b1 && grad_w2 && grad_b2 && loss && scratch && workspace, "null pointer");
    WISP_REQUIRE((n_out == 4) == (rgb_gts != nullptr) && (n_out == 4) == (w_rgb != nullptr),
                 "rgb_gts and w_rgb go with four outputs and with them only");
    WISP_REQUIRE(scratch_bytes >= wisp_sdf_lods_train_scratch_bytes(n, num_lods, channels, hidden, n_out, pos_input),
                 "scratch too small (wisp_sdf_lods_train_scratch_bytes)");
    if (n_out == 1)
        return st_lods_step<1>(__func__, coords, gts, nullptr, n, octree, exsum, points, trinkets, feats, levels, rows, num_lods,
                               channels, half_round, 1, w_sdf, nullptr, w1, b1, w2, b2, hidden, grad_feats, grad_w1, grad_b1, grad_w2,
                               grad_b2, loss, scratch, workspace, workspace_bytes, (hipStream_t)stream);
    return st_lods_step<4>(__func__, coords, gts, rgb_gts, n, octree, exsum, points, trinkets, feats, levels, rows, num_lods, channels,
                           half_round, pos_input, w_sdf, w_rgb, w1, b1, w2, b2, hidden, grad_feats, grad_w1, grad_b1, grad_w2, grad_b2,
                           loss, scratch, workspace, workspace_bytes, (hipStream_t)stream);
}
