// The three evaluation kernels of an SDF field over an arbitrary-position encoder, written once as __device__ bodies: the signed
// distance at arbitrary points with the intersection-over-union counters of a validation batch, central-difference normals, and
// one marching iteration of PackedSDFTracer including the field query.  hash_sdf_eval.hip and triplane_sdf_eval.hip wrap them in
// their __global__ kernels.  E is the encoder policy (HashSdfEnc<T>, TriSdfEnc): E::Field holds the encoder's parameters and a
// SdfDecoder `dec`, E::point_inputs writes a group's decoder inputs, E::group_floats is a group's share of LDS.
#pragma once
#include "wisp_common.h"
#include "sdf_decoder_dev.h"
#include "sphere_trace_dev.h"

#define SDF_POINT_BLOCK 256
#define SDF_POINT_GROUPS (SDF_POINT_BLOCK / SDF_GROUP)

// A group either runs the whole function or none of it (the shuffles stay inside the group).
template <class E>
static __device__ __forceinline__ float sdf_eval_point(const typename E::Field& fld, const SdfDecoderLds& s, float* gin, int c,
                                                       float px, float py, float pz) {
    E::point_inputs(fld, gin, c, px, py, pz);
    return sdf_decode<false>(fld.dec, s, gin, c, nullptr, nullptr);
}

// out [n, 1] (optional), counts {intersection, union} of (pred < 0) and (gt < 0) (optional).  Grid-stride over rounds of 16
// points: the block stages the weights once.
template <class E>
static __device__ __forceinline__ void sdf_point_query_body(const float* __restrict__ coords, int64_t n, const typename E::Field& fld,
                                                            float* __restrict__ out, const float* __restrict__ gts,
                                                            unsigned long long* __restrict__ counts) {
    extern __shared__ float s_sdf_point[];
    const SdfDecoderLds s = sdf_decoder_stage(s_sdf_point, fld.dec, E::group_floats(fld));
    const int c = threadIdx.x & (SDF_GROUP - 1), grp = threadIdx.x / SDF_GROUP;
    float* gin = s.in + grp * s.stride;
    const int64_t rounds = (n + SDF_POINT_GROUPS - 1) / SDF_POINT_GROUPS;
    unsigned int both = 0, either = 0;                   // wave-uniform; a wave sees 4 points a round: no overflow below 2^30 rounds
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * SDF_POINT_GROUPS + grp;
        const bool live = i < n;                         // dead groups evaluate the origin: every lane stays in the ballots
        const float px = live ? coords[i * 3] : 0.0f, py = live ? coords[i * 3 + 1] : 0.0f, pz = live ? coords[i * 3 + 2] : 0.0f;
        const float o = sdf_eval_point<E>(fld, s, gin, c, px, py, pz);
        if (out && live && c == 0) out[i] = o;
        if (counts) {
            const bool mine = live && c == 0;
            const bool pin = mine && o < 0.0f;
            const bool gt_in = mine && gts[i] < 0.0f;
            both += __popcll(__ballot(pin && gt_in));
            either += __popcll(__ballot(pin || gt_in));
        }
    }
    if (counts && (threadIdx.x & (WISP_WAVE - 1)) == 0) {      // one lane per wave, one add per counter
        if (both) atomicAdd(counts, (unsigned long long)both);
        if (either) atomicAdd(counts + 1, (unsigned long long)either);
    }
}

// grad[i, a] = (f(x + eps e_a) - f(x - eps e_a)) / (2 eps): finitediff_gradient in one launch.  The six positions are formed in
// fp32 as torch forms x + offs[a] / x - offs[a]; every value comes from sdf_eval_point.
template <class E>
static __device__ __forceinline__ void sdf_point_gradient_body(const float* __restrict__ coords, int64_t n, const typename E::Field& fld,
                                                               float eps, float* __restrict__ grad) {
#pragma clang fp contract(off)
    extern __shared__ float s_sdf_point[];
    const SdfDecoderLds s = sdf_decoder_stage(s_sdf_point, fld.dec, E::group_floats(fld));
    const int c = threadIdx.x & (SDF_GROUP - 1), grp = threadIdx.x / SDF_GROUP;
    float* gin = s.in + grp * s.stride;
    const int64_t rounds = (n + SDF_POINT_GROUPS - 1) / SDF_POINT_GROUPS;
    const float two_eps = 2.0f * eps;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t i = rd * SDF_POINT_GROUPS + grp;
        const bool live = i < n;
        const float x0 = live ? coords[i * 3] : 0.0f, x1 = live ? coords[i * 3 + 1] : 0.0f, x2 = live ? coords[i * 3 + 2] : 0.0f;
        float mine = 0.0f;
#pragma unroll 1
        for (int a = 0; a < 3; ++a) {
            const float ep = (a == 0 ? x0 : a == 1 ? x1 : x2) + eps, em = (a == 0 ? x0 : a == 1 ? x1 : x2) - eps;
            const float fp = sdf_eval_point<E>(fld, s, gin, c, a == 0 ? ep : x0, a == 1 ? ep : x1, a == 2 ? ep : x2);
            const float fm = sdf_eval_point<E>(fld, s, gin, c, a == 0 ? em : x0, a == 1 ? em : x1, a == 2 ? em : x2);
            const float g = (fp - fm) / two_eps;
            if (c == a) mine = g;
        }
        if (live && c < 3) grad[i * 3 + c] = mine;
    }
}

// One marching iteration of PackedSDFTracer.trace (wisp/tracers/packed_sdf_tracer.py:118-146) including the field query
// nef(coords=x, channels="sdf").  16 lanes own one pack: all 16 run the (pack-uniform) bookkeeping of sphere_trace_step
// (sphere_trace_dev.h), lane 0 stores the state, and the packs still marching evaluate the field at the new position.  A group
// leaves as a whole, so nothing below the exits is wave-wide.
template <class E>
static __device__ __forceinline__ void sdf_march_body(const SphereTraceState& st, int first, const typename E::Field& fld, float scale,
                                                      int32_t* __restrict__ any_active) {
#pragma clang fp contract(off)
    extern __shared__ float s_sdf_point[];
    const SdfDecoderLds s = sdf_decoder_stage(s_sdf_point, fld.dec, E::group_floats(fld));
    const int c = threadIdx.x & (SDF_GROUP - 1), grp = threadIdx.x / SDF_GROUP;
    const int64_t p = (int64_t)blockIdx.x * SDF_POINT_GROUPS + grp;
    if (p >= st.num_packs) return;
    float px, py, pz;
    bool m;
    if (first) {
        m = st.mask[p] != 0;
        px = st.x[p * 3]; py = st.x[p * 3 + 1]; pz = st.x[p * 3 + 2];
    } else {
        m = sphere_trace_step(st, p, c == 0, px, py, pz);
    }
    if (!m) return;
    if (c == 0 && any_active) atomicAdd(any_active, 1);
    const float o = sdf_eval_point<E>(fld, s, s.in + grp * s.stride, c, px, py, pz);
    if (c == 0) st.dist[p] = o * scale;
}

// ---------------------------------------------------------------------------------------------------- host side
// dynamic LDS of the three kernels
template <class E> static inline size_t sdf_point_lds(const typename E::Field& fld) {
    return sdf_decoder_lds_bytes(fld.dec.hidden, fld.dec.cols, E::group_floats(fld), SDF_POINT_GROUPS);
}

// enough blocks to fill the chip several times over, few enough that staging the weights (<= 53 KB) stays a small share
static inline unsigned sdf_point_grid(int64_t n) { return (unsigned)min64(ceil_div64(n, SDF_POINT_GROUPS), 2048); }
