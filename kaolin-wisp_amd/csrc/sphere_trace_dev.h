// The bookkeeping of one marching iteration of PackedSDFTracer.trace (wisp/tracers/packed_sdf_tracer.py:118-146) as one
// __device__ function: advance t by the last distance, convergence tests, far-plane test, nugget search (find_depth_bound
// with its bounds quirks, csrc/render.hip), jump to the next cell's entry, and the new query position.  Everything but the
// field query.  Shared by sphere_trace_step_kernel (csrc/render.hip: one thread per pack, the query is the caller's),
// sdf_trace_fused_kernel (csrc/sdf_eval.hip) and hash_sdf_march_kernel (csrc/hash_sdf_eval.hip: 16 lanes per pack, the query
// follows in the same launch), so that a fused march and step + query hold the same state bit for bit.
#pragma once
#include "wisp_common.h"

// State per pack p (= ray with at least one nugget), all updated in place except curr_idx, which is double-buffered because
// pack p reads pack p+1's PREVIOUS index as its search bound.  The step reads dist; the fused kernels store the query through it.
struct SphereTraceState {
    int64_t num_packs;
    const float *nug_o, *nug_d, *nug_depth;   // [P,3], [P,3], [nuggets,2] entry / exit
    const int32_t* nug_pidx;
    float dist_max, thr_close, thr_avg;        // thr_close = min_dis, thr_avg = 5 min_dis
    float *t, *dist, *dist_prev;
    uint8_t *mask, *hit;
    const int32_t* curr_in;
    int32_t* curr_out;
    int64_t* curr_pidx;
    float* x;                                  // [P,3]
};

static inline bool sphere_trace_state_complete(const SphereTraceState& s) {
    return s.nug_o && s.nug_d && s.nug_depth && s.nug_pidx && s.t && s.dist && s.dist_prev && s.mask && s.hit && s.curr_in &&
           s.curr_out && s.curr_pidx && s.x;
}

// Pack p < num_packs.  Returns whether the pack still marches, and its new position in (px, py, pz).  `store`: this lane writes
// the state - the pack's one thread, or lane 0 of the 16 that run these (pack-uniform) statements together.
static __device__ __forceinline__ bool sphere_trace_step(const SphereTraceState& s, int64_t p, bool store, float& px, float& py,
                                                         float& pz) {
#pragma clang fp contract(off)
    const int32_t cur = s.curr_in[p];
    bool m = s.mask[p] != 0;
    const bool was = m;
    bool h = s.hit[p] != 0;
    const float dd = s.dist[p];
    float tt = s.t[p] + dd;                                                      // t += dist          (:120)
    if (m) {
        h = fabsf(dd) < s.thr_close;                                             // :122
        h = h || (fabsf(dd + s.dist_prev[p]) * 0.5f < s.thr_avg);                // :123-124
        m = tt < s.dist_max;                                                     // :125
    }
    m = m && !h;                                                                 // :126
    const float dprev = dd;
    int32_t nxt = -1;
    if (cur > -1) {                                                              // find_depth_bound (:131)
        uint32_t i = (uint32_t)cur;
        const uint32_t stop = (p == s.num_packs - 1) ? (uint32_t)s.num_packs : (uint32_t)s.curr_in[p + 1];
        while (i < stop) {
            const float entry = s.nug_depth[2 * (int64_t)i], exit_ = s.nug_depth[2 * (int64_t)i + 1];
            if ((tt >= entry && tt <= exit_) || tt < entry) { nxt = (int32_t)i; break; }
            ++i;
        }
    }
    const bool keep_prev = m;                                                    // :129 runs before :132
    m = m && (nxt != -1);                                                        // :132
    const bool jumped = nxt != cur;                                              // :133
    const int32_t now = m ? nxt : cur;                                           // :134
    if (m && jumped) tt = s.nug_depth[2 * (int64_t)now];                         // :136
    px = s.nug_o[p * 3 + 0] + s.nug_d[p * 3 + 0] * tt;                           // :137-139 / :121
    py = s.nug_o[p * 3 + 1] + s.nug_d[p * 3 + 1] * tt;
    pz = s.nug_o[p * 3 + 2] + s.nug_d[p * 3 + 2] * tt;
    if (store) {
        if (keep_prev) s.dist_prev[p] = dprev;
        // (a ray deactivated in this step still gets x at the advanced t: :121 ran before the tests)
        if (m || was) { s.x[p * 3 + 0] = px; s.x[p * 3 + 1] = py; s.x[p * 3 + 2] = pz; }
        if (m) s.curr_pidx[p] = (int64_t)s.nug_pidx[now];
        s.t[p] = tt;
        s.mask[p] = m ? 1 : 0;
        s.hit[p] = h ? 1 : 0;
        s.curr_out[p] = now;
    }
    return m;
}
