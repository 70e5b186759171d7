// F.grid_sample's source coordinate for align_corners=True + padding_mode='reflection', shared by the triplanar feature
// pyramid (spc_interp.hip) and the texture lookup (mesh_tex.hip).
#pragma once
#include "wisp_common.h"

// unnormalise g in [-1, 1] to [0, size-1], reflect into that range (period 2 * (size-1)), clip.  size == 1: the span is 0 and
// the coordinate is 0.  The result lies in [0, size-1] for every input, a NaN included (fmaxf drops it).  Host-callable too, so
// that a CPU program can run the code under test.
static __host__ __device__ __forceinline__ float wisp_reflect_source_index(float g, int size) {
    float x = (g + 1.0f) * 0.5f * (float)(size - 1);
    const float span = (float)(size - 1);
    if (span <= 0.0f) return 0.0f;
    x = fabsf(x);
    const float flips = floorf(x / span);
    const float extra = x - flips * span;                 // fmod(x, span)
    x = (((int)fminf(flips, 2147483520.0f)) & 1) ? span - extra : extra;   // (bounded: the cast is defined for every input)
    return fminf(fmaxf(x, 0.0f), span);
}
