// rast_resolve.h -- the mean of one s x s block of samples, in the ONE order every resolve of the tree sums it
// (kernels_tile.h: the fused resolve, k_resolve_touched, k_resolve_full; kernels_accum.h: k_accum_resolve).
#pragma once

#include <hip/hip_runtime.h>

namespace mr {

// mean of the block whose bottom-left sample is rgb[0]; rows `row` floats apart, samples 3 floats apart
__device__ __forceinline__ void ss_block_mean(const float *rgb, int row, int shift, float m[3])
{
    const int s = 1 << shift;
    float acc[3] = { 0.f, 0.f, 0.f };
    for (int j = 0; j < s; ++j)
        for (int i = 0; i < s; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += rgb[j * row + i * 3 + c];
        }
    const float inv = 1.0f / (float)(s * s);       // a power of two: exact, and a uniform block keeps its colour
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = acc[c] * inv;
}

}  // namespace mr
