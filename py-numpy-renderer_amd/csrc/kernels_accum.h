// kernels_accum.h -- the accumulation: a weighted sum of float frames on the sample grid, finalised once.
//
//   A_0 = w_0 * F_0,   A_k = A_{k-1} + (w_k * F_k)           k_accum_add, one launch per sub-frame
//   M   = ss_block_mean(A),  R = min(M * scale, 1),  out = gamma_u8(R), rows flipped        k_accum_resolve
//
// float32 throughout, every operation rounded on its own (the build's -ffp-contract=off keeps the product and the add
// of k_accum_add apart); host_accum.h restates both on the host, bit for bit.
//
// Compiled in accum.hip, a translation unit and a code object of their own: a kernel added to mi355rast.hip's code
// object moves k_setup and k_tile to other addresses, which c4 showed as 0.4 % of a frame (profiles/accumulate_time.txt).
#pragma once

#include "kernels_shade.h"      // gamma_u8
#include "rast_resolve.h"       // ss_block_mean

namespace mr {

constexpr int ACCUM_BLOCK = 256;
constexpr unsigned ACCUM_MAX_BLOCKS = 2048;      // a memory-bound stream: a capped grid and a grid-stride loop

// acc = w * frame (first: acc is written without being read, so it needs no memset), else acc += w * frame.  Both
// buffers are DevBuf allocations (256-byte aligned): 16 bytes per lane and access, a scalar tail for n_floats % 4.
// Plain loads and stores: the sum is read again one sub-frame later and is left to the caches.
__global__ void __launch_bounds__(ACCUM_BLOCK)
k_accum_add(const float *__restrict__ frame, float *__restrict__ acc, size_t n_floats, float w, int first)
{
    const size_t n4 = n_floats / 4, stride = (size_t)gridDim.x * ACCUM_BLOCK;
    const size_t lane = (size_t)blockIdx.x * ACCUM_BLOCK + threadIdx.x;
    const float4 *f4 = reinterpret_cast<const float4 *>(frame);
    float4 *a4 = reinterpret_cast<float4 *>(acc);
    for (size_t i = lane; i < n4; i += stride) {
        const float4 f = f4[i];
        float4 a = make_float4(w * f.x, w * f.y, w * f.z, w * f.w);
        if (!first) {
            const float4 o = a4[i];
            a.x = o.x + a.x; a.y = o.y + a.y; a.z = o.z + a.z; a.w = o.w + a.w;
        }
        a4[i] = a;
    }
    const size_t t = n4 * 4 + lane;
    if (t < n_floats) {
        const float p = w * frame[t];
        acc[t] = first ? p : acc[t] + p;
    }
}

// One thread per output pixel, shaped like k_resolve_full: the block's mean in the order every resolve of the tree
// sums it, the scale, the clamp, the gamma step.  acc is (height, width, 3) on the sample grid, rows bottom-up; out is
// (height >> shift, width >> shift, 3), row 0 = top.
__global__ void __launch_bounds__(256)
k_accum_resolve(const float *__restrict__ acc, int width, int height, int shift, float scale,
                const float *__restrict__ gamma_lut, uint8_t *__restrict__ out)
{
    const int ow = width >> shift, oh = height >> shift;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)ow * oh) return;
    const int orow = (int)(i / ow), ox = (int)(i - (long long)orow * ow);
    const int py = height - ((orow + 1) << shift), px = ox << shift;
    float m[3];
    ss_block_mean(acc + ((size_t)py * width + px) * 3, width * 3, shift, m);
    uint8_t *o = out + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = m[c] * scale;
        o[c] = gamma_u8(r < 1.0f ? r : 1.0f, gamma_lut);
    }
}

}  // namespace mr
