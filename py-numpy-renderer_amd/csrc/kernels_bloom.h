// kernels_bloom.h -- k_bloom_down, k_bloom_up, k_bloom_composite: bloom from a resolution pyramid (bloom_def.h has the
// definition).  A frame with L levels runs 2 L dependent launches: L of k_bloom_down (the first applies the bright pass
// while it stages, so B0 is never written to memory), L - 1 of k_bloom_up, one k_bloom_composite.
//
// k_bloom_down: a workgroup of 256 threads owns TW x TH output samples, one a thread.  It stages its source rectangle --
// (2 TW + 2) x (2 TH + 2) samples, coordinates clamped to the source level -- in LDS ONCE, a sample a lane, as three
// planes (one a channel): consecutive lanes write consecutive words of a plane, and a thread's four taps of a row are two
// aligned 8-byte reads, (2 lx, 2 lx + 1) and (2 lx + 2, 2 lx + 3), whose 32 lanes cover the 64 banks of ds_read_b64 once.
// (Three floats a sample as they lie in memory would put lanes l and l + 16 on one bank: a stride of six words.)
// The LDS a workgroup takes is (2 TW + 2) * (2 TH + 2) * 12 bytes:
//
//   shape 0    32 x  8 samples, 256 threads    14 256 bytes
//   shape 1    64 x  4 samples, 256 threads    15 600 bytes
//   shape 2    16 x 16 samples, 256 threads    13 872 bytes
//
// At most 16 KB a workgroup: ten fit a CU's 160 KB, more waves than its four SIMDs hold.
//
// k_bloom_up and k_bloom_composite stage nothing: a fine sample reads four coarse taps a channel, its neighbour the same
// four or the next ones, and the coarse level is a quarter of the fine one -- the taps come out of the caches, and the
// traffic that reaches memory is the fine level's own 12 bytes in and 12 out (DESIGN.md 6n has the measurement).  Both write
// in place: a thread reads the fine buffer at its own sample only, and the coarse level is another buffer.
//
// No scratch, no atomics, no memset.  Compiled in bloom.hip, a translation unit and a code object of its own, like the
// other passes' kernels: a kernel added to mi355rast.hip's code object moves k_setup and k_tile to other addresses
// (kernels_accum.h).
#pragma once

#include "bloom_def.h"

namespace mr {

constexpr int bloom_lds_bytes(int tw, int th) { return (2 * tw + 2) * (2 * th + 2) * 3 * (int)sizeof(float); }

constexpr int BLOOM_UP_TW = 64, BLOOM_UP_TH = 4;      // the workgroup of k_bloom_up and k_bloom_composite, a sample a thread

// src: level l - 1 (sh x sw), or the float frame where FIRST; dst: level l (dh x dw) = (bloom_half(sh), bloom_half(sw))
template <bool FIRST, int TW, int TH, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_bloom_down(const float *__restrict__ src, float *__restrict__ dst, int sw, int sh, int dw, int dh, float threshold)
{
    constexpr int LW = 2 * TW + 2, LH = 2 * TH + 2, PLANE = LW * LH;
    static_assert(TW * TH == BLOCK && BLOCK % 64 == 0, "one sample a thread");
    static_assert(LW % 2 == 0 && PLANE % 2 == 0, "the taps are read as aligned pairs");
    __shared__ __attribute__((aligned(16))) float s_f[3 * PLANE];
    static_assert(sizeof(s_f) == (size_t)bloom_lds_bytes(TW, TH), "the LDS this header states");
    const int x0 = (int)blockIdx.x * TW, y0 = (int)blockIdx.y * TH, tid = (int)threadIdx.x;

    // ---- 1. the source rectangle, a sample a lane; outside the level: the nearest sample's
    for (int i = tid; i < PLANE; i += BLOCK) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = min(max(2 * x0 - 1 + lx, 0), sw - 1), gy = min(max(2 * y0 - 1 + ly, 0), sh - 1);
        const float *q = src + ((size_t)gy * sw + gx) * 3;
        float r = q[0], g = q[1], b = q[2];
        if (FIRST) {
            const float k = bloom_bright(r, g, b, threshold);
            r = r * k; g = g * k; b = b * k;
        }
        s_f[i] = r; s_f[PLANE + i] = g; s_f[2 * PLANE + i] = b;
    }
    __syncthreads();

    const int ly = tid / TW, lx = tid - ly * TW;
    const int gx = x0 + lx, gy = y0 + ly;
    if (gx >= dw || gy >= dh) return;                          // (behind the barrier)
    float *o = dst + ((size_t)gy * dw + gx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 *row = reinterpret_cast<const float2 *>(s_f + c * PLANE + (2 * ly + j) * LW + 2 * lx);
            const float2 a = row[0], b = row[1];
            r[j] = bloom_down4(a.x, a.y, b.x, b.y);
        }
        o[c] = bloom_down_scale(bloom_down4(r[0], r[1], r[2], r[3]));
    }
}

// up(C) at fine sample (x, y): C is the coarse level (ch x cw), three floats a sample
__device__ inline void bloom_up_at(const float *__restrict__ coarse, int cw, int ch, int x, int y, float u[3])
{
    const int nx = x >> 1, ny = y >> 1, fx = bloom_far(x, cw), fy = bloom_far(y, ch);
    const float *rn = coarse + (size_t)ny * cw * 3, *rf = coarse + (size_t)fy * cw * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = bloom_up(rn[nx * 3 + c], rn[fx * 3 + c], rf[nx * 3 + c], rf[fx * 3 + c]);
}

// fine (h x w) holds D_l and receives U_l = D_l + up(U_{l+1}); coarse is U_{l+1}, (bloom_half(h) x bloom_half(w))
__global__ void __launch_bounds__(BLOOM_UP_TW * BLOOM_UP_TH)
k_bloom_up(float *__restrict__ fine, const float *__restrict__ coarse, int w, int h, int cw, int ch)
{
    const int x = (int)blockIdx.x * BLOOM_UP_TW + (int)threadIdx.x % BLOOM_UP_TW, y = (int)blockIdx.y * BLOOM_UP_TH + (int)threadIdx.x / BLOOM_UP_TW;
    if (x >= w || y >= h) return;
    float u[3];
    bloom_up_at(coarse, cw, ch, x, y, u);
    float *o = fine + ((size_t)y * w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = o[c] + u[c];
}

// frame (h x w) receives F + g * up(U_1); coarse is U_1
__global__ void __launch_bounds__(BLOOM_UP_TW * BLOOM_UP_TH)
k_bloom_composite(float *__restrict__ frame, const float *__restrict__ coarse, int w, int h, int cw, int ch, float gain)
{
    const int x = (int)blockIdx.x * BLOOM_UP_TW + (int)threadIdx.x % BLOOM_UP_TW, y = (int)blockIdx.y * BLOOM_UP_TH + (int)threadIdx.x / BLOOM_UP_TW;
    if (x >= w || y >= h) return;
    float u[3];
    bloom_up_at(coarse, cw, ch, x, y, u);
    float *o = frame + ((size_t)y * w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = bloom_composite(o[c], gain, u[c]);
}

}  // namespace mr
