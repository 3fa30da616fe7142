// kernels_taa.h -- k_taa: temporal anti-aliasing (taa_def.h has the definition), a frame's float colours blended into the
// history fetched where every sample's surface point was, written to a second float frame and to the scene's new history.
//
// A workgroup of BLOCK = TW x TH threads owns TW x TH samples, one a thread.  It stages F for its rectangle and a halo of
// one sample round it in LDS, ONCE, as it lies in memory: three floats a sample, coordinates clamped to the frame, so the
// definition's clamped neighbourhood is nine plain LDS reads a channel (a stride of three floats from lane to lane: no
// two lanes of a half-wavefront share a bank).  The LDS a workgroup takes is (TW + 2) * (TH + 2) * 12 bytes:
//
//   shape 0    32 x  8 samples, 256 threads     4 080 bytes
//   shape 1    64 x  4 samples, 256 threads     4 752 bytes
//   shape 2    16 x 16 samples, 256 threads     3 888 bytes
//
// U is read once per sample (8 bytes); the four history taps go through the caches -- neighbouring samples move alike, so
// neighbouring lanes fetch neighbouring texels.  The result is written twice, to `out` and to `hist_out`: neither is
// `frame` or `hist`, whose other samples are still being read.  The kernel is a stream: about 12 bytes of F, 8 of U and 12
// of P read and 24 written per sample, against a few dozen float operations.  No scratch, no atomics, no memset.
//
// Compiled in taa.hip, a translation unit and a code object of its own, like the other passes' kernels: a kernel added to
// mi355rast.hip's code object moves k_setup and k_tile to other addresses (kernels_accum.h).
#pragma once

#include "taa_def.h"

namespace mr {

constexpr int taa_lds_bytes(int tw, int th) { return (tw + 2) * (th + 2) * 3 * (int)sizeof(float); }

// hist: the history, or nullptr (no history: out = F)
template <int TW, int TH, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_taa(const float *__restrict__ frame, const float2 *__restrict__ vel, const float *__restrict__ hist, float *__restrict__ out,
      float *__restrict__ hist_out, int width, int height, const TaaParams p)
{
    constexpr int LW = TW + 2, LH = TH + 2, ROW = LW * 3;
    static_assert(TW * TH == BLOCK && BLOCK % 64 == 0, "one sample a thread");
    __shared__ float s_f[LH * ROW];
    static_assert(sizeof(s_f) == (size_t)taa_lds_bytes(TW, TH), "the LDS this header states");
    const int x0 = (int)blockIdx.x * TW, y0 = (int)blockIdx.y * TH, tid = (int)threadIdx.x;

    // ---- 1. F of the rectangle and its halo, float by float in memory order; outside the frame: the nearest sample's
    for (int i = tid; i < LH * ROW; i += BLOCK) {
        const int ly = i / ROW, r = i - ly * ROW;
        const int lx = r / 3, c = r - lx * 3;
        const int gx = min(max(x0 - 1 + lx, 0), width - 1), gy = min(max(y0 - 1 + ly, 0), height - 1);
        s_f[i] = frame[((size_t)gy * width + gx) * 3 + c];
    }
    __syncthreads();

    const int ly = tid / TW, lx = tid - ly * TW;
    const int gx = x0 + lx, gy = y0 + ly;
    if (gx >= width || gy >= height) return;                   // (behind the barrier)
    const size_t g = (size_t)gy * width + gx;
    const int c0 = (ly + 1) * ROW + (lx + 1) * 3;
    float o[3] = { s_f[c0], s_f[c0 + 1], s_f[c0 + 2] };

    // ---- 2. the history where the sample's surface point was, clamped to what the 3 x 3 samples round it show now
    int hx0, hx1, hy0, hy1;
    float fx, fy;
    if (hist != nullptr) {
        const float2 u = vel[g];
        if (taa_target(gx, gy, u.x, u.y, width, height, hx0, hx1, hy0, hy1, fx, fy)) {
            const float *r0 = hist + (size_t)hy0 * width * 3, *r1 = hist + (size_t)hy1 * width * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float h = taa_fetch(r0[hx0 * 3 + c], r0[hx1 * 3 + c], r1[hx0 * 3 + c], r1[hx1 * 3 + c], fx, fy);
                float mn = s_f[c0 - ROW - 3 + c], mx = mn;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const float v = s_f[c0 + dy * ROW + dx * 3 + c];
                        mn = fminf(mn, v); mx = fmaxf(mx, v);
                    }
                o[c] = taa_blend(h, mn, mx, o[c], p.blend);
            }
        }
    }
    float *a = out + g * 3, *b = hist_out + g * 3;
    a[0] = o[0]; a[1] = o[1]; a[2] = o[2];
    b[0] = o[0]; b[1] = o[1]; b[2] = o[2];
}

}  // namespace mr
