// kernels_ao.h -- k_ao: screen-space ambient obscurance (ao_def.h has the definition) applied to a frame's float
// colours in place, from the frame's z-buffer.
//
// A workgroup of BLOCK threads owns TW x TH samples.  It reads the z-buffer of its rectangle and of a halo of
// AO_MAX_RADIUS samples round it ONCE, as float64, and keeps the float32 eye depths in LDS; +inf stands for "outside the
// frame" and for "background", so that a pair's two validity tests are the one comparison of ao_pair.  Every sample then
// reads its sixteen taps from LDS; once all have, the factors take the eye depths' place in LDS (they are held in
// registers across the barrier), and the workgroup multiplies its rows of the float frame, a wavefront to a row: 16
// bytes per lane where the row's address allows (a row of samples starts at a multiple of 12 bytes, not of 16), single
// floats in front of and behind them.  No scratch, no memset, no atomics; nothing but the float frame is written, and a
// sample's three floats are read and written by one workgroup only.
//
// Compiled in ao.hip, a translation unit and a code object of its own, like the accumulation's kernels: a kernel added
// to mi355rast.hip's code object moves k_setup and k_tile to other addresses (kernels_accum.h).
#pragma once

#include "ao_def.h"

namespace mr {

template <int TW, int TH, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_ao(const double *__restrict__ zbuf, float *__restrict__ frame, int width, int height, const AoParams p)
{
    constexpr int R = AO_MAX_RADIUS, LW = TW + 2 * R, LH = TH + 2 * R;
    constexpr int N4_MAX = 3 * TW / 4;                         // float4 pieces of a row of TW samples at the most
    constexpr int PER = TW * TH / BLOCK;                       // samples a thread owns
    static_assert(N4_MAX + 7 <= 64, "a wavefront takes one row: its float4 pieces, then up to 3 + 3 single floats");
    static_assert(PER * BLOCK == TW * TH && BLOCK % 64 == 0, "every thread owns the same number of samples");
    __shared__ float s_e[LH * LW];                             // eye depths; from step 2's second barrier on, the factors in front
    const int x0 = (int)blockIdx.x * TW, y0 = (int)blockIdx.y * TH, tid = (int)threadIdx.x;

    // ---- 1. eye depths of the rectangle and its halo
    for (int i = tid; i < LW * LH; i += BLOCK) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0 - R + lx, gy = y0 - R + ly;
        float e = INFINITY;
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const double z = zbuf[(size_t)gy * width + gx];
            const float v = ao_eye_depth(p.m, z);
            if (__builtin_isfinite(z) && __builtin_isfinite(v)) e = v;
        }
        s_e[i] = e;
    }
    __syncthreads();

    // ---- 2. every sample's factor
    const float taps[AO_PAIRS][2] = MR_AO_TAP_TABLE;
    float mine[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * BLOCK;
        const int ly = i / TW, lx = i - ly * TW;
        const float *c = s_e + (ly + R) * LW + (lx + R);
        const float e = *c;
        float ao = 1.0f;                                       // background, and the samples beyond the frame's edge
        if (e < INFINITY) {
            const float rp = ao_footprint(p, e);
            float sum = 0.0f;
#pragma unroll
            for (int t = 0; t < AO_PAIRS; ++t) {
                const int dx = (int)rintf(taps[t][0] * rp), dy = (int)rintf(taps[t][1] * rp);     // |dx|, |dy| <= R
                sum = sum + ao_pair(p, e, c[dy * LW + dx], c[-dy * LW - dx]);
            }
            ao = ao_factor(p, sum);
        }
        mine[j] = ao;
    }
    __syncthreads();                                           // every tap has been read: the factors take the depths' place
    float *s_ao = s_e;
#pragma unroll
    for (int j = 0; j < PER; ++j) s_ao[tid + j * BLOCK] = mine[j];
    __syncthreads();

    // ---- 3. the float frame's rows, in place
    const int w = min(TW, width - x0), h = min(TH, height - y0);
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < h; r += BLOCK / 64) {
        const size_t first = ((size_t)(y0 + r) * width + x0) * 3;          // the frame is a 256-byte aligned allocation
        float *row = frame + first;
        const int nf = 3 * w;
        const int head = min((int)((4 - (first & 3)) & 3), nf);
        const int n4 = (nf - head) >> 2, tail = nf - head - 4 * n4;
        const float *ao = s_ao + r * TW;
        if (lane < n4) {
            float4 *q = reinterpret_cast<float4 *>(row + head) + lane;
            const int fi = head + 4 * lane;
            float4 f = *q;
            f.x = f.x * ao[fi / 3]; f.y = f.y * ao[(fi + 1) / 3]; f.z = f.z * ao[(fi + 2) / 3]; f.w = f.w * ao[(fi + 3) / 3];
            *q = f;
        } else {
            const int s = lane - N4_MAX;
            int fi = -1;
            if (s >= 0 && s < head) fi = s;
            else if (s >= 4 && s - 4 < tail) fi = head + 4 * n4 + (s - 4);
            if (fi >= 0) row[fi] = row[fi] * ao[fi / 3];
        }
    }
}

}  // namespace mr
