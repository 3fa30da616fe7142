// kernels_dof.h -- k_dof: thin-lens depth of field (dof_def.h has the definition) gathered from a frame's float
// colours and z-buffer into a second float frame.
//
// A workgroup of BLOCK threads owns TW x TH samples.  It reads the z-buffer and the colours of its rectangle and of a halo
// of DOF_MAX_RADIUS samples round it ONCE and keeps, per staged sample, (r, g, b, s) as one 16-byte word and 1 / rr as a
// float beside it in LDS: 20 bytes a sample, 80 KiB for 32 x 32 samples and their halo, two workgroups to a compute unit.
// While staging, every thread keeps the largest rr it met; the workgroup reduces them (shuffles inside a wavefront, one
// float per wavefront through LDS, no atomics), and its square root bounds the gather's loops for all its samples -- a
// tap farther than that from any sample fails the definition's test whatever the sample, and failing taps are skipped, so
// the bound changes no bit (dof_def.h).  Rows are walked dy ascending and, inside a row, dx ascending over the chord of that
// disc; the bounds are uniform, so both loop counters live in scalar registers, and a tap outside the frame is masked,
// not branched round.  A tap is one 16-byte and one 4-byte LDS read; it divides nothing (1 / rr_t is the max of two staged
// reciprocals).  A workgroup whose rectangle and halo are in focus gathers one tap per sample.  The result goes to `out`,
// another buffer than `frame`: neighbours' colours are read.  No scratch, no memset, no atomics.
//
// Compiled in dof.hip, a translation unit and a code object of its own, like the accumulation's and the obscurance's
// kernels: a kernel added to mi355rast.hip's code object moves k_setup and k_tile to other addresses (kernels_accum.h).
#pragma once

#include "dof_def.h"

namespace mr {

template <int TW, int TH, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_dof(const double *__restrict__ zbuf, const float *__restrict__ frame, float *__restrict__ out, int width, int height, const DofParams p)
{
    constexpr int R = DOF_MAX_RADIUS, LW = TW + 2 * R, LH = TH + 2 * R;
    constexpr int PER = TW * TH / BLOCK;                       // samples a thread owns
    constexpr int WAVES = BLOCK / 64;
    static_assert(PER * BLOCK == TW * TH && BLOCK % 64 == 0, "every thread owns the same number of samples");
    __shared__ float4 s_cs[LH * LW];                           // r, g, b, s; zeroes outside the frame (never added: masked)
    __shared__ float s_inv[LH * LW];                           // 1 / rr
    // The halo's first row is tapped at its middle column only (dy = -R leaves dx = 0), so the reciprocals of its first
    // WAVES cells are never read: the reduction's floats take their place, and 32 x 32 samples stay at 80 KiB exactly.
    static_assert(WAVES <= R, "the reduction's floats lie in cells no tap reads");
    float *s_top = s_inv;
    const int x0 = (int)blockIdx.x * TW, y0 = (int)blockIdx.y * TH, tid = (int)threadIdx.x;

    // ---- 1. colours, circle and reciprocal squared radius of the rectangle and its halo; the largest rr among them
    float top = 0.25f;                                         // (no rr is smaller)
    for (int i = tid; i < LW * LH; i += BLOCK) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0 - R + lx, gy = y0 - R + ly;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float inv = 0.0f;
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const size_t g = (size_t)gy * width + gx;
            const double z = zbuf[g];
            float e = ao_eye_depth(p.m, z);
            if (!(__builtin_isfinite(z) && __builtin_isfinite(e))) e = INFINITY;
            const float s = dof_coc(p, e), rr = dof_rr(s);
            const float *f = frame + g * 3;
            v = make_float4(f[0], f[1], f[2], s);
            inv = 1.0f / rr;
            top = rr > top ? rr : top;
        }
        s_cs[i] = v;
        if (i >= WAVES) s_inv[i] = inv;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float other = __shfl_xor(top, m, 64);
        top = other > top ? other : top;
    }
    if ((tid & 63) == 0) s_top[tid >> 6] = top;
    __syncthreads();
    top = s_top[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) top = s_top[w] > top ? s_top[w] : top;
    // the bound, the same for every thread: a tap passes only if dx * dx + dy * dy <= rr_q <= top <= 256
    const int r2 = min(__builtin_amdgcn_readfirstlane((int)top), R * R);
    int bound = 0;
    while ((bound + 1) * (bound + 1) <= r2) ++bound;           // <= R: every tap stays inside the staged rectangle

    // ---- 2. the gather
#pragma unroll 1
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * BLOCK;
        const int ly = i / TW, lx = i - ly * TW;
        const int gx = x0 + lx, gy = y0 + ly;
        const bool mine = gx < width && gy < height;
        const int c = (ly + R) * LW + (lx + R);
        const float s_p = s_cs[c].w, inv_p = s_inv[c];
        const float rr_p = dof_rr(s_p);
        float W = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f;
        for (int dy = -bound; dy <= bound; ++dy) {
            const int rest = r2 - dy * dy;                     // >= 0
            int chord = (int)sqrtf((float)rest);
            if ((chord + 1) * (chord + 1) <= rest) ++chord;
            if (chord * chord > rest) --chord;
            const bool row_in = mine && (unsigned)(gy + dy) < (unsigned)height;
            const int row = c + dy * LW;
            for (int dx = -chord; dx <= chord; ++dx) {
                const float4 q = s_cs[row + dx];
                const float inv_q = s_inv[row + dx];
                const float rr_q = dof_rr(q.w);
                const bool behind = q.w > s_p;
                const float rr_t = (behind && rr_p < rr_q) ? rr_p : rr_q;         // dof_tap_rr
                const float w = (behind && inv_p > inv_q) ? inv_p : inv_q;        // 1.0f / rr_t
                if (row_in && (unsigned)(gx + dx) < (unsigned)width && (float)(dx * dx + dy * dy) <= rr_t) {
                    W = W + w;
                    S0 = S0 + w * q.x; S1 = S1 + w * q.y; S2 = S2 + w * q.z;
                }
            }
        }
        if (mine) {
            float *o = out + ((size_t)gy * width + gx) * 3;
            o[0] = S0 / W; o[1] = S1 / W; o[2] = S2 / W;
        }
    }
}

}  // namespace mr
