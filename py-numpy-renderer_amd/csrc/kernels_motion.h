// kernels_motion.h -- k_velocity and k_mblur: per-sample screen-space motion from the z-buffer and the winner map, and the
// blur gathered along it from a frame's float colours into a second float frame (motion_def.h has the definition).
//
// k_velocity: one thread per sample.  It reads 8 + 4 bytes (z and winner) and writes 8 (U).  The tables -- the class
// matrices, the background's, the models' first faces and their classes -- are one small read-only block that every thread
// reads through the caches; the model of a face is a binary search over the first faces.
//
// k_mblur has k_dof's structure.  A workgroup of BLOCK threads owns TW x TH samples.  It reads z, U and the colours of its
// rectangle and of a halo of MOTION_MAX_HALF samples round it ONCE and keeps, per staged sample, (r, g, b, e) as one 16-byte
// word and (d.x, d.y, h, 1 / (2 h + 1)) as another: 32 bytes a sample, 128 KiB for 32 x 32 samples and their halo (one
// workgroup to a compute unit), 72 KiB for 16 x 16 (two).  While staging, every thread keeps the largest h it met; the
// workgroup reduces them (shuffles inside a wavefront, one float per wavefront through LDS, no atomics) and motion_bound
// of it bounds both loops of the gather for all its samples: the taps left out fail the definition's test, and failing
// taps are skipped, so the bound changes no bit.  The bounds are uniform, so both loop counters live in scalar registers;
// a tap outside the frame is masked, not branched round.  A tap is two 16-byte LDS reads and divides nothing.  A workgroup
// whose rectangle and halo are at rest gathers one tap per sample.  The result goes to `out`, another buffer than
// `frame`: neighbours' colours are read.  No scratch, no memset, no atomics in either kernel.
//
// Compiled in motion.hip, a translation unit and a code object of its own, like the accumulation's, the obscurance's and
// the depth of field's kernels: a kernel added to mi355rast.hip's code object moves k_setup and k_tile to other addresses
// (kernels_accum.h).
#pragma once

#include "motion_def.h"

namespace mr {

constexpr int VELOCITY_BLOCK = 256;

// tables: (n_classes * MOTION_T + MOTION_B) doubles, then n_models first faces, then n_models classes (int32 each)
__global__ void __launch_bounds__(VELOCITY_BLOCK)
k_velocity(const double *__restrict__ zbuf, const int32_t *__restrict__ winner, const double *__restrict__ tables, float2 *__restrict__ vel,
           int width, int height, const MotionParams p)
{
    const size_t i = (size_t)blockIdx.x * VELOCITY_BLOCK + threadIdx.x;
    if (i >= (size_t)width * height) return;
    const int y = (int)(i / (size_t)width), x = (int)(i - (size_t)y * width);
    const double *B = tables + (size_t)p.n_classes * MOTION_T;
    const int32_t *face_off = reinterpret_cast<const int32_t *>(B + MOTION_B), *class_of = face_off + p.n_models;
    const int32_t w = winner[i];
    int cls = 0;
    if (w >= 0 && p.n_models > 0) cls = class_of[motion_model_of(face_off, p.n_models, w)];
    float ux, uy;
    motion_velocity(tables + (size_t)cls * MOTION_T, B, zbuf[i], x, y, ux, uy);
    vel[i] = make_float2(ux, uy);
}

template <int TW, int TH, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
k_mblur(const double *__restrict__ zbuf, const float2 *__restrict__ vel, const float *__restrict__ frame, float *__restrict__ out,
        int width, int height, const MotionParams p)
{
    constexpr int R = MOTION_MAX_HALF, LW = TW + 2 * R, LH = TH + 2 * R;
    constexpr int PER = TW * TH / BLOCK;                       // samples a thread owns
    constexpr int WAVES = BLOCK / 64;
    static_assert(PER * BLOCK == TW * TH && BLOCK % 64 == 0, "every thread owns the same number of samples");
    __shared__ float4 s_ce[LH * LW];                           // r, g, b, e; outside the frame: never added (masked)
    __shared__ float4 s_seg[LH * LW];                          // d.x, d.y, h, 1 / (2 h + 1)
    __shared__ float s_top[WAVES];
    const int x0 = (int)blockIdx.x * TW, y0 = (int)blockIdx.y * TH, tid = (int)threadIdx.x;

    // ---- 1. colours, eye depth and motion segment of the rectangle and its halo; the largest h among them
    float top = 0.0f;
    for (int i = tid; i < LW * LH; i += BLOCK) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0 - R + lx, gy = y0 - R + ly;
        float4 ce = make_float4(0.0f, 0.0f, 0.0f, INFINITY), seg = make_float4(1.0f, 0.0f, 0.0f, 1.0f);
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const size_t g = (size_t)gy * width + gx;
            const double z = zbuf[g];
            float e = ao_eye_depth(p.m, z);
            if (!(__builtin_isfinite(z) && __builtin_isfinite(e))) e = INFINITY;
            const float2 u = vel[g];
            const float *f = frame + g * 3;
            ce = make_float4(f[0], f[1], f[2], e);
            motion_segment(p.shutter, u.x, u.y, seg.z, seg.x, seg.y, seg.w);
            top = seg.z > top ? seg.z : top;
        }
        s_ce[i] = ce;
        s_seg[i] = seg;
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
    // the bound, the same for every thread and <= R: every tap stays inside the staged rectangle
    const int bound = __builtin_amdgcn_readfirstlane(motion_bound(top));

    // ---- 2. the gather
#pragma unroll 1
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * BLOCK;
        const int ly = i / TW, lx = i - ly * TW;
        const int gx = x0 + lx, gy = y0 + ly;
        const bool mine = gx < width && gy < height;
        const int c = (ly + R) * LW + (lx + R);
        const float e_p = s_ce[c].w;
        const float4 seg_p = s_seg[c];
        float W = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f;
        for (int dy = -bound; dy <= bound; ++dy) {
            const bool row_in = mine && (unsigned)(gy + dy) < (unsigned)height;
            const int row = c + dy * LW;
            for (int dx = -bound; dx <= bound; ++dx) {
                const float4 q = s_ce[row + dx];
                const float4 sq = s_seg[row + dx];
                float w;
                const bool pass = motion_tap(dx, dy, e_p, seg_p.z, seg_p.w, q.w, sq.z, sq.w, sq.x, sq.y, w);
                if (row_in && (unsigned)(gx + dx) < (unsigned)width && pass) {
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
