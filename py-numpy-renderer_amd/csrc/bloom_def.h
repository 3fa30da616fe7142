// bloom_def.h -- bloom, a glow round the samples brighter than a threshold, gathered from a resolution pyramid: the
// definition, once, for the kernels (kernels_bloom.h) and for the host mirror (host_bloom.h), which both include this file;
// tests/bloom_ref.py restates it in NumPy.  No kernel lives here: mi355rast.hip includes this header and its code object
// must not grow (kernels_accum.h says why).
//
// On the sample grid (Hs, Ws), rows bottom-up, with F the float frame in front of the pass (behind the motion blur, in
// front of the overlay), t = threshold, g = gain, L = levels in 1 .. 8.  float32 throughout, every operation rounded on
// its own (-ffp-contract=off), every weight dyadic:
//
//   bright pass    m = fmaxf(fmaxf(r, g), b);   k = m > t ? (m - t) / m : 0;   B0 = F * k            per channel
//   level sizes    H0, W0 = Hs, Ws;   H_l = (H_{l-1} + 1) / 2,  W_l = (W_{l-1} + 1) / 2   (the ceiling; 1 x 1 halves to 1 x 1)
//   down           D_0 = B0;  D_l[y][x] from D_{l-1} at the source taps 2x-1 .. 2x+2 by 2y-1 .. 2y+2, coordinates clamped
//                  to the source level.  Rows first, in ascending source row order:
//                      r_j = (a0 + a3) + 3*(a1 + a2)          j = 0 .. 3
//                      v   = (r0 + r3) + 3*(r1 + r2);    D_l = v * (1/64)
//   up             up(C) onto a finer grid (H, W): for a fine index i, near = i / 2, far = near - 1 for even i and
//                  near + 1 for odd i, clamped to the coarse level; per coarse row h = 3*C[near_x] + C[far_x], then
//                      v = 3*h[near_y] + h[far_y];       up = v * (1/16)
//   up chain       U_L = D_L;   U_l = D_l + up(U_{l+1})       l = L-1 .. 1
//   composite      out = F + g * up(U_1)                       on the sample grid
//
// What follows, and what the tests rely on:
//   * Where no sample exceeds t, B0 is +0 everywhere (F >= 0), every level is +0, and out == F + g*0 == F bit for bit.
//   * A uniform field stays uniform at every level, exactly: 8c/8 and 4c/4 are exact (sums of at most 64 c scaled by a
//     power of two).  The glow of a uniform bright value b is then the iterated sum b + (b + (...)) with L terms.
//   * Away from borders the pair conserves mass: every source sample's down weights sum to 1/4 over the four times
//     smaller level, every coarse sample's up weights sum to 4 over the finer one.  The glow of one bright sample sums to
//     L times its bright value; exactly so on a dyadic input at L <= 3.
//   * F is finite, so every level is finite: no division but the bright pass's, whose divisor is m > t >= 0.
//   * Every index is formed after its clamp.
#pragma once

#include <cmath>
#include <cstdint>

#include "ao_def.h"

namespace mr {

constexpr int BLOOM_MAX_LEVELS = 8;

// What the kernels take: mr_bloom_desc as float32, checked (host_bloom.h, bloom_params).
struct BloomParams {
    float threshold, gain;
    int32_t levels;
};

// the next level's extent
MR_AO_HD inline int bloom_half(int n) { return (n + 1) / 2; }

// the bright pass's factor of one sample
MR_AO_HD inline float bloom_bright(float r, float g, float b, float t)
{
    const float m = fmaxf(fmaxf(r, g), b);
    return m > t ? (m - t) / m : 0.0f;
}

// four taps of the down filter, along a row or across the four rows' sums
MR_AO_HD inline float bloom_down4(float a0, float a1, float a2, float a3) { return (a0 + a3) + 3.0f * (a1 + a2); }

MR_AO_HD inline float bloom_down_scale(float v) { return v * 0.015625f; }

// the far coarse index of fine index i, clamped to a coarse level of n
MR_AO_HD inline int bloom_far(int i, int n)
{
    const int near = i >> 1;
    const int far = (i & 1) ? near + 1 : near - 1;
    return far < 0 ? 0 : (far > n - 1 ? n - 1 : far);
}

// one channel of up(C): the four coarse taps, near row first
MR_AO_HD inline float bloom_up(float nn, float nf, float fn, float ff)
{
    const float h_near = 3.0f * nn + nf;     // the near row: C[near_y][near_x], C[near_y][far_x]
    const float h_far = 3.0f * fn + ff;      // the far row:  C[far_y][near_x],  C[far_y][far_x]
    return (3.0f * h_near + h_far) * 0.0625f;
}

// out = F + g * up(U_1)
MR_AO_HD inline float bloom_composite(float f, float g, float u) { return f + g * u; }

}  // namespace mr
