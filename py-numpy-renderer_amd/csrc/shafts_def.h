// shafts_def.h -- light shafts, the sky's light streaming past occluders towards a light's place on the screen: the
// definition, once, for the kernels (kernels_shafts.h) and for the host mirror (host_shafts.h), which both include this
// file; tests/shafts_ref.py restates it in NumPy.  No kernel lives here: mi355rast.hip includes this header and its code
// object must not grow (kernels_accum.h says why).
//
// On the sample grid (Hs, Ws), rows bottom-up, with F the float frame in front of the pass (behind the motion blur, in
// front of the bloom and the overlay), Z the z-buffer, t = threshold, g = gain, d = levels in 1 .. 4, n = samples in
// 1 .. 128, (lx, ly) the light on level d, step = float32(density / n), w_i the weights.  float32 throughout, every
// operation rounded on its own (-ffp-contract=off), no fma:
//
//   source       a sample is SKY when Z is not finite (what ao_def.h calls background: k_tile leaves +-inf there, under
//                a colour sky and under a skybox alike).  S_0 = F * bloom_bright(r, g, b, t) per channel at a sky
//                sample, +0 elsewhere.  The bright factor is bloom_def.h's.
//   level sizes  H_0, W_0 = Hs, Ws;  H_l = bloom_half(H_{l-1}), W_l = bloom_half(W_{l-1})   (the ceiling)
//   reduction    B_0 = S_0;  B_{l+1}[y][x] = ((a00 + a01) + (a10 + a11)) * 0.25 over B_l at (2y, 2x), (2y, 2x+1),
//                (2y+1, 2x), (2y+1, 2x+1); a sample outside the level counts +0 (what is beyond the frame is not sky).
//                S = B_d, (H_d, W_d).  The tree is the definition; how it is spread over lanes or registers is not.
//   fetch        fetch(A, qx, qy) of a level A (H, W) is for -0.5 <= qx <= W - 0.5 and -0.5 <= qy <= H - 0.5, tested on
//                the floats before any conversion; a position outside that rectangle (or not a number) fetches nothing
//                and the tap contributes +0.  Inside: qx clamped to [0, W - 1], x0 = (int)qx, x1 = min(x0 + 1, W - 1),
//                fx = qx - (float)x0, likewise y; per channel h0 = a00 + fx*(a01 - a00), h1 = a10 + fx*(a11 - a10),
//                v = h0 + fy*(h1 - h0).
//   march        for the coarse sample (x, y), cx = (float)x, cy = (float)y:  dx = (lx - cx) * step, dy = (ly - cy) * step;
//                q_i = (cx + dx*(float)i, cy + dy*(float)i), i = 0 .. n-1;  R = sum_i w_i * fetch(S, q_i), summed in
//                ascending i as acc = acc + w_i * v from +0.
//   composite    out = bloom_composite(F, g, fetch(R, (x + 0.5) * 2^-d - 0.5, (y + 0.5) * 2^-d - 0.5)) on the sample
//                grid; those coordinates are exact in float32 and always inside.
//
// What follows, and what the tests rely on:
//   * No sky sample, or none above t: S = R = +0 and out == F + g*0 == F bit for bit (F >= 0).
//   * A uniform sky s over a whole grid whose sides are multiples of 2^d: S is s * k everywhere, exactly (4c/4), and with
//     the light inside the frame and density <= 1 every tap is inside and fetches that value exactly (a + f*(a - a) = a):
//     R is the same iterated sum acc = acc + w_i * S at every coarse sample.
//   * A ray's coordinates are monotone in i (one rounded product, one rounded sum) and tap 0 is the sample itself, so once
//     a tap is outside every later one is: a march may stop at its first outside tap.  acc is never -0, so a tap that is
//     left out and a tap that adds +0 are the same thing.
//   * Every value is finite for a finite F: the only division is the bright factor's, whose divisor is m > t >= 0.
//   * Every index is formed after its clamp.
#pragma once

#include <cmath>
#include <cstdint>

#include "ao_def.h"
#include "bloom_def.h"

namespace mr {

constexpr int SHAFTS_MAX_LEVELS = 4;
constexpr int SHAFTS_MAX_SAMPLES = 128;

// What the kernels take: mr_light_shafts_desc, checked (host_shafts.h, shafts_params).
struct ShaftsParams {
    float light_x, light_y, threshold, gain, step;
    int32_t samples, levels;
    float weights[SHAFTS_MAX_SAMPLES];
};

// sky: no face covers the sample
MR_AO_HD inline bool shafts_sky(double z) { return !__builtin_isfinite(z); }

// one channel's three steps up the tree: the four samples under a coarser one, rows ascending
MR_AO_HD inline float shafts_pair(float a, float b) { return a + b; }
MR_AO_HD inline float shafts_quad(float row0, float row1) { return (row0 + row1) * 0.25f; }

// 2^-d, exact
MR_AO_HD inline float shafts_inv_scale(int levels) { return 1.0f / (float)(1 << levels); }

// where a tap reads: the four corners and the two fractions
struct ShaftsTap {
    int x0, x1, y0, y1;
    float fx, fy;
};

// the tap of position (qx, qy) on a level of h x w; false: outside (or not a number), and it fetches nothing -- `t` is
// then still a place inside the level, so that a caller may read it and discard what it read
MR_AO_HD inline bool shafts_tap(float qx, float qy, int w, int h, ShaftsTap &t)
{
    const bool inside = qx >= -0.5f && qx <= (float)w - 0.5f && qy >= -0.5f && qy <= (float)h - 0.5f;
    const float ux = inside ? fminf(fmaxf(qx, 0.0f), (float)(w - 1)) : 0.0f;
    const float uy = inside ? fminf(fmaxf(qy, 0.0f), (float)(h - 1)) : 0.0f;
    t.x0 = (int)ux; t.y0 = (int)uy;
    t.x1 = t.x0 + 1 < w - 1 ? t.x0 + 1 : w - 1;
    t.y1 = t.y0 + 1 < h - 1 ? t.y0 + 1 : h - 1;
    t.fx = ux - (float)t.x0; t.fy = uy - (float)t.y0;
    return inside;
}

// one channel of a fetch: rows first
MR_AO_HD inline float shafts_bilerp(float a00, float a01, float a10, float a11, float fx, float fy)
{
    const float h0 = a00 + fx * (a01 - a00);
    const float h1 = a10 + fx * (a11 - a10);
    return h0 + fy * (h1 - h0);
}

// tap i of the ray from c towards the light, one coordinate
MR_AO_HD inline float shafts_ray_delta(float light, float c, float step) { return (light - c) * step; }
MR_AO_HD inline float shafts_ray_at(float c, float delta, int i) { return c + delta * (float)i; }

// acc = acc + w_i * v
MR_AO_HD inline float shafts_add(float acc, float w, float v) { return acc + w * v; }

// where a sample of the grid reads R: (x + 0.5) * 2^-d - 0.5
MR_AO_HD inline float shafts_coarse_at(int x, float inv_scale) { return ((float)x + 0.5f) * inv_scale - 0.5f; }

}  // namespace mr
