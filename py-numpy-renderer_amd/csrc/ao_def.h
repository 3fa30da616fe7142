// ao_def.h -- screen-space ambient obscurance from the z-buffer: the definition, once, for the kernel (kernels_ao.h)
// and for the host mirror (host_ao.h), which both include this file; tests/ao_ref.py restates it in NumPy.  No kernel
// lives here: mi355rast.hip includes this header and its code object must not grow (kernels_ao.h says why).
//
// On the sample grid (Hs, Ws), rows bottom-up, with Z the z-buffer (mr_read_z) and F the float frame before the overlay:
//
//   e     = (float)((m0 * Z + m1) / (m2 * Z + m3))          float64, every operation rounded on its own, then one
//                                                           rounding to float32; Z or e not finite: background
//   rp    = perspective ? k / e_p : k;   rp = min(max(rp, 1), 32)                              float32, in samples
//   for i = 0 .. 7:   dx = (int)rintf(AO_TAPS[i][0] * rp),  dy = (int)rintf(AO_TAPS[i][1] * rp)       ties to even
//       a = e(x + dx, y + dy),  b = e(x - dx, y - dy)
//       valid = both taps inside the frame and neither background, |e_p - a| <= range and |e_p - b| <= range
//       c   = (e_p - a) + (e_p - b)
//       t   = (c - bias) * inv_fall;   occ = t < 0 ? 0 : t > 1 ? 1 : t;   sum += valid ? occ : 0
//   ao    = 1 - strength * (sum * 0.125f);   ao = ao < 0 ? 0 : ao
//   F'[p] = F[p] * ao                                       a background sample keeps F
//
// float32 from rp on, every operation rounded on its own (-ffp-contract=off), i ascending.  An invalid pair contributes
// nothing -- the whole pair, not one tap: with one tap rejected a steep plane whose far tap leaves `range` darkens.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MR_AO_HD __host__ __device__
#else
#define MR_AO_HD
#endif

namespace mr {

constexpr int AO_PAIRS = 8;
constexpr int AO_MAX_RADIUS = 32;            // the footprint's clamp, in samples: the halo a workgroup stages

// u_i = (cos(i pi / 8), sin(i pi / 8)) * (1 for even i, 0.5 for odd i): eight antipodal pairs, two rings
#define MR_AO_TAP_TABLE { { 1.0f, 0.0f }, { 0.46193977f, 0.19134172f }, { 0.70710678f, 0.70710678f }, { 0.19134172f, 0.46193977f }, \
                          { 0.0f, 1.0f }, { -0.19134172f, 0.46193977f }, { -0.70710678f, 0.70710678f }, { -0.46193977f, 0.19134172f } }

// What the kernel takes by value: mr_ao_desc as float32, checked (host_ao.h, ao_params).
struct AoParams {
    double m[4];                 // Z -> eye depth
    float k;                     // footprint in samples at eye depth 1 (perspective) or everywhere
    float strength, range, bias, inv_fall;
    int32_t perspective;
};

// eye depth of one z-buffer value; not finite for a background sample
MR_AO_HD inline float ao_eye_depth(const double m[4], double z)
{
    const double num = m[0] * z + m[1], den = m[2] * z + m[3];
    return (float)(num / den);
}

MR_AO_HD inline float ao_footprint(const AoParams &p, float e)
{
    float rp = p.perspective ? p.k / e : p.k;
    rp = rp > 1.0f ? rp : 1.0f;
    return rp < (float)AO_MAX_RADIUS ? rp : (float)AO_MAX_RADIUS;
}

// one pair's share; a, b: the taps' eye depths, +inf for a tap that is outside the frame or background
MR_AO_HD inline float ao_pair(const AoParams &p, float e, float a, float b)
{
    const float da = e - a, db = e - b;
    if (!(fabsf(da) <= p.range && fabsf(db) <= p.range)) return 0.0f;
    const float t = ((da + db) - p.bias) * p.inv_fall;
    return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
}

MR_AO_HD inline float ao_factor(const AoParams &p, float sum)
{
    const float ao = 1.0f - p.strength * (sum * 0.125f);
    return ao < 0.0f ? 0.0f : ao;
}

}  // namespace mr
