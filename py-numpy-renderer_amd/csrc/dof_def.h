// dof_def.h -- thin-lens depth of field from the z-buffer: the definition, once, for the kernel (kernels_dof.h) and for
// the host mirror (host_dof.h), which both include this file; tests/dof_ref.py restates it in NumPy.  No kernel lives
// here: mi355rast.hip includes this header and its code object must not grow (kernels_dof.h says why).
//
// On the sample grid (Hs, Ws), rows bottom-up, with Z the z-buffer (mr_read_z) and F the float frame after the lights'
// sum and the obscurance, before the overlay:
//
//   e      = ao_eye_depth(m, Z)                     the obscurance's eye depth (ao_def.h: a float64 chain, one rounding to
//                                                   float32); Z or e not finite: background, e = +inf
//   s      = perspective ? kf * (1 - focus / e)     the signed circle of confusion in samples, > 0 behind the plane in focus;
//                         : kf * (e - focus)        background: kf under perspective, +inf under an orthographic camera
//   c      = min(|s|, DOF_MAX_RADIUS)
//   rr     = max(c * c, 0.25f)                      the squared effective radius: a sample always covers itself
//   for dy = -16 .. 16 ascending, for dx = -16 .. 16 ascending, q = p + (dx, dy) inside the frame:
//       behind = s_q > s_p                          q lies behind p
//       rr_t   = behind ? min(rr_q, rr_p) : rr_q    a blurred background does not bleed over a sharper foreground
//       if (float)(dx * dx + dy * dy) <= rr_t:      a tap that fails is SKIPPED, not added as a zero
//           w = 1.0f / rr_t;   W = W + w;   S[ch] = S[ch] + w * F[q][ch]        the product rounded, then the sum
//   F'[p][ch] = S[ch] / W
//
// float32 from s on, every operation rounded on its own (-ffp-contract=off), the divisions IEEE.  kf = float32(lens_radius
// * 0.5 * Hs * |P[1][1]| / focus): a point at eye depth e spreads over a disc of lens_radius * |e - focus| / focus world
// units at its own depth (a thin lens focused at eye depth `focus`), which is |s| samples.
//
// What follows from it, and what the kernel relies on:
//   * Background samples take part: a sky blurs (a skybox's colours are in F), and under perspective it has c = min(kf, 16).
//   * A tap passes only if its squared distance is <= rr_q, and failing taps are skipped in a fixed order: any loop bound
//     whose square is at or above the largest rr among the samples a workgroup can tap gives the same bits.  The kernel
//     bounds its loops by the largest rr of the rectangle it stages; where that is in focus a sample costs one tap.
//   * 1.0f / min(a, b) == max(1.0f / a, 1.0f / b) bit for bit (a correctly rounded quotient is monotone), so 1 / rr is
//     staged once per sample and a tap takes a max; it does not divide.
//   * Where c < 0.5 for p and for every q in front of it within 16 samples, only p's own tap passes, w = 4, and
//     (4 F) / 4 == F bit for bit.
#pragma once

#include "ao_def.h"

namespace mr {

constexpr int DOF_MAX_RADIUS = 16;           // the circle's clamp, in samples: the halo a workgroup stages

// What the kernel takes by value: mr_dof_desc as float32, checked (host_dof.h, dof_params).
struct DofParams {
    double m[4];                 // Z -> eye depth (ao_eye_depth)
    float kf, focus;
    int32_t perspective;
};

// signed circle of confusion of a sample at eye depth e (+inf: background), in samples
MR_AO_HD inline float dof_coc(const DofParams &p, float e)
{
    return p.perspective ? p.kf * (1.0f - p.focus / e) : p.kf * (e - p.focus);
}

// squared effective radius of a sample whose signed circle is s
MR_AO_HD inline float dof_rr(float s)
{
    const float a = fabsf(s);
    const float c = a < (float)DOF_MAX_RADIUS ? a : (float)DOF_MAX_RADIUS;
    const float rr = c * c;
    return rr > 0.25f ? rr : 0.25f;
}

// the squared radius a tap q is tested against and weighs by, seen from p
MR_AO_HD inline float dof_tap_rr(float s_p, float rr_p, float s_q, float rr_q)
{
    return (s_q > s_p && rr_p < rr_q) ? rr_p : rr_q;
}

}  // namespace mr
