// motion_def.h -- motion blur from a per-sample velocity buffer: the definition, once, for the kernels (kernels_motion.h)
// and for the host mirrors (host_motion.h), which both include this file; tests/motion_ref.py restates it in NumPy.  No
// kernel lives here: mi355rast.hip includes this header and its code object must not grow (kernels_accum.h says why).
//
// On the sample grid (Hs, Ws), rows bottom-up, at integer screen coordinates (x, y), with Z the z-buffer (mr_read_z), w the
// winner map (mr_read_winner) and F the float frame after the lights' sum, the obscurance and the depth of field, before
// the overlay.
//
// VELOCITY (k_velocity).  The host hands over one float64 4 x 3 matrix T per motion class (row vectors, row-major) and one
// 3 x 3 matrix B for the background; class 0 is "the camera only", a model whose pose changed has a class of its own.
//
//   class    = w < 0 ? 0 : class_of_model[model of face w]             model: the last m with face_off[m] <= w
//   finite Z:     u_c = ((x*Z)*T[0][c] + (y*Z)*T[1][c] + Z*T[2][c]) + T[3][c]           c = 0, 1, 2
//   background (Z not finite):  u_c = (x*B[0][c] + y*B[1][c]) + B[2][c]
//   front = finite Z ? u_2 * Z > 0 : u_2 > 0                            the point lay in front of the previous camera
//   U = front ? ((float)(x - u_0/u_2), (float)(y - u_1/u_2)) : (0, 0);  U = (0, 0) too unless both floats are finite
//
// float64, left to right, every operation rounded on its own (-ffp-contract=off), IEEE divisions, one rounding to float32
// at the end.  U is the displacement in samples since the previous frame, unclamped.  (u_0/u_2, u_1/u_2) is where the
// sample's surface point was on the previous frame's sample grid: (x*Z, y*Z, Z, 1) is proportional to the sample's
// homogeneous world point pushed through the frame's own view, projection, viewport and the inverse of linearize_z, and T
// carries it on through the inverse of all that, the model's motion and the previous frame's matrices
// (_pack.motion_matrices), so that u = (Z / w_now) * (the point's previous homogeneous screen position): w_now > 0 for what a
// frame shows, and u_2 * Z has the sign of the previous w whichever side of linearize_z's pole Z lies on (an orthographic
// camera, whose near plane passes through the scene, shows both).  T is scaled by a positive number only.  The background
// lies at infinity where the camera has a perspective -- under a rotating camera a sky moves, under a translating one it
// does not -- and on the far plane where it has none; B maps (x, y, 1) to its previous homogeneous screen position.
//
// BLUR (k_mblur).  float32 from here on, every operation rounded on its own; e = ao_eye_depth as in dof_def.h (a sample
// whose Z or e is not finite is background, e = +inf).  Per sample:
//
//   v = shutter * U;   L = sqrtf(v.x*v.x + v.y*v.y)
//   0.5f <= L <= FLT_MAX :  h = min(L*0.5f, 16),  d = (v.x / L, v.y / L)
//   else                 :  h = 0,                d = (1, 0)          less than half a sample (or no number): at rest
//   inv = 1.0f / (2.0f*h + 1.0f)
//
//   for dy = -16 .. 16 ascending, dx = -16 .. 16 ascending, q = p + (dx, dy) inside the frame:
//       o      = (-dx, -dy)                                     from q to p
//       along  = o.x*d_q.x + o.y*d_q.y;   perp = o.x*d_q.y - o.y*d_q.x
//       behind = e_q > e_p
//       h_t    = (behind && h_p < h_q) ? h_p : h_q              a moving background does not smear over a stiller foreground
//       if fabsf(along) <= h_t + 0.5f && fabsf(perp) <= 0.5f:   a tap that fails is SKIPPED, not added as a zero
//           w = 1.0f / (2.0f*h_t + 1.0f);   W = W + w;   S[ch] = S[ch] + w * F[q][ch]
//   F'[p][ch] = S[ch] / W
//
// A sample gathers from the samples whose motion segment, q +- v_q / 2 and half a sample wide, passes over it: k_dof's
// scheme with a segment in place of a disc.  What follows, and what the kernel relies on:
//   * A sample's own tap always passes: o = (0, 0) gives along = perp = 0 whatever the (finite) d, and 0 <= h_t + 0.5.
//   * Where h = 0 for p and for every q in front of it within 16 samples, only the own tap passes: another tap has
//     h_t = 0 (q in front: h_q; q behind: min(h_p, h_q) = 0), and along^2 + perp^2 = dx^2 + dy^2 >= 1 up to rounding
//     cannot have both parts <= 0.5.  The own w is 1.0f / 1.0f = 1 exactly, so F'[p] == F[p] bit for bit: a frame in which
//     nothing moves by half a sample is render()'s, byte for byte.
//   * w is the staged reciprocal of the sample h_t was taken from: a tap divides nothing.
//   * A passing tap has dx^2 + dy^2 <= (h_q + 0.5)^2 + 0.25 < (h_q + 1)^2, so |dx|, |dy| <= floor(h_max + 1) (capped at 16)
//     for a workgroup whose staged rectangle has largest half-length h_max, and only the own tap passes where h_max = 0:
//     the bound is 0 there.  Failing taps are skipped, so the bound changes no bit, and a rectangle at rest costs one tap
//     per sample.
//   * (float)sqrt((double)s) == sqrtf(s) for every float s (53 >= 2 * 24 + 2 bits), should a device's sqrtf ever differ.
//   * One layer only: what shows behind a moving object is not in the frame.
#pragma once

#include <cfloat>

#include "dof_def.h"

namespace mr {

constexpr int MOTION_MAX_HALF = 16;          // the half-length's clamp, in samples: the halo a workgroup stages
constexpr int MOTION_T = 12, MOTION_B = 9;   // doubles of a class matrix and of the background's

// What the kernels take by value: mr_motion_desc's scalars, checked (host_motion.h, motion_params).
struct MotionParams {
    double m[4];                 // Z -> eye depth (ao_eye_depth)
    float shutter;
    int32_t n_classes, n_models;
};

// the model that owns face w >= 0: the last m with face_off[m] <= w (face_off ascending, face_off[0] == 0)
MR_AO_HD inline int motion_model_of(const int32_t *face_off, int n_models, int32_t w)
{
    int lo = 0, hi = n_models - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (face_off[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// U of one sample; T: the 12 doubles of its class, B: the background's 9
MR_AO_HD inline void motion_velocity(const double *T, const double *B, double z, int x, int y, float &ux, float &uy)
{
    const double xd = (double)x, yd = (double)y;
    double u[3];
    if (__builtin_isfinite(z)) {
        const double xz = xd * z, yz = yd * z;
        for (int c = 0; c < 3; ++c) u[c] = ((xz * T[c] + yz * T[3 + c]) + z * T[6 + c]) + T[9 + c];
    } else {
        for (int c = 0; c < 3; ++c) u[c] = (xd * B[c] + yd * B[3 + c]) + B[6 + c];
    }
    ux = uy = 0.0f;
    const double front = __builtin_isfinite(z) ? u[2] * z : u[2];
    if (front > 0.0) {
        const float a = (float)(xd - u[0] / u[2]), b = (float)(yd - u[1] / u[2]);
        if (__builtin_isfinite(a) && __builtin_isfinite(b)) { ux = a; uy = b; }
    }
}

// a sample's motion segment: half-length h, unit direction d, inv = 1 / (2 h + 1)
MR_AO_HD inline void motion_segment(float shutter, float ux, float uy, float &h, float &dx, float &dy, float &inv)
{
    const float vx = shutter * ux, vy = shutter * uy;
    const float L = sqrtf(vx * vx + vy * vy);
    if (L >= 0.5f && L <= FLT_MAX) {
        const float half = L * 0.5f;
        h = half < (float)MOTION_MAX_HALF ? half : (float)MOTION_MAX_HALF;
        dx = vx / L; dy = vy / L;
    } else {
        h = 0.0f; dx = 1.0f; dy = 0.0f;
    }
    inv = 1.0f / (2.0f * h + 1.0f);
}

// whether the tap q = p + (dx, dy) passes, and its weight
MR_AO_HD inline bool motion_tap(int dx, int dy, float e_p, float h_p, float inv_p, float e_q, float h_q, float inv_q, float dqx, float dqy,
                                float &w)
{
    const float ox = (float)-dx, oy = (float)-dy;
    const float along = ox * dqx + oy * dqy, perp = ox * dqy - oy * dqx;
    const bool own = e_q > e_p && h_p < h_q;                 // behind, and longer than p's
    const float h_t = own ? h_p : h_q;
    w = own ? inv_p : inv_q;
    return fabsf(along) <= h_t + 0.5f && fabsf(perp) <= 0.5f;
}

// the loop bound for a largest half-length h_max (0 .. 16)
MR_AO_HD inline int motion_bound(float h_max)
{
    if (!(h_max > 0.0f)) return 0;
    const int b = (int)(h_max + 1.0f);
    return b < MOTION_MAX_HALF ? b : MOTION_MAX_HALF;
}

}  // namespace mr
