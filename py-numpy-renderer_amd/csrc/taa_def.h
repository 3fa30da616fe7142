// taa_def.h -- temporal anti-aliasing, a frame's float colours blended into a reprojected history: the definition, once,
// for the kernel (kernels_taa.h) and for the host mirror (host_taa.h), which both include this file; tests/taa_ref.py
// restates it in NumPy.  No kernel lives here: mi355rast.hip includes this header and its code object must not grow
// (kernels_accum.h says why).
//
// On the sample grid (Hs, Ws), rows bottom-up, at integer screen coordinates p = (x, y), with F the float frame in front
// of the pass (after the lights' sum and the obscurance, before the depth of field, the motion blur and the overlay), U
// the velocity (motion_def.h: the displacement of every sample, in samples, since the previous frame), P the history --
// the float frame the previous temporal-AA frame of the scene left behind this pass -- or none, and a = blend.  float32
// throughout, every operation rounded on its own (-ffp-contract=off):
//
//   C = F[p]
//   no history                                          :  out = C
//   rx = (float)x - U.x ;  ry = (float)y - U.y             where the sample's surface point was
//   !(rx >= 0 && rx <= Ws-1 && ry >= 0 && ry <= Hs-1)   :  out = C        off the frame, or no number
//   x0 = (int)floorf(rx),  fx = rx - (float)x0,  x1 = min(x0 + 1, Ws-1);   y0, fy, y1 likewise
//   per channel:   t0 = P[y0][x0] + fx*(P[y0][x1] - P[y0][x0]);   t1 = the same on row y1;   H = t0 + fy*(t1 - t0)
//   mn, mx = fminf / fmaxf over F at the 3 x 3 samples round p, coordinates clamped to the frame, rows then columns
//            ascending, starting from the first of them
//   Hk  = fminf(fmaxf(H, mn), mx)
//   out = Hk + a*(C - Hk)
//   P'[p] = out                                            every sample, also where out = C
//
// What follows, and what the tests rely on:
//   * U == 0 gives rx = x, fx = fy = 0, t0 = P[y][x] + 0*(..) and H == P[p] bit for bit (P finite): the history is fetched
//     at integer positions under a still camera over a still scene.
//   * P == F then gives mn <= H <= mx, Hk == C and out == C + a*0 == C bit for bit: a still scene without jitter repeats
//     render()'s bytes on every frame.
//   * a == 1 is not special-cased: out = Hk + (C - Hk), which is C up to one rounding.
//   * The neighbourhood clamp is the only rejection of stale history: a history colour outside what the 3 x 3 samples
//     round p show now is pulled to the nearest of them.  No depth or winner test, no clipping in another colour space.
//   * A history value that is no number is replaced by mn (fmaxf returns its other argument); F is always finite.
//   * Every index is formed after the range test, so x0, x1, y0, y1 lie inside the frame whatever U holds.
#pragma once

#include <cmath>
#include <cstdint>

#include "ao_def.h"

namespace mr {

// What the kernel takes by value: mr_taa_desc's scalar, checked (host_taa.h, taa_params).
struct TaaParams {
    float blend;
};

// Where the history is fetched for sample (x, y): false when the target lies off the frame or U is no number
MR_AO_HD inline bool taa_target(int x, int y, float ux, float uy, int width, int height, int &x0, int &x1, int &y0, int &y1, float &fx, float &fy)
{
    const float rx = (float)x - ux, ry = (float)y - uy;
    if (!(rx >= 0.0f && rx <= (float)(width - 1) && ry >= 0.0f && ry <= (float)(height - 1))) return false;
    x0 = (int)floorf(rx); y0 = (int)floorf(ry);
    fx = rx - (float)x0; fy = ry - (float)y0;
    x1 = x0 + 1 < width - 1 ? x0 + 1 : width - 1;
    y1 = y0 + 1 < height - 1 ? y0 + 1 : height - 1;
    return true;
}

// one channel of the history at the target: the four taps, rows y0 and y1
MR_AO_HD inline float taa_fetch(float p00, float p01, float p10, float p11, float fx, float fy)
{
    const float t0 = p00 + fx * (p01 - p00);
    const float t1 = p10 + fx * (p11 - p10);
    return t0 + fy * (t1 - t0);
}

// one channel of the result from the fetched history, the neighbourhood's bounds and the sample's own colour
MR_AO_HD inline float taa_blend(float h, float mn, float mx, float c, float a)
{
    const float hk = fminf(fmaxf(h, mn), mx);
    return hk + a * (c - hk);
}

}  // namespace mr
