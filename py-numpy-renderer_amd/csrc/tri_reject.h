// tri_reject.h -- conservative rejection of a (large triangle, tile) pair while binning (kernels_bin.h, bin_work_body).
//
// Plain C++ over rast_types.h: the kernels include it through kernels_bin.h, and tools/host_tri_reject_check.cpp
// compiles the very same function for the CPU and holds it to the kernels' float32 coverage expression sample by sample.
#pragma once

#include <math.h>

#include "rast_types.h"

#if defined(__HIPCC__)
#define MR_TRI_HD __host__ __device__
#else
#define MR_TRI_HD
#endif

namespace mr {

// May the triangle cover a sample of the 16 x 16 tile whose first sample is (gx, gy)?  False only when no sample of
// the tile can pass the coverage test every consumer applies (tri_bary / PairMath::bary: float32 u, v, w >= 0); true
// is always allowed.  The whole tile is a superset of the samples a consumer visits, whatever pixel box, band or
// frame clamp it applies.
//
// With D20 = (p - a) . v0 and D21 = (p - a) . v1 exact,
//     v^ = (d11 D20 - d01 D21) inv_den,   w^ = (d00 D21 - d01 D20) inv_den,   u^ = 1 - v^ - w^
// are affine in the sample p = (x, y) for the record's stored fields, so their largest values over the tile are taken
// at its four corner samples; |D20|, |D21| and the other magnitudes below are convex in p, so theirs are too.  The
// corners are evaluated in float64.  What the kernels compute in float32 differs from v^ by at most
//     Ev = G (|d11 D20| + |d01 D21|) |inv_den|                               the float32 roundings
//        + (G64 (|d11| S20 + |d01| S21) + TINY (|d11| + |d01| + 2)) |inv_den| + TINY
// (likewise Ew with d00 for d11 and the dots exchanged), and from u^ by at most Eu = Ev + Ew + G (1 + |v^| + |w^|).
//   G = 2^-21.  Each of the two terms of v carries four float32 roundings of 2^-24 relative: the float64 dot
//     rounded to float32, the product with d11 (d01), the subtraction, the product with inv_den; (1 + 2^-24)^4 - 1 <
//     4.0000004 * 2^-24.  G = 8 * 2^-24 is twice that: the factor 2 pays for the second-order terms and for this
//     function's own float64 roundings (2^-29 of a float32 one).  u = (1 - v) - w adds two roundings of operands no
//     larger than 1 + |v| + |w|: G is four times those, which also pays for |v| against |v^| there.
//   G64 = 2^-49, on S20 = |rx v0x| + |ry v0y| >= |D20|.  The kernels' float64 dot is three roundings of 2^-53 relative
//     to S20 (p - a, the first product, the fma) in either summation order -- which is why the TF_SINGLE_* flags do not
//     matter here -- and this function's own dot three more: 6 * 2^-53 = 0.1875 * 2^-49, a factor 5 in hand.  It matters
//     only where D20 cancels to nothing, on the line through a along v0's normal.
//   TINY = 2^-124 is an absolute error per float32 operation whose result leaves the normal range, four times the
//     2^-126 a flushed result can lose (a gradual underflow loses 2^-149): one for each dot's conversion, scaled by
//     the d it is multiplied with, one for each product, one for the last product.
// A tile is rejected when the largest corner value of v^, w^ or u^ is below -Ev, -Ew or -Eu.  Anything that is not
// finite, or large enough (2^100) for a float32 intermediate to overflow, keeps the tile: the comparisons are written so
// that a NaN fails them.
MR_TRI_HD inline bool tri_touches_tile(const TriRec &t, int gx, int gy)
{
    constexpr double G = 0x1p-21, G64 = 0x1p-49, TINY = 0x1p-124, LARGE = 0x1p100;
    const double d00 = t.d00, d01 = t.d01, d11 = t.d11, inv = t.inv_den;
    const double a00 = fabs(d00), a01 = fabs(d01), a11 = fabs(d11), ainv = fabs(inv);
    double vmax = 0, wmax = 0, umax = 0;                          // largest corner values (set by the first corner)
    double m20 = 0, m21 = 0, s20 = 0, s21 = 0, mv = 0, mw = 0;    // largest |D20|, |D21|, S20, S21, |v^|, |w^|
    for (int c = 0; c < 4; ++c) {
        const double rx = (double)(gx + (c & 1) * (TILE_W - 1)) - t.ax, ry = (double)(gy + (c >> 1) * (TILE_H - 1)) - t.ay;
        const double p0 = rx * t.v0x, p1 = ry * t.v0y, q0 = rx * t.v1x, q1 = ry * t.v1y;
        const double D20 = p0 + p1, D21 = q0 + q1;
        const double v = (d11 * D20 - d01 * D21) * inv, w = (d00 * D21 - d01 * D20) * inv, u = 1.0 - v - w;
        vmax = c == 0 ? v : fmax(vmax, v);  wmax = c == 0 ? w : fmax(wmax, w);  umax = c == 0 ? u : fmax(umax, u);
        m20 = fmax(m20, fabs(D20));  m21 = fmax(m21, fabs(D21));
        s20 = fmax(s20, fabs(p0) + fabs(p1));  s21 = fmax(s21, fabs(q0) + fabs(q1));
        mv = fmax(mv, fabs(v));  mw = fmax(mw, fabs(w));
        // (fmax drops a NaN operand: a NaN corner is caught by the sum below, which carries every operand)
        if (!(fabs(v) + fabs(w) + fabs(p0) + fabs(p1) + fabs(q0) + fabs(q1) < LARGE)) return true;
    }
    const double pv = a11 * m20 + a01 * m21, pw = a00 * m21 + a01 * m20;
    if (!(pv + pw < LARGE)) return true;
    const double Ev = (G * pv + G64 * (a11 * s20 + a01 * s21) + TINY * (a11 + a01 + 2.0)) * ainv + TINY;
    const double Ew = (G * pw + G64 * (a00 * s21 + a01 * s20) + TINY * (a00 + a01 + 2.0)) * ainv + TINY;
    const double Eu = Ev + Ew + G * (1.0 + mv + mw);
    return !(vmax < -Ev || wmax < -Ew || umax < -Eu);
}

}  // namespace mr
