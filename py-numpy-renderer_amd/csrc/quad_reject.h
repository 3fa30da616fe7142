// quad_reject.h -- the depth rules of a shadow quad: per sample (quad_depth_pass), per rectangle of samples
// (quad_rect_verdict: k_tile's 16 x 4 strips), and per tile while binning (quad_tile_bound in k_bin_work, quad_tile_none
// in k_tile).  One copy of each.
//
// Plain C++: the kernels include it through kernels_bin.h, and tools/host_quad_cull_check.cpp compiles the very same
// functions for the CPU and holds the tile rule to the strip rule and to the per-sample rule.
//
// Why the tile rule changes no frame.  A quad's plane value t(x, y) = (nx x + ny y) + d is, as computed, monotone in x and
// in y (every step is a rounded monotone function of the one before), so over a rectangle of samples its extremes are at
// the four corner samples, and a tile's corner range contains the corner range of every strip inside it.  Everything
// quad_rect_bounds derives from that range is monotone in it and in the rectangle's far corner (xb, yb >= 0): the range
// of -t / nz (rounded products with one common factor), the slack (a larger range and a larger corner give a larger
// one), and so
//     den_hi(tile) >= den_hi(strip),   den_lo(tile) <= den_lo(strip),   sane(tile) => sane(strip).
// k_bin_work stores den_hi rounded UP to float32 (right-handed; den_lo rounded DOWN otherwise), which keeps the
// inequality, and k_tile compares against the most favourable covered z of the whole tile, which is no less favourable
// than any strip's.  The operands of the two products are positive where it matters and rounded products of positive
// operands are monotone:
//   right-handed   lo > zt * B.  zt > 0: every strip has z_strip <= zt and den_hi <= B, so z_strip * den_hi <= zt * B < lo
//                  (a strip with z_strip <= 0, or none covered: its product is <= 0 < lo).  zt <= 0: every strip's z is
//                  <= 0 and so is its product.  lo > 0 because sane holds (two_nf > 0).
//   left-handed    hi < zt * B needs zt > 0 (hi > 0); every strip has z_strip >= zt and den_lo >= B >= 0, so
//                  z_strip * den_lo >= zt * B > hi.
// So a tile-level `none` implies the strip-level `none` (with `sane`) in all four strips: k_tile would have rejected the
// quad in every wavefront, after staging and classifying it.  A bound that is not usable is stored as NaN, with which the
// comparison is false.
//
// That is the case of positive denominators, the only one the strip rule knows.  A right-handed camera's frames have
// negative ones throughout (z and the quads' depths are negative there): for those the tile rule carries the mirrored
// comparison (quad_rect_sane_neg, quad_tile_none with a negative bound), which answers for the per-sample rule itself --
// a culled quad is one the strips keep, walk, and find failing at every sample.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MR_QUAD_FN __device__ __forceinline__
#define MR_QUAD_ANY(x) __ballot(x)
#else
#define MR_QUAD_FN inline
#define MR_QUAD_ANY(x) (x)
#endif

namespace mr {

#if !defined(__HIPCC__)
// The kernels' approx_rcp (rast_math.h) is the hardware's estimate and two Newton steps: correct to an ulp or two.  The
// CPU check may put its own model here (a quotient pushed a few ulps either way).
#ifndef MR_QUAD_HOST_RCP
#define MR_QUAD_HOST_RCP(x) (1.0 / (x))
#endif
inline double approx_rcp(double x) { return MR_QUAD_HOST_RCP(x); }
#endif

// The depth rule of a shadow quad's sample (obj/triangular.py:351-360), the one copy both walks of phase 3 call: does
// the sample (dpx, dpy) of the quad with plane (q_nx, q_ny, nzq, q_d) pass against the pixel's final z?
// zq = two_nf / (f_plus_n + (t / nz) * f_minus_n) with t the plane's value at the sample.  The reference's value needs
// two IEEE divisions; the DECISION needs none: multiplied through by nz, zbest - zq has the sign of E / D with
// D = f_plus_n * nz + t * f_minus_n and E = zbest * D - two_nf * nz (a0 = f_plus_n * nz and b0 = two_nf * nz come with
// the staged record).  That settles it unless z-buffer and quad depth agree to nine digits or D is close to its pole
// (or something is not finite); only then is the exactly rounded expression evaluated.  t itself is computed exactly
// as the reference does.  Decisions stay bit-exact.  `in`: the lane holds a sample of the quad (the others' verdicts
// are not used).
MR_QUAD_FN bool quad_depth_pass(double q_nx, double q_ny, double nzq, double q_d, double a0, double b0,
                                double dpx, double dpy, double zbest, bool rh, bool in,
                                double f_plus_n, double f_minus_n, double two_nf)
{
    const double t = (q_nx * dpx + q_ny * dpy) + q_d;
    const double tf = t * f_minus_n;
    const double den = a0 + tf;
    const double prod = zbest * den;
    const double e = prod - b0;
    // an empty z-buffer entry (+-inf) beats or loses against every finite depth
    const bool zinf = fabs(zbest) == INFINITY;
    bool pass = zinf ? (rh ? zbest > 0 : zbest < 0) : (rh ? ((e > 0) == (den > 0)) : ((e < 0) == (den > 0)));
    const bool clear = zinf || fabs(e) > 1e-9 * (fabs(prod) + fabs(b0));
    const bool unsure = in && !(clear && fabs(den) > 2e-4 * (fabs(a0) + fabs(tf)));
    if (MR_QUAD_ANY(unsure)) {
        if (unsure) {
            const double z = two_nf / (f_plus_n - (-t / nzq) * f_minus_n);     // linearize_z (obj/core.py:226-228)
            pass = rh ? (zbest >= z) : (zbest <= z);
        }
    }
    return pass;
}

// Depth bounds of a quad over the rectangle of samples [xa, xb] x [ya, yb].  The quad's plane depth is affine over the
// screen, so over the rectangle -t/nz is extreme at a corner, and linearize_z is monotone while its denominator stays
// positive: with 0 < den_lo <= den <= den_hi over the rectangle (bounds pushed outwards by a slack that dwarfs the
// rounding of the per-pixel expression and of the approximate reciprocal used here) the depth two_nf / den lies in
// [two_nf / den_hi, two_nf / den_lo], and comparisons against it are decided without dividing.
struct QuadRectBounds { double den_lo, den_hi, inz; };
MR_QUAD_FN QuadRectBounds quad_rect_bounds(double nx, double ny, double nz, double d, double xa, double xb, double ya, double yb,
                                           double f_plus_n, double f_minus_n)
{
    const double t00 = (nx * xa + ny * ya) + d, t10 = (nx * xb + ny * ya) + d;
    const double t01 = (nx * xa + ny * yb) + d, t11 = (nx * xb + ny * yb) + d;
    const double tmin = fmin(fmin(t00, t10), fmin(t01, t11)), tmax = fmax(fmax(t00, t10), fmax(t01, t11));
    const double inz = approx_rcp(nz);
    const double za = -tmin * inz, zb = -tmax * inz;
    const double slack = 1e-12 * fmax(fabs(za), fabs(zb)) +
                         1e-15 * ((fabs(nx) * xb + fabs(ny) * yb) + fabs(d)) * fabs(inz);
    const double zs_lo = fmin(za, zb) - slack, zs_hi = fmax(za, zb) + slack;
    QuadRectBounds b;
    b.den_lo = f_plus_n - zs_hi * f_minus_n; b.den_hi = f_plus_n - zs_lo * f_minus_n; b.inz = inz;
    return b;
}
// ... which holds only while this does.  `fpn` is f_plus_n and `tnf` two_nf again (k_tile hands over copies the compiler
// cannot trace, see there).
MR_QUAD_FN bool quad_rect_sane(const QuadRectBounds &b, double nz, double f_minus_n, double two_nf, double fpn)
{
    return two_nf > 0 && f_minus_n > 0 && b.den_lo > 1e-9 * fpn && nz != 0 &&
           fabs(b.inz) < 1e300 && b.den_hi < 1e300;
}

// The verdicts for the whole rectangle, against its most (zlim) and least (zhard) favourable covered z:
//   all pass: even the quad's least favourable depth passes against the least favourable covered z of the rectangle
//             (uncovered pixels pass anyway: their z is +-inf) -> the per-pixel depth arithmetic is skipped, the verdict
//             is the same;
//   none can: (used only when the frame is all that is asked for, no MR_FRAME_COUNTERS: the stencil matters where a
//             triangle was drawn) even its most favourable depth loses against the most favourable covered z -> the
//             quad is skipped.
// Both hold only with quad_rect_sane.  rh: a pixel passes when zbuf >= zq; lh: when zbuf <= zq.
struct QuadRectVerdict { bool none, all; };
MR_QUAD_FN QuadRectVerdict quad_rect_verdict(const QuadRectBounds &b, double tnf, double zlim, double zhard, bool rh)
{
    const double lo = tnf * (1.0 - 1e-12), hi = tnf * (1.0 + 1e-12);
    QuadRectVerdict v;
    v.none = rh ? lo > zlim * b.den_hi : hi < zlim * b.den_lo;
    v.all = rh ? hi <= zhard * b.den_lo : lo >= zhard * b.den_hi;
    return v;
}

// ---- the same rule for a whole tile, split between the kernel that lists the quad and the one that walks it

// x rounded to float32 away from zero or towards it; NaN where the result would not be a normal float32
MR_QUAD_FN float quad_bound_f32(double x, bool away)
{
    const double m = fabs(x);
    if (!(m >= 0x1p-100 && m <= 0x1p100)) return NAN;
    float f = (float)m;
    uint32_t bits;
    memcpy(&bits, &f, 4);
    if (away ? (double)f < m : (double)f > m) bits += away ? 1u : 0xffffffffu;      // the neighbour on the far side of m
    memcpy(&f, &bits, 4);
    return x < 0 ? -f : f;
}

// The mirrored case of quad_rect_sane: every denominator of the rectangle is negative (the depth two_nf / den is then
// negative and still lies in [two_nf / den_hi, two_nf / den_lo]: 1 / den falls on either side of its pole).  The frames
// of a right-handed camera are of this kind: there z and the quads' depths are negative.
MR_QUAD_FN bool quad_rect_sane_neg(const QuadRectBounds &b, double nz, double f_minus_n, double two_nf, double fpn)
{
    return two_nf > 0 && f_minus_n > 0 && b.den_hi < -1e-9 * fpn && nz != 0 &&
           fabs(b.inz) < 1e300 && b.den_lo > -1e300;
}

// k_bin_work, for a quad it lists in the tile whose first sample is (gx, gy): the bound over the tile's tile_w x tile_h
// samples that quad_tile_none compares against, rounded to float32 so that the comparison can only get harder to win.
//   quad_rect_sane      den_hi (right-handed) or den_lo, positive: the strip rule's own comparison, see the top;
//   quad_rect_sane_neg  den_hi (right-handed) or den_lo, NEGATIVE -- the sign says which comparison applies;
//   neither             NaN: every comparison is false.
MR_QUAD_FN float quad_tile_bound(double nx, double ny, double nz, double d, int gx, int gy, int tile_w, int tile_h,
                                 double f_plus_n, double f_minus_n, double two_nf, bool rh)
{
    const QuadRectBounds b = quad_rect_bounds(nx, ny, nz, d, (double)gx, (double)(gx + tile_w - 1), (double)gy, (double)(gy + tile_h - 1),
                                              f_plus_n, f_minus_n);
    if (quad_rect_sane(b, nz, f_minus_n, two_nf, f_plus_n)) return quad_bound_f32(rh ? b.den_hi : b.den_lo, rh);
    if (quad_rect_sane_neg(b, nz, f_minus_n, two_nf, f_plus_n)) return quad_bound_f32(rh ? b.den_hi : b.den_lo, !rh);
    return NAN;
}

// k_tile: can no sample of the tile pass?  zt: the most favourable covered z of the tile (the largest in a
// right-handed frame, the smallest otherwise).
//   bound > 0: the comparison of quad_rect_verdict's `none`, with the stored bound.
//   bound < 0: every depth of the quad over the tile is negative and no smaller than two_nf / den_hi (no larger than
//     two_nf / den_lo).  Right-handed, a sample passes when zbuf >= zq: none can when zt < two_nf / den_hi, which
//     multiplied by den_hi < 0 is zt * den_hi > two_nf; a bound rounded towards zero makes the product of two negative
//     numbers smaller, and zt >= 0 never culls.  Left-handed, a sample passes when zbuf <= zq: none can when
//     zt > two_nf / den_lo, that is zt * den_lo < two_nf; a bound rounded away from zero makes the product larger, and
//     zt >= 0 is above every negative depth.  The strip rule knows no such case (it keeps these quads and the walk finds
//     that every sample fails): this verdict answers for the per-sample rule directly, with the margins of the other
//     one, and tools/host_quad_cull_check.cpp holds it to quad_depth_pass at every sample.
MR_QUAD_FN bool quad_tile_none(float bound, double zt, double tnf, bool rh)
{
    const double lo = tnf * (1.0 - 1e-12), hi = tnf * (1.0 + 1e-12);
    const double prod = zt * (double)bound;
    if (bound < 0) return rh ? prod > hi : prod < lo;
    return rh ? lo > prod : hi < prod;
}

}  // namespace mr
