// tonemap_def.h -- tone mapping, an exposure metered from a luminance histogram of the frame and a tone curve: the
// definition, once, for the kernels (kernels_tonemap.h) and for the host mirror (host_tonemap.h), which both include this
// file; tests/tonemap_ref.py restates it in NumPy.  No kernel lives here: mi355rast.hip includes this header and its code
// object must not grow (kernels_accum.h says why).
//
// On the sample grid, with F the float frame in front of the pass (behind the bloom, in front of the overlay): F >= 0 and
// finite.  All arithmetic is float32 with every operation rounded on its own (-ffp-contract=off), or integer: no float
// atomics, no log, no exp -- the metered exposure does not depend on the order in which the samples are counted, and the
// host gets the device's bits.
//
//   luminance   Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b                      Y >= 0
//   bin         b = clamp((bits(Y) >> 20) - ((127 - 24) << 3), 0, 255)       8 bins a stop over 32 stops from 2^-24: the
//                                                                            exponent and three bits of the mantissa
//   histogram   n[i] = number of samples in bin i                            uint32; n[0] (black, below 2^-24) is metered
//                                                                            out: n[0] := 0
//   trim        N = sum n;  lo = N*low_pm / 1000;  hi = N*high_pm / 1000     integer
//               C_i = n[1] + .. + n[i-1];   u_i = max(0, min(C_i + n[i], hi) - max(C_i, lo))
//   centre      c_i = ((i >> 3) - 24) * 256 + FRAC[i & 7]                    1/256 stops; FRAC = {22, 63, 100, 134, 165, 193,
//                                                                            220, 244} = round(256*log2(1 + (m + 0.5)/8))
//   mean        S = sum u_i*c_i;  M = sum u_i   (int64);   q = floor((2S + M) / (2M))     floor division, S may be negative
//   target      -q = 256*a + f,  0 <= f < 256;   e_t = clamp(ldexpf(key * EXP2[f], a), min_exposure, max_exposure)
//   adapt       e = e_prev + speed * (e_t - e_prev)   where the scene has a previous exposure, else e = e_t
//               M == 0 (nothing metered): e = e_prev, else 1.0f
//   curve       x = F * e per channel;
//               linear    x
//               reinhard  (x * (1 + x / (white*white))) / (1 + x)
//               aces      min((x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f), 1)
//
// EXP2[f] = float32(2^(f/256)) comes with the description (the packer computes it in float64): kernel, mirror and
// reference read the same bits, and no exp2 runs anywhere.  With a fixed exposure nothing is metered and e is that value.
//
// What follows, and what the tests rely on:
//   * Scaling a frame by 2^k moves every sample 8k bins, q by 256k, and e_t by exactly 2^-k -- while no sample leaves
//     bins 1 .. 254 and the clamp is not hit.
//   * The half-bin centre is the meter's whole error against the geometric mean: at most 1/16 of a stop a sample.
//   * linear with e = 1 is the identity, bit for bit: x = F * 1.
//   * -q lies in -2036 .. 6081, so a lies in -8 .. 23: 2^a is a normal float32 and ldexpf is one product by it.
//   * Every count and sum is an integer.
#pragma once

#include <cmath>
#include <cstdint>

#include "ao_def.h"

namespace mr {

constexpr int TONE_BINS = 256;
constexpr int TONE_LINEAR = 0, TONE_REINHARD = 1, TONE_ACES = 2;
constexpr unsigned TONE_MAX_BLOCKS = 1024;               // the largest grid of k_lum_hist a caller may ask for: the slab's rows
constexpr unsigned TONE_HIST_BLOCKS = 256;               // its default cap (MR_TONEMAP_GRID)

// What k_exposure takes of the description: mr_tone_map_desc as float32, checked (host_tonemap.h, tone_params).
struct ToneMeter {
    float key, speed, min_exposure, max_exposure;
    int32_t low_pm, high_pm;
    float exp2[TONE_BINS];
};

// What the pass takes: the operator, the exposure where it is fixed, white*white (one float32 product), the meter.
struct ToneParams {
    int32_t op, fixed;
    float exposure, white2;
    ToneMeter meter;
    bool adaptive() const { return !fixed && meter.speed < 1.0f; }     // the one case that carries state from frame to frame
};

MR_AO_HD inline float tone_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// (the sign bit is masked: -0 is black, as +0 is)
MR_AO_HD inline int tone_bin(float y)
{
    const int b = (int)((__builtin_bit_cast(uint32_t, y) & 0x7fffffffu) >> 20) - ((127 - 24) << 3);
    return b < 0 ? 0 : (b > TONE_BINS - 1 ? TONE_BINS - 1 : b);
}

MR_AO_HD inline int tone_bin(float r, float g, float b) { return tone_bin(tone_luminance(r, g, b)); }

// the centre of bin i in 1/256 stops; FRAC as eight bytes, lowest first
MR_AO_HD inline int tone_centre(int i)
{
    const int frac = (int)((0xf4dcc1a586643f16ull >> (8 * (i & 7))) & 0xff);
    return ((i >> 3) - 24) * 256 + frac;
}

// u_i: how many of bin i's samples lie between the trims; c = C_i, n = n[i]
MR_AO_HD inline int64_t tone_kept(int64_t c, int64_t n, int64_t lo, int64_t hi)
{
    const int64_t top = c + n < hi ? c + n : hi, bottom = c > lo ? c : lo;
    return top > bottom ? top - bottom : 0;
}

// floor(a / b), b > 0
MR_AO_HD inline int64_t tone_floor_div(int64_t a, int64_t b)
{
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// ldexpf(v, a) for a in -126 .. 127: the product by 2^a
MR_AO_HD inline float tone_ldexp(float v, int a)
{
    a = a < -126 ? -126 : (a > 127 ? 127 : a);
    return v * __builtin_bit_cast(float, (uint32_t)(a + 127) << 23);
}

// e_t from the sums, M > 0
MR_AO_HD inline float tone_target(int64_t s, int64_t m, const ToneMeter &p)
{
    const int64_t nq = -tone_floor_div(2 * s + m, 2 * m);
    const int64_t a = tone_floor_div(nq, 256);
    const int f = (int)(nq - 256 * a);
    const float v = tone_ldexp(p.key * p.exp2[f], (int)a);
    return v < p.min_exposure ? p.min_exposure : (v > p.max_exposure ? p.max_exposure : v);
}

// e of a frame: from the sums, the meter and the scene's previous exposure where it has one
MR_AO_HD inline float tone_exposure(int64_t s, int64_t m, const ToneMeter &p, bool has_prev, float e_prev)
{
    if (m == 0) return has_prev ? e_prev : 1.0f;
    const float e_t = tone_target(s, m, p);
    return has_prev ? e_prev + p.speed * (e_t - e_prev) : e_t;
}

template <int OP>
MR_AO_HD inline float tone_curve(float f, float e, float white2)
{
    const float x = f * e;
    if (OP == TONE_LINEAR) return x;
    if (OP == TONE_REINHARD) return (x * (1.0f + x / white2)) / (1.0f + x);
    return fminf((x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f), 1.0f);
}

}  // namespace mr
