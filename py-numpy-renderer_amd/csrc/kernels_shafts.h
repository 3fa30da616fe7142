// kernels_shafts.h -- k_shaft_source, k_shaft_march, k_shaft_composite: light shafts (shafts_def.h has the definition).
// A frame with the pass runs three dependent launches.  Unlike every other gather of the library none of them stages a
// rectangle in LDS: a ray towards the light crosses the whole frame, so no halo bounds it.  The march's source S is built
// small enough to lie in an XCD's 4 MiB L2 -- at 1080p and a quarter of the resolution 480 x 270 samples of 16 bytes,
// 2.1 MB -- and is marched from there through the caches.
//
// On the device a sample of S and of R is 16 bytes, (r, g, b, 0): a tap's corner is one 16-byte load, four a tap, where
// three floats a sample would take twelve narrow ones.  mr_debug_light_shafts_post and the mirror hand out (H_d, W_d, 3).
//
// k_shaft_source<D>: mask, bright factor and the D-level tree in one launch; S_0 and the levels in between never exist in
// memory.  A thread owns one coarse sample, that is 2^D x 2^D samples of the grid, and lanes run along x: a wavefront's
// reads of one fine row are one contiguous run at D <= 2 (at D = 2, 48 bytes of F and 32 bytes of Z a lane, 3 KB and 2 KB a
// wavefront).  The tree is evaluated in registers as rows arrive (shaft_pairs): a row of the grid becomes its pair sums at
// once, two rows of pair sums a row of the next level.  At D = 3 and 4 a thread owns a column four samples wide and the
// two or four lanes of a group combine the upper levels across lanes (shaft_column), so that a wavefront's reads of a row
// stay one run: a thread that walked its own 8 x 8 block read 48-byte pieces 96 bytes apart and streamed at 3.0 TB/s
// where this streams at 6.0 TB/s.  26, 68, 76 and 80 registers at D = 1 .. 4, nothing in scratch.  Where the
// grid's width is a multiple of four samples every row starts on a 16-byte boundary and a lane's four samples are read
// with 16-byte loads (8-byte ones for the two samples of D = 1); other widths, and the lanes that straddle the right
// border, read sample by sample.  Rows and samples beyond the grid are the definition's +0.
//
// k_shaft_march: a thread per coarse sample, a wavefront an 8 x 8 block of them, so that the taps of its lanes stay near
// each other all the way to the light; a workgroup is four wavefronts, 16 x 16 samples.  The loop runs over the n taps;
// the weights are read from the kernel's arguments with a uniform index.  A ray that has left the level never comes back
// (shafts_def.h), so a wavefront stops at the first tap that is outside for all its lanes.
//
// k_shaft_composite streams F once, in place, with four taps of R a sample: the shape of k_bloom_composite.
//
// No LDS, no scratch, no atomics.  Compiled in shafts.hip, a translation unit and a code object of its own, like the other
// passes' kernels (kernels_accum.h).
#pragma once

#include "shafts_def.h"

namespace mr {

constexpr int SHAFT_SRC_TW = 64, SHAFT_SRC_TH = 4;      // the workgroup of k_shaft_source, in coarse samples, one a thread
constexpr int SHAFT_MARCH_T = 16;                       // k_shaft_march's workgroup: 16 x 16 coarse samples, 8 x 8 a wavefront
constexpr int SHAFT_COMP_TW = 64, SHAFT_COMP_TH = 4;    // k_shaft_composite's, a sample of the grid a thread

struct ShaftSrc {
    const float *__restrict__ frame;
    const double *__restrict__ zbuf;
    int w, h;
    int wide;                                           // rows start on 16-byte boundaries: w % 4 == 0 and both bases aligned
    float threshold;
};

// S_0 of one sample
__device__ __forceinline__ void shaft_s0(float r, float g, float b, double z, float t, float s[3])
{
    const float k = bloom_bright(r, g, b, t);
    const bool sky = shafts_sky(z);
    s[0] = sky ? r * k : 0.0f; s[1] = sky ? g * k : 0.0f; s[2] = sky ? b * k : 0.0f;
}

// S_0 of the M samples from x0 of row y of the grid; beyond the grid: +0
template <int M>
__device__ __forceinline__ void shaft_load_row(const ShaftSrc &a, int x0, int y, float s[M][3])
{
    static_assert(M == 2 || M == 4, "two samples at D = 1, else four at a time");
    if (y >= a.h) {
#pragma unroll
        for (int k = 0; k < M; ++k) s[k][0] = s[k][1] = s[k][2] = 0.0f;
        return;
    }
    const size_t at = (size_t)y * a.w + x0;
    if (a.wide && x0 + M <= a.w) {
        float f[M * 3];
        double z[M];
        if (M == 2) {
            const float2 *q = reinterpret_cast<const float2 *>(a.frame + at * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) { const float2 v = q[k]; f[2 * k] = v.x; f[2 * k + 1] = v.y; }
        } else {
            const float4 *q = reinterpret_cast<const float4 *>(a.frame + at * 3);
#pragma unroll
            for (int k = 0; k < M * 3 / 4; ++k) { const float4 v = q[k]; f[4 * k] = v.x; f[4 * k + 1] = v.y; f[4 * k + 2] = v.z; f[4 * k + 3] = v.w; }
        }
        const double2 *qz = reinterpret_cast<const double2 *>(a.zbuf + at);
#pragma unroll
        for (int k = 0; k < M / 2; ++k) { const double2 v = qz[k]; z[2 * k] = v.x; z[2 * k + 1] = v.y; }
#pragma unroll
        for (int k = 0; k < M; ++k) shaft_s0(f[3 * k], f[3 * k + 1], f[3 * k + 2], z[k], a.threshold, s[k]);
        return;
    }
#pragma unroll
    for (int k = 0; k < M; ++k) {
        if (x0 + k < a.w) {
            const float *q = a.frame + (at + k) * 3;
            shaft_s0(q[0], q[1], q[2], a.zbuf[at + k], a.threshold, s[k]);
        } else {
            s[k][0] = s[k][1] = s[k][2] = 0.0f;
        }
    }
}

// The pair sums of row `ly` of level L of the block whose sample (0, 0) of the grid is (x0, y0): N sums of the row's 2 N
// values.  A row of level L > 0 is shafts_quad of the pair sums of the rows 2 ly and 2 ly + 1 below it.
template <int L, int N>
__device__ __forceinline__ void shaft_pairs(const ShaftSrc &a, int x0, int y0, int ly, float p[N][3])
{
    float v[2 * N][3];
    if constexpr (L == 0) {
        shaft_load_row<2 * N>(a, x0, y0 + ly, v);
    } else {
        float lo[2 * N][3], hi[2 * N][3];
        shaft_pairs<L - 1, 2 * N>(a, x0, y0, 2 * ly, lo);
        shaft_pairs<L - 1, 2 * N>(a, x0, y0, 2 * ly + 1, hi);
#pragma unroll
        for (int k = 0; k < 2 * N; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[k][c] = shafts_quad(lo[k][c], hi[k][c]);
    }
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[j][c] = shafts_pair(v[2 * j][c], v[2 * j + 1][c]);
}

// The sample of level L <= 2 that lies over (x0, y0) of the grid: at most sixteen samples, straight-line code.
template <int L>
__device__ __forceinline__ void shaft_value(const ShaftSrc &a, int x0, int y0, float out[3])
{
    static_assert(L >= 1 && L <= 2, "deeper trees are spread over lanes: shaft_column");
    float lo[1][3], hi[1][3];
    shaft_pairs<L - 1, 1>(a, x0, y0, 0, lo);
    shaft_pairs<L - 1, 1>(a, x0, y0, 1, hi);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = shafts_quad(lo[0][c], hi[0][c]);
}

// Levels 3 and 4, E = 1 or 2 levels above a thread's 4 x 4 blocks.  A lane owns a column four samples wide and 4 << E high
// at (x0, y0); the 2^E lanes of a group stand side by side and form one sample of level 2 + E, which every one of them
// receives.  The column's halves are visited by a loop that stays a loop (unrolled, the scheduler gathers every load of
// the column in front of the sums); each half's value is added to the neighbour group's, left + right -- the sum is the
// same bits in both lanes -- and the last round leaves (row0 + row1) * 0.25: the definition's tree, its upper levels
// combined across lanes.  Every lane of the wavefront takes part: a lane beyond the grid loads the definition's +0.
template <int E>
__device__ __forceinline__ void shaft_column(const ShaftSrc &a, int x0, int y0, float out[3])
{
    if constexpr (E == 0) {
        shaft_value<2>(a, x0, y0, out);
    } else {
        float below[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll 1
        for (int by = 0; by < 2; ++by) {
            float v[3];
            shaft_column<E - 1>(a, x0, y0 + by * (4 << (E - 1)), v);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float row = shafts_pair(v[c], __shfl_xor(v[c], 1 << (E - 1)));
                out[c] = shafts_quad(below[c], row);
                below[c] = row;
            }
        }
    }
}

// dst: S, (dh x dw) = the grid (a.h x a.w) halved D times, 16 bytes a sample.  D <= 2: a thread a coarse sample, the grid
// is (dw, dh) over (SHAFT_SRC_TW, SHAFT_SRC_TH).  D = 3, 4: a thread a column of four samples, 2^(D-2) threads a coarse
// sample, the grid is (ceil(w / 4), dh) over the same block -- a wavefront's reads of a row are one run at every D.
template <int D>
__global__ void __launch_bounds__(SHAFT_SRC_TW * SHAFT_SRC_TH)
k_shaft_source(ShaftSrc a, float4 *__restrict__ dst, int dw, int dh)
{
    static_assert(D >= 1 && D <= SHAFTS_MAX_LEVELS, "the levels the description takes");
    static_assert(SHAFT_SRC_TW == 64, "a row of the block is one wavefront: a group's lanes are lanes of one wavefront, and a row beyond the level leaves whole");
    const int col = (int)blockIdx.x * SHAFT_SRC_TW + (int)threadIdx.x % SHAFT_SRC_TW;
    const int y = (int)blockIdx.y * SHAFT_SRC_TH + (int)threadIdx.x / SHAFT_SRC_TW;
    float s[3];
    if constexpr (D <= 2) {
        if (col >= dw || y >= dh) return;
        shaft_value<D>(a, col << D, y << D, s);
        dst[(size_t)y * dw + col] = make_float4(s[0], s[1], s[2], 0.0f);
    } else {
        constexpr int E = D - 2;
        if (y >= dh) return;                                   // (the whole wavefront)
        shaft_column<E>(a, col << 2, y << D, s);
        const int x = col >> E;
        if ((col & ((1 << E) - 1)) == 0 && x < dw) dst[(size_t)y * dw + x] = make_float4(s[0], s[1], s[2], 0.0f);
    }
}

// the four corners of a tap and their blend, three channels
__device__ __forceinline__ void shaft_fetch(const float4 *__restrict__ level, int w, const ShaftsTap &t, float v[3])
{
    const float4 *r0 = level + (size_t)t.y0 * w, *r1 = level + (size_t)t.y1 * w;
    const float4 a00 = r0[t.x0], a01 = r0[t.x1], a10 = r1[t.x0], a11 = r1[t.x1];
    v[0] = shafts_bilerp(a00.x, a01.x, a10.x, a11.x, t.fx, t.fy);
    v[1] = shafts_bilerp(a00.y, a01.y, a10.y, a11.y, t.fx, t.fy);
    v[2] = shafts_bilerp(a00.z, a01.z, a10.z, a11.z, t.fx, t.fy);
}

// src: S, dst: R, both (h x w), 16 bytes a sample
__global__ void __launch_bounds__(SHAFT_MARCH_T * SHAFT_MARCH_T)
k_shaft_march(const float4 *__restrict__ src, float4 *__restrict__ dst, int w, int h, ShaftsParams p)
{
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int x = (int)blockIdx.x * SHAFT_MARCH_T + (wave & 1) * 8 + (lane & 7);
    const int y = (int)blockIdx.y * SHAFT_MARCH_T + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const float cx = (float)x, cy = (float)y;
    const float dx = shafts_ray_delta(p.light_x, cx, p.step), dy = shafts_ray_delta(p.light_y, cy, p.step);
    float acc[3] = { 0.0f, 0.0f, 0.0f };
    for (int i = 0; i < p.samples; ++i) {
        ShaftsTap t;
        const bool inside = shafts_tap(shafts_ray_at(cx, dx, i), shafts_ray_at(cy, dy, i), w, h, t);
        if (!__any(inside)) break;                           // (no lane's ray comes back: shafts_def.h)
        float v[3];
        shaft_fetch(src, w, t, v);
        const float wi = p.weights[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = inside ? shafts_add(acc[c], wi, v[c]) : acc[c];
    }
    dst[(size_t)y * w + x] = make_float4(acc[0], acc[1], acc[2], 0.0f);
}

// frame (h x w) receives F + g * fetch(R, ...); coarse is R, (ch x cw)
__global__ void __launch_bounds__(SHAFT_COMP_TW * SHAFT_COMP_TH)
k_shaft_composite(float *__restrict__ frame, const float4 *__restrict__ coarse, int w, int h, int cw, int ch, float inv_scale, float gain)
{
    const int x = (int)blockIdx.x * SHAFT_COMP_TW + (int)threadIdx.x % SHAFT_COMP_TW;
    const int y = (int)blockIdx.y * SHAFT_COMP_TH + (int)threadIdx.x / SHAFT_COMP_TW;
    if (x >= w || y >= h) return;
    ShaftsTap t;
    (void)shafts_tap(shafts_coarse_at(x, inv_scale), shafts_coarse_at(y, inv_scale), cw, ch, t);      // (always inside)
    float v[3];
    shaft_fetch(coarse, cw, t, v);
    float *o = frame + ((size_t)y * w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = bloom_composite(o[c], gain, v[c]);
}

}  // namespace mr
