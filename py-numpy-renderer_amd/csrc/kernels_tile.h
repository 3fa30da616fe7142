// kernels_tile.h -- the tile kernel: everything between the tile lists and the finished pixels.
//
// Design (MI355X-first, not a port of the reference's per-face loops): the frame is cut into
// 16x16-pixel tiles; one 256-thread workgroup owns one tile from the first triangle to the uint8
// pixels.  The tile's z-buffer and winner map live in LDS, each pixel's stencil count in a
// register of the thread that owns the pixel, so the frame's z / stencil / float colour -- the
// buffers the reference's three loops hammer (obj/core.py:588-591) -- never exist in HBM unless a
// caller asks to read them back.  Measured on MI355X (tools/micro/atomic_bench.hip): scattered
// 64-bit global atomics run at 24 G/s, LDS atomics at 1 900 G/s.
//
// Phases of a tile (k_tile):
//   1. big (triangle, tile) pairs -- a floor triangle -- one PIXEL per thread, the records staged
//      64 at a time in LDS and read as broadcasts (obj/triangular.py:72-118);
//   2. small pairs -- a dense mesh's triangles cover a handful of samples -- four lanes per
//      TRIANGLE (two where the tile lists more than a round of those, eight where at most half a round): they share out
//      the few samples of the pixel box and do an LDS atomicMin on the order-preserving key of z, appending key, pixel
//      and face of every covered sample to the lane's log in LDS (PairLog); then (second sweep, behind a barrier) an LDS
//      atomicMax of the face index for the logged keys that equal the tile's final z -- no record, no barycentrics, no
//      depth; only a lane whose log ran over walks its pairs again, from the sample that did not fit
//      (MR_PAIR_LOG=0 .. 4 sets the log's capacity, 0 for none; mr_debug_pair_log counts both).  The reference's
//      sequential rule (a fragment writes when zbuf >= z, so the last face in order wins ties) is reproduced
//      order-free: smallest z, and among equal z the largest face index;
//   3. the tile's shadow quads against the final z, QUAD_BATCH records staged in LDS per round -- in the frame-only
//      single-light kernels only the quads that k_bin_work's depth bound lets pass against the tile's most favourable
//      covered z (quad_tile_none, quad_reject.h; MR_QUAD_TILE_CULL=0 stages them all), and a tile none of whose quads
//      can pass skips the phase; lane j of every wavefront classifies quad j against the wavefront's 16x4 strip.  A survivor is then walked in one of two ways
//      (obj/triangular.py:335-368): the STRIP walk, one quad at a time, every lane its own pixel, stencil +-1 in the
//      lane's register; or -- single light, where enough of the strip's quads are crossed by an edge -- the SPAN walk:
//      (quad, row) items dealt to the lanes, sixteen quads to a round, the row's samples found as one interval by
//      bisection with the strip walk's own rounded edge expression, stencil +-1 as LDS atomics on the pixel's word (the
//      winner map's, dead by then), read back once behind the last batch.  One depth rule for both (quad_depth_pass).
//      MR_QUAD_WALK=strips | spans forces either; mr_debug_quad_walks counts them;
//   4. deferred shading of the winner (kernels_shade.h), finalise, uint8 store.
//
// A frame with several lights (k_tile<., ., true>) keeps one stencil count per light in phase 3 and adds the
// lights' colours in phase 4; see the kernel's ML parameter.
//
//   k_reduce_tile_stats   sums the per-tile fragment counts (only when statistics are asked for)
#pragma once

#include "kernels_bin.h"
#include "kernels_shade.h"
#include "rast_resolve.h"

namespace mr {

// Order-preserving key of a non-NaN double: unsigned comparison of keys == comparison of values.
__device__ __forceinline__ unsigned long long z_key(double z)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(z);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double z_unkey(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// Coverage and depth of a sample as the tile kernel's pair loops evaluate them.  The reference's (N,K)@(K,) products
// round in one of two orders (rows_dot2 / rows_dot3 in rast_math.h: a dot for one row, a gemv for more), chosen per face
// by TF_SINGLE_BOX and TF_SINGLE_Z.  Evaluating both and selecting cost four float64 operations and four selects per
// sample on top of the four that count, and two and two more per depth; here the ORDER is folded into the operands,
// once per (lane, triangle):  gemv2(a0, a1, b0, b1) = chain2(a1, a0, b1, b0) and gemv3(a0, a1, a2, ...) =
// chain3(a1, a0, a2, ...), so one chain serves both with the first two operand pairs swapped.  Same operations on the
// same values as tri_bary / rows_dot3: bit-identical.  MAYBE_SINGLE == false: the caller knows neither flag is set.
template <bool MAYBE_SINGLE>
struct PairMath {
    double a0, a1, p0, p1, q0, q1, k0, k1, k2;
    float d00, d01, d11, inv_den;
    bool sbox, sz;
    __device__ __forceinline__ explicit PairMath(const TriRec &t)
    {
        sbox = MAYBE_SINGLE && (t.flags & TF_SINGLE_BOX) != 0;
        sz = MAYBE_SINGLE && (t.flags & TF_SINGLE_Z) != 0;
        a0 = sbox ? t.ax : t.ay;   a1 = sbox ? t.ay : t.ax;
        p0 = sbox ? t.v0x : t.v0y; p1 = sbox ? t.v0y : t.v0x;
        q0 = sbox ? t.v1x : t.v1y; q1 = sbox ? t.v1y : t.v1x;
        k0 = sz ? t.zl0 : t.zl1;   k1 = sz ? t.zl1 : t.zl0;   k2 = t.zl2;
        d00 = t.d00; d01 = t.d01; d11 = t.d11; inv_den = t.inv_den;
    }
    // tri_bary (obj/transformation.py:18-31) at the sample (x, y), given widened to double
    __device__ __forceinline__ void bary(double x, double y, float &u, float &v, float &w) const
    {
        const double r0 = (sbox ? x : y) - a0, r1 = (sbox ? y : x) - a1;
        const float d20 = (float)fma(r1, p1, r0 * p0);
        const float d21 = (float)fma(r1, q1, r0 * q0);
        v = (d11 * d20 - d01 * d21) * inv_den;
        w = (d00 * d21 - d01 * d20) * inv_den;
        u = 1.0f - v - w;
    }
    __device__ __forceinline__ void bary(int x, int y, float &u, float &v, float &w) const
    {
        bary((double)(sbox ? x : y), (double)(sbox ? y : x), true, u, v, w);
    }
    // bar @ zlin (obj/triangular.py:97)
    __device__ __forceinline__ double depth(float u, float v, float w) const
    {
        const float m0 = sz ? u : v, m1 = sz ? v : u;
        return fma((double)w, k2, fma((double)m1, k1, (double)m0 * k0));
    }
private:
    __device__ __forceinline__ void bary(double c0, double c1, bool, float &u, float &v, float &w) const   // operands in chain order already
    {
        const double r0 = c0 - a0, r1 = c1 - a1;
        const float d20 = (float)fma(r1, p1, r0 * p0);
        const float d21 = (float)fma(r1, q1, r0 * q0);
        v = (d11 * d20 - d01 * d21) * inv_den;
        w = (d00 * d21 - d01 * d20) * inv_den;
        u = 1.0f - v - w;
    }
};

// One small (triangle, tile) pair shared by SMALL_LANES neighbouring lanes: the samples of the
// pixel box that lie in the tile are dealt to them round-robin (a tile of a dense mesh lists
// 50-200 such pairs of 1-24 samples each; one lane per pair left three of the four wavefronts
// idle behind long serial walks).  SWEEP 0: atomicMin/Max of z into the tile's LDS z-buffer.
// SWEEP 1: the same samples again; where this face's z is the final z, atomicMax of the face
// index.  Pairs that need the per-fragment clip test never come here (pair_class).
constexpr int SMALL_LANES = 4;

// What a lane's first sweep leaves for its second (see the winners' sweep in k_tile): a log of the samples it covered
// -- z key, pixel and face of every sample that had a depth, in the order it met them, through all its rounds.  A lane
// covers little more than one sample per pair whatever it walks, so PAIR_LOG_K entries answer for nearly all of them
// (the bench torus, tools/sim_pair_log.py: all but 0.04 % of the samples walked; three entries would leave 0.7 %, and
// then most wavefronts still hold a lane that walks again: measured, profiles/pair_log_ab.txt).  Pixel (bits 0..7) and
// face (bits 8..) share a word, which is what lets four entries fit the staging area: a scene with more than
// PAIR_LOG_MAX_FACE faces gets capacity 0 from the host.  The first sample that does not fit fixes where the lane
// walks again from: `resume`, the lane's round in bits 8.. and the walk position inside that pair below (a pair has at
// most TILE_PX / 2 samples per lane); nothing later of the lane is logged.  Entry e of thread t is at [e][t] of each
// array: a wavefront's accesses fall on distinct banks whatever entry each lane is at.
constexpr int PAIR_LOG_K = 4;
constexpr uint32_t PAIR_LOG_NONE = 0xffffffffu, PAIR_LOG_MAX_FACE = 1u << 24;
struct PairLog {
    unsigned long long (*key)[TILE_PX];
    uint32_t (*word)[TILE_PX];        // pixel | face << 8
    uint32_t n, cap;                  // entries written; entries the lane may write (TileArgs::pair_log; 0 once it met a face that writes no z)
    uint32_t resume;                  // PAIR_LOG_NONE: everything so far is in the log
};

// the frame's limits a tile clamps its pixel boxes to (values, not the frame constants: see kernargs())
struct TileBounds { int width, band_y0, band_y1; };

// SWEEP 0: every sample that has a depth goes to `log` (thread `tid`'s) where the atomic on its key is; returns the walk
// position of the pair's first sample that did not fit (PAIR_LOG_NONE: all did).  A select, not a branch, and the resume
// point is put together once per pair by the caller: every level of divergent control flow inside the walk holds a pair
// of scalar registers, and the multi-light general kernel has none to spare.  SWEEP 1: skips
// the lane's first `first` samples (the log answered for them), and counts the samples it walks in `frags` (COUNT; SWEEP 0: the fragments).
// FULL == false (a frame-only kernel, see tile_body): no fragment count, and no face of a depth_test == False model.
template <int SWEEP, bool FULL, bool COUNT = FULL>
__device__ __forceinline__ uint32_t small_pair(const TileBounds &tb, const TriRec &t, int gx, int gy, bool rh,
                                           unsigned long long *s_key, int *s_win, int sub, int lanes, unsigned int &frags,
                                           PairLog *log = nullptr, int tid = 0, int first = 0)
{
    const int x0 = max((int)t.x0, gx), x1 = min((int)t.x1, min(gx + TILE_W, tb.width));
    const int y0 = max(max((int)t.y0, gy), tb.band_y0), y1 = min(min((int)t.y1, gy + TILE_H), tb.band_y1);
    const PairMath<true> pm(t);
    // Model.depth_test == False (obj/triangular.py:117): the face's fragments are tested, never written to z.
    // The pixel then shows the LAST face in order among those that pass against the final z (see k_tile).
    const bool nodepth = FULL && ((t.flags >> 8) & FF_NO_DEPTH) != 0;
    const int bw = x1 - x0;
    uint32_t over = PAIR_LOG_NONE;
    // a face that writes no z is never logged: the lane walks again from its first such pair at the latest
    if (SWEEP == 0 && nodepth) { log->cap = 0; over = 0; }
    if (bw <= 0) return over;
    int px = x0 + sub, py = y0;
    while (px >= x1) { px -= bw; ++py; }
    int walked = 0;
    while (py < y1) {
        if (SWEEP == 0 || walked >= first) {
            float u, v, w;
            pm.bary(px, py, u, v, w);
            bool ok = u >= 0 && v >= 0 && w >= 0;
            if (COUNT) frags += SWEEP == 0 ? (ok ? 1u : 0u) : 1u;
            if (ok && (SWEEP == 1 || !nodepth)) {
                const double z = pm.depth(u, v, w);
                if (z == z) {                            // a NaN depth never passes the reference's test
                    const int p = (py - gy) * TILE_W + (px - gx);
                    const unsigned long long k = z_key(z);
                    if (SWEEP == 0) {
                        if (rh) atomicMin(&s_key[p], k); else atomicMax(&s_key[p], k);
                        const bool fits = log->n < log->cap;
                        over = fits ? over : min(over, (uint32_t)walked);
                        if (fits) {
                            log->key[log->n][tid] = k; log->word[log->n][tid] = (uint32_t)p | ((uint32_t)t.face << 8);
                            ++log->n;
                        }
                    } else if (nodepth ? (rh ? k <= s_key[p] : k >= s_key[p]) : s_key[p] == k) {
                        atomicMax(&s_win[p], t.face);
                    }
                }
            }
        }
        ++walked;
        px += lanes;
        while (px >= x1) { px -= bw; ++py; }
    }
    return over;
}

// Row of the device's output buffer that screen row py (in local tile row l) lands in.  A band of
// rows is stored top row first (the flip of obj/core.py:640).  In the striped layout (multi-GPU,
// interleaved tile rows) every device's buffer holds out_tile_rows blocks of TILE_H rows, its
// highest tile row first, rows inside a block top-down; the host un-permutes after the all-gather.
__device__ __forceinline__ int out_row(const FrameConst &fc, int py, int l)
{
    if (fc.out_tile_rows > 0)
        return (fc.out_tile_rows - 1 - l) * TILE_H + (tile_row_frame(fc, l) * TILE_H + TILE_H - 1 - py);
    return fc.band_y1 - 1 - py;
}

// ---- supersampling (MR_FRAME_SUPERSAMPLE2/4; FrameConst::ss_mode): the tile works on the sample grid, and output
// pixel (x, y) is the mean of samples (s x + i, s y + j), i, j < s.  s divides the tile, so every block of s x s samples
// lies inside one tile, and width / band are multiples of s, so a block is entirely inside the band or entirely out.
// The block's s * s colours are summed in ONE fixed order -- row-major from its bottom-left sample -- by the fused
// resolve below, k_resolve_touched and k_resolve_full alike, so the three give the same bytes.
// Output row of the block whose bottom-left sample is screen row py (band rows top first, like out_row).
__device__ __forceinline__ uint8_t *ss_out_pixel(uint8_t *out, int width, int band_y1, int shift, int px, int py)
{
    return out + ((size_t)((band_y1 - 1 - py) >> shift) * (width >> shift) + (px >> shift)) * 3;
}
// (ss_block_mean, the block's mean: rast_resolve.h)
// The fused resolve: the tile's 256 sample colours are staged in LDS (s_rgb, 3 floats per sample, row-major from the
// tile's bottom row); (16 / s)^2 threads each finalise one output pixel.  Call after the barrier behind the staging.
__device__ __forceinline__ void ss_resolve_tile(const FrameConst &fc, const float *s_rgb, uint8_t *out, int gx, int gy, int tid,
                                                const float *s_gamma)
{
    const int shift = fc.ss_mode & SS_SHIFT_MASK, n_log = 4 - shift;      // TILE_W == 16: (16 / s) blocks per side
    static_assert(TILE_W == 16 && TILE_H == 16, "ss_resolve_tile");
    if (tid >= 1 << (2 * n_log)) return;
    const int bx = tid & ((1 << n_log) - 1), by = tid >> n_log;
    const int px = gx + (bx << shift), py = gy + (by << shift);
    if (px >= fc.width || py < fc.band_y0 || py >= fc.band_y1) return;
    float m[3];
    ss_block_mean(s_rgb + ((by << shift) * TILE_W + (bx << shift)) * 3, TILE_W * 3, shift, m);
    uint8_t *o = ss_out_pixel(out, fc.width, fc.band_y1, shift, px, py);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = gamma_u8(m[c], s_gamma);
}

constexpr int QUAD_STAGE_U4 = 12;     // uint4 pieces staged per quad: 64-byte header + 4 edges
static_assert(offsetof(QuadRec, e) == 64 && sizeof(QuadEdge) == 32, "QuadRec layout");
static_assert(QUAD_BATCH == WAVE, "lane j of every wavefront classifies quad j of the batch");

struct QuadHead {                     // the first 64 bytes of a QuadRec, as staged
    double nx, ny, nz, d;
    int16_t x0, x1, y0, y1;
    int32_t n, is_front, edge;
    uint32_t pad[3];
};
static_assert(sizeof(QuadHead) == 64, "QuadHead mirrors QuadRec's header");

// How phase 3 of k_tile walks a quad (TileArgs::quad_walk, MR_QUAD_WALK).
enum : uint32_t { QUAD_WALK_AUTO = 0, QUAD_WALK_STRIPS = 1, QUAD_WALK_SPANS = 2 };
// auto: a (quad, strip) pair takes the span walk when at least this many of its edges cross the strip (0 would send
// the fat pairs too, whose every sample is inside: each row is then a loop of sixteen samples in one lane) ...
#ifndef MR_SPAN_MIN_EDGES
#define MR_SPAN_MIN_EDGES 1
#endif
// ... and the wavefront's strip has at least this many such quads in the batch: a round of spans costs what a few
// strip walks do, whatever it holds.  Both from the A/B in profiles/quad_spans_ab.txt (c4 / c3, quoted regime, MI355X:
// edges 1 / quads 6: 0.0782 / 0.0891 ms; 2 / 3: 0.0790 / 0.0924; 3 / 2: 0.0868 / 0.0950; 1 / 12: 0.0790 / 0.0892; the
// strip walk alone: 0.0905 / --).  A function of the batch's records and the strip, not of timing.
#ifndef MR_SPAN_MIN_QUADS
#define MR_SPAN_MIN_QUADS 6
#endif

// (quad_depth_pass, the depth rule of a shadow quad's sample both walks of phase 3 call: quad_reject.h)

constexpr int MAT_LDS = 8;            // scenes with up to this many materials keep them in LDS
static_assert(sizeof(Material) % 8 == 0 && MAT_LDS * sizeof(Material) / 8 <= TILE_PX, "material staging");

// Heaviest tiles first.  A tile under the mesh AND its shadow volume takes 10-80x the time of a floor
// tile.  In plain row-major order such tiles start in the middle of the launch and finish 40 us after
// everything else, and even with only the heaviest moved to the front the launch ended on the 10-20 us
// tiles that happened to start last.  Frames of a sequence resemble each other, so every tile leaves the
// class of its estimated cost (one byte, a plain store) for the slot's NEXT frame, whose k_bin_work sorts
// the tiles by class (order_tiles_block in kernels_bin.h: a counting sort in one workgroup, beside the
// binning) and whose tile workgroup b renders entry b of that order: longest-processing-time first.  The
// order is a permutation of the tiles by construction, and a grid with any tile of unknown class (a first
// frame, a new tile grid) is rendered in row-major order: a stale history costs time, never correctness.
// (A loop "list entry, then own tile" inside one workgroup doubled the kernel's register budget -- the
// compiler hoists the frame constants' register copies out of it; per-class lists appended to with atomics
// held every workgroup for the 2 us of a device-scope atomic's round trip: 82 -> 119 us.)
// cost thresholds of classes 1..7 (tile_cost units, ~0.1 us); the rest is class 8
#ifndef MR_CLASS_SCALE
#define MR_CLASS_SCALE 100            // per cent: tools/ab.sh "-DMR_CLASS_SCALE=70" ... moves all seven limits at once
#endif
__device__ __forceinline__ int tile_class(uint32_t cost)
{
    const uint32_t c = cost * 100u / (uint32_t)MR_CLASS_SCALE;
    return c >= 500u ? 1 : c >= 350u ? 2 : c >= 250u ? 3 : c >= 170u ? 4 : c >= 110u ? 5 : c >= 70u ? 6 : c >= 40u ? 7 : 8;
}
static_assert(ORDER_CLASSES == 8, "tile_class");
// On a device that owns few tiles (a rank of a multi-GPU split: all its tiles are resident at once and
// the launch lasts as long as its slowest tile) the heaviest class is not only started first: those
// tiles' shadow quads -- walked one after the other, up to a hundred and more where a mesh's
// outline and its shadow volume overlap -- are SHARED OUT over HEAVY_SPLIT workgroups.  Each of them
// rasterises the tile (same lists, same order-free arithmetic: the same z and winners), counts its share
// of the quads, and leaves its stencil counts in a scratch slot; the workgroup that arrives last (a
// counter, no waiting) adds the others' and shades.  Only frames rendered for the frame's sake are split
// (no MR_FRAME_COUNTERS), and only in the k_tile<true> instantiation: on a device that owns the whole
// frame the launch is bound by the tiles' total work, which the repeated rasterisation only adds to
// (measured on MI355X in round 2, c4: 86 -> 90 us whole frame; a rank of 8: 56 -> 38 us).  Round 3: with the
// heaviest tiles started first a whole frame's launch lasts exactly as long as its single heaviest tile (c4:
// 63.7 of 64.4 us, 46 of them its 111 shadow quads), so a lone whole frame now shares out its few heaviest tiles
// too -- a dozen on c4, chosen by a higher threshold (TileArgs::split_cost / split_quads) -- and nothing else.
#ifndef MR_HEAVY0_MAX
#define MR_HEAVY0_MAX 128
#endif
constexpr int HEAVY_SPLIT = 4, HEAVY0_MAX = MR_HEAVY0_MAX;
#ifndef MR_TILE_WAVES
#define MR_TILE_WAVES 5
#endif
constexpr int K_TILE_WAVES = MR_TILE_WAVES;              // wavefronts per SIMD the multi-light tile kernel's register budget allows
#ifndef MR_TILE_WAVES_1L
#define MR_TILE_WAVES_1L 6
#endif
constexpr int K_TILE_WAVES_1L = MR_TILE_WAVES_1L;        // ... and the single-light instantiations': 80 registers, held by tests/test_kernel_budget.py
constexpr int SPLIT_FRONT = HEAVY_SPLIT * HEAVY0_MAX;     // extra workgroups of a k_tile<true> launch

// estimated cost of a tile in ~0.1 us from its list lengths: the least-squares fit of the measured tile times of
// c4 on MI355X with six wavefronts per SIMD, 20.1 + 1.63 small + 29.8 big + 3.19 quads (tools/diag_tiles.py), rounded
__device__ __forceinline__ uint32_t tile_cost(uint32_t n_small, uint32_t n_big, uint32_t n_quad)
{
    return 20u + 2u * n_small + 30u * n_big + 3u * n_quad;
}

struct TileArgs {
    const TriClip *clips;
    const QuadRec *quads;
    uint32_t *bin_count;          // cursors = list lengths; zeroed again at the end of the tile
    const uint32_t *items[BIN_CLASSES];
    uint32_t cap[BIN_CLASSES];
    uint32_t pair_log;            // 0 .. PAIR_LOG_K: MR_PAIR_LOG, the entries a lane's log may hold (phase 2).  (In the hole behind cap[]: the
                                  // arguments behind it stay where they were, and with them how the kernels' scalar loads group.)
    const uint8_t *tap_mask;      // [tiles of the whole frame] or null: only the tiles marked here write the taps below (the overlay's tiles)
    double *zbuf;                 // optional taps (MR_FRAME_KEEP_BUFFERS): may be null
    int32_t *winner, *stencil;
    uint32_t *tile_stats;
    Counters *ctr, *next_ctr;     // this frame's counters; the next frame's (cleared here)
    Sticky *sticky;               // overflow verdicts of the slot's earlier frames (see Sticky)
    int32_t *split_sten;          // [HEAVY0_MAX][HEAVY_SPLIT][TILE_PX] stencil counts of a split tile's parts, then [HEAVY0_MAX][HEAVY_SPLIT] counts of the quads they staged
    uint32_t *split_arrive;       // [HEAVY0_MAX] parts that have left theirs (zero between frames)
    const uint32_t *order;        // ORDER_HEAD words, then the tiles in the order to render them (k_bin_work); null: row-major
    uint8_t *tile_class;          // [n_tiles] what this frame leaves for the next: 1 + the tile's cost class
    uint32_t split_cost, split_quads;   // k_tile<true>: a tile this costly, with this many shadow quads, is shared out next frame ...
    uint32_t split_max;                 // ... if no more than this many are (<= HEAVY0_MAX)
    uint32_t quad_walk;                 // QUAD_WALK_*: MR_QUAD_WALK (single-light instantiations, phase 3)
    const float *quad_bound;            // [n_tiles * cap[2]] beside items[2]: k_bin_work's quad_tile_bound of every listed quad
    uint32_t quad_cull;                 // MR_QUAD_TILE_CULL: bit 0, the frame-only single-light kernels drop a tile's quads by that bound (phase 3);
                                        // bit 1, they leave the number they staged in word 8 of the tile's record
};

// A frame with several lights (k_tile<., ., true>): the lights (all of them, FrameLights) and the stencil taps of
// lights 1.. (light 0's is TileArgs::stencil).  Behind everything else, like SetupKernArgs::lights.
struct TileLights {
    FrameLights lights;
    int32_t *stencil[MAX_LIGHTS - 1];
};
struct TileKernArgs { FrameConst fc; TileArgs ta; ShadeArgs sh; TileLights ml; };

// One workgroup per tile, one pixel per thread.  Tiles are dealt to workgroups in plain
// row-major order, i.e. round-robin over the XCDs: heavy tiles cluster on the screen, and an
// XCD-contiguous mapping (tried first) left six of the eight XCDs idle behind the two that
// owned the mesh and its shadow.
// SPLIT: the heaviest tiles' shadow quads are shared out over HEAVY_SPLIT workgroups (see HEAVY_SPLIT).
// SS: a supersampled frame (FrameConst::ss_mode != 0; the host launches SS only then): the uint8 output is written by
// the resolve of s x s samples, not per sample.  An instantiation of its own so that the plain frame's code is
// untouched by it (a runtime branch on ss_mode cost the plain c4 frame 1.2 %).
// ML: a frame with several lights (TileLights), an instantiation of its own for the same reason.  Coverage, z and
// winner are the light's business nowhere, so phases 1 and 2 are the plain frame's; phase 3 walks the tile's ONE quad
// list once and keeps one stencil count per light (a quad carries its light's index, the same in every lane while the
// quad is walked); phase 4 works out what of a pixel does not depend on the light once and adds the lights'
// contributions F_k in float32, in the order of the lights: F = min(F_0 + F_1 + ..., 1), every F_k clipped to
// [0.05, 1] like the reference's one.  Such frames never split tiles.
// FULL: the one body of the two kernels below.  FULL == true is the general kernel (k_tile_full).  FULL == false is what
// a frame rendered for the frame's sake needs (k_tile; the plan's choice, FramePlan::full): no MR_FRAME_COUNTERS, no
// MR_FRAME_FACE_STATUS, no depth_test == False model in the scene.  It carries no fragment accumulators, ballots or
// per-tile counts (words 0..4 of the tile's record are not written), `counters` is a constant, and the faces that
// write no z -- the late pass over the big pairs, the nodepth branches of small_pair -- do not exist.  The list lengths
// (words 5..7), the overflow reports, the cursors and the class byte are the same in both; the time stamps are zero.  The
// regime bench.py quotes follows the length of the instruction stream: this is that stream without what the
// frame cannot use.  Same arithmetic on the same values: every byte of the frame, z, winner and stencil is the same.
template <bool SPLIT, bool SS, bool ML, bool FULL>
__device__ __forceinline__ void tile_body()
{
    static_assert(!(SPLIT && ML), "frames with several lights do not split their heavy tiles");
    __shared__ unsigned long long s_key[TILE_PX];
    __shared__ int s_win[TILE_PX];
    __shared__ unsigned int s_cnt[TILE_STATS];            // (FULL only: never referenced otherwise, and not allocated)
    __shared__ uint4 s_quad[QUAD_BATCH * QUAD_STAGE_U4];
    __shared__ uint32_t s_id[QUAD_BATCH];
    __shared__ float s_gamma[GAMMA_LUT_SIZE];
    __shared__ unsigned long long s_mat[MAT_LDS * sizeof(Material) / 8];
    // CULL: the frame-only single-light kernels drop the shadow quads that lie behind everything the tile shows before
    // they stage them (phase 3).  The multi-light kernel is at its 96 registers with scratch and the general ones count
    // every fragment or are at their budgets: they keep the strip-level rule alone.
    constexpr bool CULL = !FULL && !ML;
    __shared__ unsigned long long s_zt;                   // (CULL only) key of the tile's most favourable covered z

    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int lp = tid;                                   // pixel of this thread inside the tile
    // the four time stamps of the tile's record (mr_debug_read_tile_records): the general kernel's only -- in the regime
    // bench.py quotes they cost the c4 frame 0.8 % (profiles/frame_only_path_ab.txt); the frame-only kernel leaves zeros
    auto stamp = []() -> unsigned long long { return FULL ? __builtin_amdgcn_s_memrealtime() : 0ull; };

    // ---- 0. which tile, and what it lists
    int tile = 0, part = 0, n_parts = 1, entry = 0, n_tiles, ltr, gx, gy;
    bool rh, counters, live, mat_lds, taps;
    uint32_t n_small_raw, n_big_raw, n_quad_raw, n_small, n_big, n_quad, cost;
    unsigned long long t_start;
    {
        const TileKernArgs &ka = kernargs<TileKernArgs>();
        const FrameConst &fc = ka.fc;
        const TileArgs &ta = ka.ta;
        const ShadeArgs &sh = ka.sh;
        n_tiles = fc.tiles_x * fc.tiles_y;
        rh = fc.system == 1;
        counters = FULL && (fc.flags & MR_FRAME_COUNTERS) != 0;

        if (blockIdx.x == 0) {
            // The next frame's counter block is the previous frame's (double-buffered by parity; that frame is
            // complete: same stream).  Its overflow verdicts move to the slot's sticky record before the block is
            // cleared; nobody touches either before this kernel ends.
            if (tid == 0) {
                const Counters &old = *ta.next_ctr;
                uint32_t longest = 0;                     // the fullest stretch of the work list decides what the list needs
                for (int s = 0; s < WORK_SHARDS; ++s) longest = max(longest, old.work[s].n);
                if (old.overflow | old.n_quads | longest) {
                    Sticky &st = *ta.sticky;
                    st.overflow |= old.overflow;
#pragma unroll
                    for (int c = 0; c < BIN_CLASSES; ++c) st.max_list[c] = max(st.max_list[c], old.max_list[c]);
                    st.n_work = max(st.n_work, longest * (uint32_t)WORK_SHARDS);
                    st.n_quads = max(st.n_quads, old.n_quads);
                    st.n_quads_drawn = max(st.n_quads_drawn, old.n_quads_drawn);
                }
            }
            __syncthreads();
            uint32_t *words = reinterpret_cast<uint32_t *>(ta.next_ctr);
            for (int i = tid; i < (int)(sizeof(Counters) / 4); i += TILE_PX) words[i] = 0u;
        }

        // heaviest tiles first: entry blockIdx.x of the order k_setup left (see tile_class)
        uint32_t idx = blockIdx.x;
        if (SPLIT) {
            // the class whose quads are shared out -- when it is a handful of tiles, i.e. when the launch would end on them
            // alone; a frame with hundreds of them keeps the device full to the end, and rasterising each four times
            // only adds to that (c3: 209 qualify, k_tile 76 -> 84 us with the split; c5: 143, 253 -> 270; c4: some 40, 66 -> 63)
            const uint32_t n_heavy = ta.order ? ta.order[0] : 0u;
            const uint32_t n0 = n_heavy <= ta.split_max ? n_heavy : 0u;
            if (idx < (uint32_t)SPLIT_FRONT) {
                entry = (int)idx / HEAVY_SPLIT;
                part = (int)idx % HEAVY_SPLIT;
                n_parts = counters ? 1 : HEAVY_SPLIT;
                if (entry >= (int)n0 || part >= n_parts) return;
                idx = (uint32_t)entry;
            } else {
                idx = idx - (uint32_t)SPLIT_FRONT + n0;
            }
        }
        if (idx >= (uint32_t)n_tiles) return;
        tile = ta.order ? (int)ta.order[ORDER_HEAD + idx] : (int)idx;
        ltr = tile / fc.tiles_x;                          // local tile row
        gx = (tile % fc.tiles_x) * TILE_W; gy = tile_row_frame(fc, ltr) * TILE_H;
        const int px = gx + (lp & (TILE_W - 1)), py = gy + lp / TILE_W;
        live = px < fc.width && py >= fc.band_y0 && py < fc.band_y1;
        t_start = stamp();

        // list lengths (a list that ran over its capacity is truncated; the host grows it and re-renders)
        n_small_raw = ta.bin_count[tile]; n_big_raw = ta.bin_count[n_tiles + tile]; n_quad_raw = ta.bin_count[2 * n_tiles + tile];
        n_small = min(n_small_raw, ta.cap[0]); n_big = min(n_big_raw, ta.cap[1]); n_quad = min(n_quad_raw, ta.cap[2]);
        // the heaviest tiles are the frame's critical path: their wavefronts go first wherever they
        // compete with a lighter tile's for a SIMD's issue slots
        cost = tile_cost(n_small_raw, n_big_raw, n_quad_raw);
        if (cost >= 500u) __builtin_amdgcn_s_setprio(3);
        else if (cost >= 250u) __builtin_amdgcn_s_setprio(1);

        // Nothing listed for this tile (a third of a typical frame): its pixels show the background, which
        // the host has finalised already, or the skybox (no lists to walk, no barriers but the gamma table's).
        // Shadow quads over it only matter to the counters.
        const bool sky_tile = (fc.flags & MR_FRAME_SKYBOX) && sh.sky;
        taps = (sh.frame || ta.zbuf) && (!ta.tap_mask || ta.tap_mask[tile_row_frame(fc, ltr) * fc.tiles_x + tile % fc.tiles_x]);
        if (n_small_raw == 0 && n_big_raw == 0 && (n_quad_raw == 0 || !counters) && (sky_tile || (fc.background_u8 >> 24)) &&
            !taps) {
            if (part != 0) return;                        // (a tile that was heavy a frame ago: one part will do)
            uint8_t *o = sh.out + ((size_t)out_row(fc, py, ltr) * fc.width + px) * 3;
            const int ss = SS ? fc.ss_mode : 0;           // (never SS_SEPARATE here: that frame writes every tile's float colour)
            if (sky_tile) {
                s_gamma[tid] = sh.gamma_lut[tid];
                if (tid == 0) s_gamma[GAMMA_LUT_SIZE - 1] = sh.gamma_lut[GAMMA_LUT_SIZE - 1];
                float rgb[3] = { 0.f, 0.f, 0.f };
                if (live) sky_color(fc, sh.sky, px, py, rgb);
                if (ss) {                                 // the sky's samples, resolved like any tile's
                    float *s_rgb = reinterpret_cast<float *>(s_quad);
#pragma unroll
                    for (int j = 0; j < 3; ++j) s_rgb[lp * 3 + j] = rgb[j];
                }
                __syncthreads();
                if (ss) {
                    ss_resolve_tile(fc, reinterpret_cast<const float *>(s_quad), sh.out, gx, gy, tid, s_gamma);
                } else if (live) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) o[j] = gamma_u8(rgb[j], s_gamma);
                }
            } else if (ss) {                              // (16 / s)^2 output pixels of the finalised background
                const int shift = ss & SS_SHIFT_MASK, n_log = 4 - shift;
                const int bpx = gx + ((tid & ((1 << n_log) - 1)) << shift), bpy = gy + ((tid >> n_log) << shift);
                if (tid < 1 << (2 * n_log) && bpx < fc.width && bpy >= fc.band_y0 && bpy < fc.band_y1) {
                    uint8_t *ob = ss_out_pixel(sh.out, fc.width, fc.band_y1, shift, bpx, bpy);
                    ob[0] = (uint8_t)fc.background_u8; ob[1] = (uint8_t)(fc.background_u8 >> 8); ob[2] = (uint8_t)(fc.background_u8 >> 16);
                }
            } else if (live) {
                o[0] = (uint8_t)fc.background_u8; o[1] = (uint8_t)(fc.background_u8 >> 8); o[2] = (uint8_t)(fc.background_u8 >> 16);
            }
            if (tid == 0) {
                uint32_t *rec = ta.tile_stats + (size_t)tile * TILE_REC;
                for (int k = 0; k < TILE_REC; ++k) rec[k] = 0;
                rec[7] = n_quad_raw;
                rec[8] = rec[10] = rec[11] = (uint32_t)t_start;
                rec[9] = (uint32_t)stamp();
                ta.bin_count[2 * n_tiles + tile] = 0;
                ta.tile_class[tile] = (uint8_t)ORDER_CLASSES;
            }
            return;
        }
        // (a tile that goes on stores its first stamp here: carried to the record's other words at the end, it held a
        // pair of scalar registers through every phase, and the multi-light general kernel spilled it)
        if (FULL && tid == 0) ta.tile_stats[(size_t)tile * TILE_REC + 8] = (uint32_t)t_start;
        if (FULL && tid < TILE_STATS) s_cnt[tid] = 0;
        if (CULL && tid == 0) s_zt = rh ? 0ull : ~0ull;   // below (above) the key of every z: "nothing covered" (read behind phase 3's entry barrier)
        s_gamma[tid] = sh.gamma_lut[tid];
        if (tid == 0) s_gamma[GAMMA_LUT_SIZE - 1] = sh.gamma_lut[GAMMA_LUT_SIZE - 1];
        mat_lds = fc.n_materials <= MAT_LDS;
        if (mat_lds && tid < fc.n_materials * (int)(sizeof(Material) / 8))
            s_mat[tid] = reinterpret_cast<const unsigned long long *>(sh.materials)[tid];
    }
    // The pixel's coordinates are recomputed from the thread index where a phase needs them (two instructions),
    // from a copy of the index the compiler cannot connect to the other phases': kept in registers from the first
    // phase to the last, px, py and their float64 images held six of the 80 registers a wavefront may use when
    // six share a SIMD.
    auto my_pixel = [&](int &px, int &py) {
        int l = lp;
        asm volatile("" : "+v"(l));
        px = gx + (l & (TILE_W - 1)); py = gy + l / TILE_W;
    };

    // ---- 1. big pairs, one pixel per thread (obj/triangular.py:72-118)
    double zbest = rh ? INFINITY : -INFINITY;
    int best = -1;
    {
        const TileKernArgs &ka = kernargs<TileKernArgs>();
        const FrameConst &fc = ka.fc;
        const TileArgs &ta = ka.ta;
        const ShadeArgs &sh = ka.sh;
        // (what the loops below read of the arguments is fetched here, once: a load through the opaque pointer is
        // not hoisted out of a loop by the compiler when it sits under a condition)
        const TriRec *__restrict__ tris = sh.tris;
        const TriClip *__restrict__ clips = ta.clips;
        const uint32_t *__restrict__ small_items = ta.items[0] + (size_t)tile * ta.cap[0];
        const uint32_t *__restrict__ big_items = ta.items[1] + (size_t)tile * ta.cap[1];
        const bool same_clip = fc.same_clip != 0, has_no_depth = FULL && fc.has_no_depth != 0;
        const TileBounds tb = { fc.width, fc.band_y0, fc.band_y1 };
        int px, py;
        my_pixel(px, py);
        const double dpx = (double)px, dpy = (double)py;
        unsigned int frags = 0;
        // The records of up to 64 pairs are copied to LDS once per workgroup, 16 bytes per lane and step
        // (the staging area of the shadow quads, not in use yet), and every lane then reads the pair it is
        // testing at the same LDS address (a broadcast read).  Each wavefront fetching the records itself,
        // one per lane, and handing them round with v_readlane cost ~45 vector instructions per pair and
        // wavefront on top of the arithmetic; scalar loads cost a dependent memory round trip per pair.
        constexpr int TRI_U4 = (int)(sizeof(TriRec) / 16);
        static_assert(WAVE * TRI_U4 <= QUAD_BATCH * QUAD_STAGE_U4, "big-pair records are staged in the quad area");
        // LATE == false: the faces that write z.  LATE == true (only in scenes that have a model with
        // depth_test == False, after the tile's final z is known): those that do not -- they own the pixel
        // when they pass against the final z and come later in face order than the current owner.
        auto big_pairs = [&](const bool late) {
            for (uint32_t base = 0; base < n_big; base += WAVE) {
                const int n = (int)min((uint32_t)WAVE, n_big - base);
                if (base || late) __syncthreads();        // the staging area is free
                for (int i = tid; i < n * TRI_U4; i += TILE_PX) {
                    const int q = i / TRI_U4, piece = i - q * TRI_U4;
                    s_quad[i] = reinterpret_cast<const uint4 *>(tris + big_items[base + q])[piece];
                }
                __syncthreads();
                for (int j = 0; j < n; ++j) {
                    const TriRec &t = *reinterpret_cast<const TriRec *>(s_quad + j * TRI_U4);
                    const uint32_t flags = t.flags;
                    const bool nodepth = FULL && ((flags >> 8) & FF_NO_DEPTH) != 0;
                    if (late && !nodepth) continue;
                    // the pair is the same for every lane, so are its flags: the usual face (neither of the two
                    // summation-order flags) takes a copy of the arithmetic without their selects (see PairMath)
                    auto pair = [&](auto maybe_single) {
                        const PairMath<decltype(maybe_single)::value> pm(t);
                        const int f = t.face;
                        bool in = live && px >= t.x0 && px < t.x1 && py >= t.y0 && py < t.y1;
                        float u, v, w;
                        pm.bary(dpx, dpy, u, v, w);
                        in = in && u >= 0 && v >= 0 && w >= 0;
                        const unsigned long long m = __ballot(in);
                        if (!m) return;
                        if (FULL && !late) frags += (unsigned int)__popcll(m);
                        if (nodepth && !late) return;
                        if (flags & TF_CLIP) {
                            if (in) {
                                const TriClip &c = clips[f];
                                double p[3];
                                persp_bary(t.dp, u, v, w, (flags & TF_SINGLE_BOX) != 0, p);
                                in = inside_clip(p, c.clip) && (same_clip || inside_clip(p, c.clipd));
                            }
                        }
                        const double z = pm.depth(u, v, w);
                        if (late) {
                            if (in && (rh ? z <= zbest : z >= zbest) && f > best) best = f;
                        } else {
                            // sequential rule "zbuf >= z writes" == smallest z, and among equal z the latest face
                            const bool closer = rh ? (z < zbest) : (z > zbest);
                            if (in && (closer || (z == zbest && f > best))) { zbest = z; best = f; }
                        }
                    };
                    if (flags & (TF_SINGLE_BOX | TF_SINGLE_Z)) pair(std::true_type{});
                    else pair(std::false_type{});
                }
            }
        };
        big_pairs(false);
        if (n_small) { s_key[lp] = z_key(zbest); s_win[lp] = -1; }     // the small pairs' LDS z-buffer starts from the big pairs' z
        __syncthreads();                                  // s_cnt is zeroed, the LDS tables are loaded
        if (FULL && lane == 0 && frags) atomicAdd(&s_cnt[0], frags);
        if (n_small) {
            // ---- 2. small pairs, SMALL_LANES lanes per triangle, z into the LDS z-buffer
            // The second sweep (who owns the final z?) needs every covered sample's z key again.  The first sweep
            // leaves them in the lane's log (PairLog; the staging area of the shadow quads, not in use yet: 12 KB,
            // exactly), and the second compares those without the item, the record, the barycentrics or the depth.
            // Only a lane whose log ran over -- or that met a face that writes no z -- walks again, from there on.
            static_assert(PAIR_LOG_K * TILE_PX * (8 + 4) <= (int)sizeof(s_quad), "the pair log fits the quad area");
            PairLog log;
            log.key = reinterpret_cast<unsigned long long (*)[TILE_PX]>(s_quad);
            log.word = reinterpret_cast<uint32_t (*)[TILE_PX]>(log.key + PAIR_LOG_K);
            log.n = 0;
            // (the general kernel of a frame with several lights keeps the plain second walk, capacity 0 at compile time:
            // at 96 registers it spills already, and the log's state cost it 4 to 16 bytes of scratch more, past the
            // budget tests/test_kernel_layout.py holds it to)
            log.cap = FULL && ML ? 0u : min(kernargs<TileKernArgs>().ta.pair_log, (uint32_t)PAIR_LOG_K);
            log.resume = log.cap ? PAIR_LOG_NONE : 0u;        // capacity 0: every sample is walked again
            unsigned int sfrags = 0;
            // SMALL_LANES lanes per pair; two where the list is longer than one round of those (a round is two
            // dependent memory round trips whatever it holds: 65 pairs in two rounds cost twice what 64 do), eight
            // where it is at most half a round (the lanes would idle otherwise; c2's larger triangles: -2 %)
            const int spl = n_small > (uint32_t)(TILE_PX / SMALL_LANES) ? SMALL_LANES / 2
                          : n_small > (uint32_t)(TILE_PX / (2 * SMALL_LANES)) ? SMALL_LANES : 2 * SMALL_LANES;
            const uint32_t per_round = (uint32_t)(TILE_PX / spl), my_pair = (uint32_t)(tid / spl);
            const int sub = tid % spl;
            for (uint32_t i = my_pair; i < n_small; i += per_round) {
                const TriRec t = tris[small_items[i]];
                const uint32_t over = small_pair<0, FULL>(tb, t, gx, gy, rh, s_key, s_win, sub, spl, sfrags, &log, tid);
                // (a lane whose log is full has n == cap from then on: every later covered sample reports `over`, the first counts)
                log.resume = (log.resume == PAIR_LOG_NONE && over != PAIR_LOG_NONE) ? ((i / per_round) << 8) | over : log.resume;
            }
            if (FULL && sfrags) atomicAdd(&s_cnt[0], sfrags);
            __syncthreads();

            // winners: a big pair keeps its face where its z survived (an atomic like the small pairs' sweep: the
            // largest face index among those at the final z, in any order)
            const unsigned long long kfinal = s_key[lp];
            if (best >= 0 && kfinal == z_key(zbest)) atomicMax(&s_win[lp], best);
            const uint32_t n_logged = log.n;
#pragma unroll
            for (uint32_t e = 0; e < (uint32_t)PAIR_LOG_K; ++e)
                if (e < n_logged) {
                    const uint32_t w = log.word[e][tid], p = w & 0xffu;
                    if (s_key[p] == log.key[e][tid]) atomicMax(&s_win[p], (int)(w >> 8));
                }
            sfrags = 0;                                   // (general kernel: the samples walked again)
            if (log.resume != PAIR_LOG_NONE) {
                int first = (int)(log.resume & 0xffu);
                for (uint32_t i = my_pair + (log.resume >> 8) * per_round; i < n_small; i += per_round) {
                    const TriRec t = tris[small_items[i]];
                    small_pair<1, FULL, FULL>(tb, t, gx, gy, rh, s_key, s_win, sub, spl, sfrags, nullptr, tid, first);
                    first = 0;
                }
            }
            if (counters) {                               // mr_debug_pair_log: entries answered from the log, samples walked again
                unsigned int a = n_logged, b = sfrags;
#pragma unroll
                for (int off = WAVE / 2; off; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
                if (lane == 0 && a) atomicAdd(&ta.ctr->pad0[5], a);
                if (lane == 0 && b) atomicAdd(&ta.ctr->pad0[6], b);
            }
            __syncthreads();
            best = s_win[lp];
            zbest = z_unkey(kfinal);
        }
        if (has_no_depth) big_pairs(true);
    }
    const bool covered = live && best >= 0;
    const unsigned long long t_raster = stamp();

    // ---- 3. shadow quads against the final z: stencil +-1 (obj/triangular.py:335-368).  The
    // batch's records (header and first four edges: 192 bytes each) are copied to LDS once, 16 bytes
    // per lane, and every lane then reads the quad it is testing at the same LDS address (a
    // broadcast read).  Adds commute, so the order of the quads never mattered
    // (obj/triangular.py:365-368); the strip walk's count stays in this thread's register, the span walk's in the
    // pixel's LDS word, and the two are added behind the last batch.
    int sten = 0;
    int sten_x[MAX_LIGHTS - 1] = { 0, 0, 0 };             // ML: lights 1.. (always indexed by constants: registers)
    unsigned int qfrags = 0, qupd = 0;
    // without the counters only the frame is the contract: the stencil matters where a triangle was drawn
    unsigned int q_kept = 0;                              // CULL: the quads this workgroup staged (word 8 of the tile's record)
    // CULL (the frame-only single-light kernels): the tile's most favourable covered z is the extreme of its strips',
    // one LDS atomic per wavefront that covers anything, in front of the entry barrier; a word nobody touched says what
    // __syncthreads_or(covered) says in the other kernels.
    int zt_seen = 0;
    if (CULL && n_quad) {
        if (__ballot(covered)) {
            // (the wavefront's extreme again below, where the strip's two limits are worked out together)
            double zw = covered ? zbest : (rh ? -INFINITY : INFINITY);
#pragma unroll
            for (int off = WAVE / 2; off; off >>= 1) { const double o = __shfl_xor(zw, off); zw = rh ? fmax(zw, o) : fmin(zw, o); }
            if (lane == 0) { if (rh) atomicMax(&s_zt, z_key(zw)); else atomicMin(&s_zt, z_key(zw)); }
        }
        __syncthreads();
        zt_seen = __builtin_amdgcn_readfirstlane(s_zt != (rh ? 0ull : ~0ull) ? 1 : 0);
    }
    if (n_quad && (CULL ? zt_seen != 0 : (counters || __syncthreads_or(covered)))) {
        const TileKernArgs &ka = kernargs<TileKernArgs>();
        const FrameConst &fc = ka.fc;
        const TileArgs &ta = ka.ta;
        const uint32_t *__restrict__ quad_items = ta.items[2] + (size_t)tile * ta.cap[2];
        const QuadRec *__restrict__ quads = ta.quads;
        const double f_plus_n = fc.f_plus_n, f_minus_n = fc.f_minus_n, two_nf = fc.two_nf;     // fetched once, see above
        // most and least favourable covered z of this wavefront's strip (see the depth verdicts below)
        double zlim = rh ? -INFINITY : INFINITY, zhard = rh ? INFINITY : -INFINITY;
        if (covered) zlim = zhard = zbest;
#pragma unroll
        for (int off = WAVE / 2; off; off >>= 1) {
            const double o = __shfl_xor(zlim, off), h = __shfl_xor(zhard, off);
            zlim = rh ? fmax(zlim, o) : fmin(zlim, o);
            zhard = rh ? fmin(zhard, h) : fmax(zhard, h);
        }
        // (frame-only: both are the same in every lane now, and go to scalar registers -- without the counted frame's
        // code the compiler hoists the batch loop's invariants out of it, and four vector registers fewer keep it from
        // spilling them; the general kernel is the code it was)
        if (!FULL) {
            zlim = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(zlim)), __builtin_amdgcn_readfirstlane(__double2loint(zlim)));
            zhard = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(zhard)), __builtin_amdgcn_readfirstlane(__double2loint(zhard)));
        }
        // (CULL: set up in front of the first batch that is staged, if any is -- the key from a copy of z the compiler
        // cannot trace, or it is worked out in front of the batch loop and spilled)
        auto span_words = [&]() {
            if (ta.quad_walk != QUAD_WALK_STRIPS) {
                double zb = zbest;
                asm volatile("" : "+v"(zb));
                if (!n_small) s_key[lp] = z_key(zb);
                s_win[lp] = 0;
            }
        };
        // The span walk (single light): the final z in LDS (the keys are there already wherever the tile had small
        // pairs), and the stencil words it adds to in s_win, dead since `best` was read.  Each thread writes its own
        // pixel's; the batch's staging barrier stands between these stores and the first span.
        // (the walk's few arguments are read where they are used, batch by batch: kept in scalar registers from here
        // on they cost the kernel its sixth wavefront)
        if (!CULL && !ML && ta.quad_walk != QUAD_WALK_STRIPS) {
            if (!n_small) s_key[lp] = z_key(zbest);
            s_win[lp] = 0;
        }
        const uint32_t q_begin = SPLIT ? (uint32_t)((unsigned long long)part * n_quad / n_parts) : 0u,
                       q_end = SPLIT ? (uint32_t)((unsigned long long)(part + 1) * n_quad / n_parts) : n_quad;    // this part's share
        for (uint32_t qbase = q_begin; qbase < q_end; qbase += QUAD_BATCH) {
            int n = (int)min((uint32_t)QUAD_BATCH, q_end - qbase);
            // Staging also folds two per-quad facts into the copy: a back-facing quad's edge vectors are
            // negated (the rounded cross product changes sign exactly, so "inner side" is "> 0" for every
            // staged quad), and the last 16 bytes of the header, unused here, receive f_plus_n * nz and
            // two_nf * nz of the depth test below.
            if (CULL) {
                // Lane j of every wavefront takes entry j of the batch and the bound k_bin_work left beside it, and drops
                // the quad when no sample of the tile can pass against the tile's z (quad_tile_none, quad_reject.h: the
                // strip rule below would reject it in all four wavefronts).  Every wavefront reads the same values, so
                // the ballot is the same in all four: an empty one skips the batch with its two barriers in the whole
                // workgroup, otherwise the survivors move to the lanes 0 .. n-1 in order and only they are staged and
                // classified.  (The tile's z is read per batch: held in scalar registers it was spilled.)
                bool keep = lane < n;
                uint32_t my_id = 0;
                if (keep) {
                    my_id = quad_items[qbase + lane];
                    if (ta.quad_cull & 1u) {
                        double tnf = two_nf;                // (an untraceable copy again: see the strip's verdicts below)
                        asm volatile("" : "+v"(tnf));
                        keep = !quad_tile_none(ta.quad_bound[(size_t)tile * ta.cap[2] + qbase + lane], z_unkey(s_zt), tnf, rh);
                    }
                }
                const unsigned long long km = __ballot(keep);
                n = __popcll(km);
                if (!n) continue;
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u));
                const int ids = __builtin_amdgcn_ds_permute((keep ? rank : n + (lane - rank)) << 2, (int)my_id);
                if (q_kept) __syncthreads();              // the previous batch has been read
                else span_words();
                q_kept += (unsigned int)n;
                // (staged as below, the survivor's id from the wavefront's own copy of the list: every lane takes part)
                for (int i0 = 0; i0 < n * QUAD_STAGE_U4; i0 += TILE_PX) {
                    const int i = i0 + tid, q = i / QUAD_STAGE_U4, piece = i - q * QUAD_STAGE_U4;
                    const uint32_t id = (uint32_t)__builtin_amdgcn_ds_bpermute(q << 2, ids);
                    if (i < n * QUAD_STAGE_U4) {
                        const QuadRec *src = quads + id;
                        uint4 val = reinterpret_cast<const uint4 *>(src)[piece];
                        if (piece == 3) {
                            const double a0 = f_plus_n * src->nz, b0 = two_nf * src->nz;
                            val = make_uint4((uint32_t)__double2loint(a0), (uint32_t)__double2hiint(a0),
                                             (uint32_t)__double2loint(b0), (uint32_t)__double2hiint(b0));
                        } else if (piece >= 5 && (piece & 1) && !src->is_front) {
                            val.y ^= 0x80000000u; val.w ^= 0x80000000u;
                        }
                        s_quad[i] = val;
                        if (piece == 0) s_id[q] = id;
                    }
                }
            } else {
                if (qbase != q_begin) __syncthreads();    // the previous batch has been read
                for (int i = tid; i < n * QUAD_STAGE_U4; i += TILE_PX) {
                    const int q = i / QUAD_STAGE_U4, piece = i - q * QUAD_STAGE_U4;
                    const uint32_t id = quad_items[qbase + q];
                    const QuadRec *src = quads + id;
                    uint4 val = reinterpret_cast<const uint4 *>(src)[piece];
                    if (piece == 3) {
                        const double a0 = f_plus_n * src->nz, b0 = two_nf * src->nz;
                        val = make_uint4((uint32_t)__double2loint(a0), (uint32_t)__double2hiint(a0),
                                         (uint32_t)__double2loint(b0), (uint32_t)__double2hiint(b0));
                    } else if (piece >= 5 && (piece & 1) && !src->is_front) {
                        val.y ^= 0x80000000u; val.w ^= 0x80000000u;
                    } else if (ML && piece == 2) {
                        val.w |= src->light << 1;               // beside is_front (0 / 1): the header's last 16 bytes are overwritten above
                    }
                    s_quad[i] = val;
                    if (piece == 0) s_id[q] = id;
                }
            }
            __syncthreads();

            // Lane j classifies quad j against this wavefront's 16x4 pixel strip with the same
            // corner argument as quad_touches_tile: per edge, the rounded cross product is monotone
            // in x and in y, so over the strip it is extreme at a corner.  No corner on the inner
            // side of some edge -> no sample of the strip is inside (skip the quad); all four
            // corners on the inner side of every edge -> every sample is inside (skip the
            // per-pixel edge tests).  Exact, no margins.
            // Per edge too: an edge whose inner side holds all four corners needs no per-pixel test
            // in this strip (bit i of emask clear); typically one edge of a quad crosses a strip.
            bool q_reject = lane >= n;
            bool q_finite = true;                           // every term of the corner tests is finite (the span walk needs it)
            int emask = 0;
            if (!q_reject) {
                const QuadHead &h = *reinterpret_cast<const QuadHead *>(s_quad + lane * QUAD_STAGE_U4);
                const QuadEdge *e = reinterpret_cast<const QuadEdge *>(s_quad + lane * QUAD_STAGE_U4 + 4);
                const double xa = (double)gx, xb = (double)(gx + TILE_W - 1);
                const double ya = (double)(gy + (tid / WAVE) * (WAVE / TILE_W)), yb = ya + (double)(WAVE / TILE_W - 1);
                if (h.n > 4) emask |= 16;                   // edges beyond the staged four: always per pixel
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < 3 || h.n > 3) {
                        const double px0 = (xa - e[i].sx) * e[i].ey, px1 = (xb - e[i].sx) * e[i].ey;
                        const double py0 = (ya - e[i].sy) * e[i].ex, py1 = (yb - e[i].sy) * e[i].ex;
                        const double c00 = px0 - py0, c10 = px1 - py0, c01 = px0 - py1, c11 = px1 - py1;
                        const bool any = c00 > 0 || c10 > 0 || c01 > 0 || c11 > 0;
                        const bool all = c00 > 0 && c10 > 0 && c01 > 0 && c11 > 0;
                        q_reject = q_reject || !any;
                        if (!ML) q_finite = q_finite && fabs(px0) + fabs(px1) + fabs(py0) + fabs(py1) < INFINITY;
                        if (!all) emask |= 1 << i;
                    }
                }
            }
            // Depth verdicts for the whole strip (quad_rect_bounds / quad_rect_sane / quad_rect_verdict, quad_reject.h): `all pass` skips
            // the per-pixel depth arithmetic; `none can` (only when the frame is all that is asked for, no
            // MR_FRAME_COUNTERS: the stencil matters where a triangle was drawn) skips the quad.
            bool q_allpass = false;
            if (!q_reject) {
                const QuadHead &h = *reinterpret_cast<const QuadHead *>(s_quad + lane * QUAD_STAGE_U4);
                const double xa = (double)gx, xb = (double)(gx + TILE_W - 1);
                const double ya = (double)(gy + (tid / WAVE) * (WAVE / TILE_W)), yb = ya + (double)(WAVE / TILE_W - 1);
                const QuadRectBounds b = quad_rect_bounds(h.nx, h.ny, h.nz, h.d, xa, xb, ya, yb, f_plus_n, f_minus_n);
                // (single light: three products of frame constants, worked out here per batch from copies the compiler
                // cannot trace -- hoisted out of the batch loop they held six registers through the span walk)
                double fpn = f_plus_n, tnf = two_nf;
                if (!ML) asm volatile("" : "+v"(fpn), "+v"(tnf));
                const bool sane = quad_rect_sane(b, h.nz, f_minus_n, two_nf, fpn);
                const QuadRectVerdict v = quad_rect_verdict(b, tnf, zlim, zhard, rh);
                if (sane && !counters && v.none) q_reject = true;
                q_allpass = sane && v.all;
            }
            unsigned long long todo = __ballot(!q_reject);
            const unsigned long long allpass = __ballot(q_allpass);

            // ---- the span walk: sliver quads as (quad, row) items, sixteen quads to a round of this wavefront.
            // For a fixed row y the staged inside test of edge i, rn(rn(rn(x - sx) * ey) - rn(rn(y - sy) * ex)) > 0, has
            // a constant second term and a first term monotone in x (every step is a monotone function of the one
            // before, and nothing is NaN: q_finite bounds both products by their finite values at the strip's corners).
            // So the x that pass form a half-line -- x >= F for ey > 0, x < F for ey < 0, all or none for ey == 0 -- and
            // F is found by bisection over the row's 16 positions with the very expression the strip walk evaluates
            // per pixel: no division, no estimate to repair.  The quad's samples in the row are the interval left by its
            // crossing edges (the others hold on the whole strip: emask) and the clamped box.  Per sample: the depth rule
            // (quad_depth_pass) against the pixel's final z from LDS, then an LDS atomic add on the pixel's stencil word.
            // Which quads come here is a function of the batch's records and the strip alone, never of timing.
            const uint32_t quad_walk = ML ? (uint32_t)QUAD_WALK_STRIPS : kernargs<TileKernArgs>().ta.quad_walk;
            if (!ML && quad_walk != QUAD_WALK_STRIPS) {
                const bool span_ok = !q_reject && q_finite && !(emask & 16);
                unsigned long long smask = __ballot(span_ok && (quad_walk == QUAD_WALK_SPANS || __popc(emask & 15) >= MR_SPAN_MIN_EDGES));
                if (quad_walk == QUAD_WALK_AUTO && __popcll(smask) < MR_SPAN_MIN_QUADS) smask = 0;
                todo &= ~smask;
                if (smask) {
                    // compaction without LDS: the survivors push their lane to the lanes 0 .. cnt-1 in order, the
                    // others fill the rest (a permutation), with the strip verdicts beside the lane
                    const int cnt = __popcll(smask);
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(smask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)smask, 0u));
                    int ln = lane;                          // (frame-only: a copy the compiler cannot trace, or 1 << lane is held from outside the batch loop)
                    if (!FULL) asm volatile("" : "+v"(ln));
                    const int dest = ((smask >> ln) & 1) ? rank : cnt + (lane - rank);
                    const int list = __builtin_amdgcn_ds_permute(dest << 2, lane | (emask << 8) | ((q_allpass ? 1 : 0) << 16));
                    const int ly = (tid / WAVE) * (WAVE / TILE_W) + (lane & 3);       // the item's row of the tile
                    const int y = gy + ly;
                    const double dy = (double)y;
                    const FrameConst &fcs = kernargs<TileKernArgs>().fc;
                    const int f_width = fcs.width, f_band_y0 = fcs.band_y0, f_band_y1 = fcs.band_y1;
#pragma unroll 1
                    for (int base = 0; base < cnt; base += WAVE / 4) {
                        const int k = base + (lane >> 2);
                        const int it = __builtin_amdgcn_ds_bpermute(k << 2, list);
                        const int j = it & (WAVE - 1), em = (it >> 8) & 15;
                        const uint4 *rec = s_quad + j * QUAD_STAGE_U4;
                        const uint4 hb = rec[2];
                        const int x0 = (int)(int16_t)(hb.x & 0xffffu), x1 = (int)(int16_t)(hb.x >> 16);
                        const int y0 = (int)(int16_t)(hb.y & 0xffffu), y1 = (int)(int16_t)(hb.y >> 16);
                        // positions of the row, 0 .. 16: the box clamped to the tile and the frame
                        int lo = max(x0 - gx, 0), hi = min(min(x1, f_width) - gx, TILE_W);
                        const bool item = k < cnt && y >= max(y0, f_band_y0) && y < min(y1, f_band_y1) && lo < hi;
                        if (counters) {                     // (quad, row) items: mr_debug_quad_walks
                            const unsigned long long im = __ballot(item);
                            if (lane == 0 && im) atomicAdd(&kernargs<TileKernArgs>().ta.ctr->pad0[1], (unsigned int)__popcll(im));
                        }
                        auto d2 = [](uint32_t l, uint32_t h) { return __hiloint2double((int)h, (int)l); };
#pragma unroll 1
                        for (int i = 0; i < 4; ++i) {
                            if (item && ((em >> i) & 1)) {
                                const uint4 a = rec[4 + 2 * i], b = rec[5 + 2 * i];
                                const double sx = d2(a.x, a.y), ex = d2(b.x, b.y), ey = d2(b.z, b.w);
                                const double cy = (dy - d2(a.z, a.w)) * ex;
                                const bool down = ey < 0;
                                // up(p): position p is on the side the half-line extends to on the right
                                auto up = [&](int p) { return (((double)(gx + p) - sx) * ey - cy > 0) != down; };
                                int f = up(7) ? 0 : 8;               // first position that is `up`, 0 .. 16
                                f += up(f + 3) ? 0 : 4;
                                f += up(f + 1) ? 0 : 2;
                                f += up(f) ? 0 : 1;
                                f += up(f) ? 0 : 1;
                                if (down) hi = min(hi, f); else lo = max(lo, f);
                            }
                        }
                        if (!item) hi = lo;
                        if (lo < hi) {
                            const uint4 p0 = rec[0], p1 = rec[1], p3 = rec[3];
                            const double q_nx = d2(p0.x, p0.y), q_ny = d2(p0.z, p0.w), nzq = d2(p1.x, p1.y), q_d = d2(p1.z, p1.w);
                            const double a0 = d2(p3.x, p3.y), b0 = d2(p3.z, p3.w);
                            const bool need_z = !((it >> 16) & 1);
                            const int delta = hb.w != 0 ? 1 : -1;
                            unsigned int passed = 0;
                            for (int x = lo; x < hi; ++x) {
                                const int p = ly * TILE_W + x;
                                bool pass = true;
                                if (need_z)
                                    pass = quad_depth_pass(q_nx, q_ny, nzq, q_d, a0, b0, (double)(gx + x), dy, z_unkey(s_key[p]), rh, true,
                                                           f_plus_n, f_minus_n, two_nf);
                                if (pass) { atomicAdd(&s_win[p], delta); ++passed; }
                            }
                            if (counters) {
                                atomicAdd(&s_cnt[1], (unsigned int)(hi - lo));
                                if (passed) atomicAdd(&s_cnt[2], passed);
                            }
                        }
                    }
                }
            }

            // (single light: the pixel's coordinates are worked out behind the span walk, whose registers they would take)
            int px, py;
            my_pixel(px, py);
            const double dpx = (double)px, dpy = (double)py;
            if (!ML && counters) {                          // (quad, strip) walks, and those the span walk is not defined for
                const unsigned long long poly = todo & __ballot((emask & 16) != 0), wild = todo & __ballot(!q_finite);
                Counters *ctr = kernargs<TileKernArgs>().ta.ctr;
                if (lane == 0 && todo) atomicAdd(&ctr->pad0[2], (unsigned int)__popcll(todo));
                if (lane == 0 && poly) atomicAdd(&ctr->pad0[3], (unsigned int)__popcll(poly));
                if (lane == 0 && wild) atomicAdd(&ctr->pad0[4], (unsigned int)__popcll(wild));
            }
            while (todo) {
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                // The whole record is fetched up front with 16-byte broadcast reads (every lane the same
                // LDS address) behind ONE wait: a heavy tile walks 50-100 quads one after the other, and
                // a read issued only where its value is needed puts an LDS round trip on that serial
                // chain each time (measured: 0.5 us per quad against 0.2).  Which edges need the per-pixel
                // test is wavefront-uniform (lane j's verdict), so the skipped ones cost no arithmetic.
                const uint4 *rec = s_quad + j * QUAD_STAGE_U4;
                const uint4 p0 = rec[0], p1 = rec[1], hb = rec[2], p3 = rec[3];
                const uint4 ea0 = rec[4], eb0 = rec[5], ea1 = rec[6], eb1 = rec[7], ea2 = rec[8], eb2 = rec[9],
                            ea3 = rec[10], eb3 = rec[11];
                const int em = __builtin_amdgcn_readlane(emask, j);
                const int x0 = (int)(int16_t)(hb.x & 0xffffu), x1 = (int)(int16_t)(hb.x >> 16);
                const int y0 = (int)(int16_t)(hb.y & 0xffffu), y1 = (int)(int16_t)(hb.y >> 16);
                const int nv = (int)hb.z;
                const bool front = ML ? (hb.w & 1u) != 0 : hb.w != 0;
                bool in = live & (px >= x0) & (px < x1) & (py >= y0) & (py < y1);
                auto d2 = [](uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); };
                auto inner = [&](const uint4 &a, const uint4 &b) {       // staged edges: inner side is > 0
                    const double ax = dpx - d2(a.x, a.y), ay = dpy - d2(a.z, a.w);
                    return ax * d2(b.z, b.w) - ay * d2(b.x, b.y) > 0;
                };
                if (em & 1) in = in & inner(ea0, eb0);
                if (em & 2) in = in & inner(ea1, eb1);
                if (em & 4) in = in & inner(ea2, eb2);
                if (em & 8) in = in & inner(ea3, eb3);
                if (em & 16) {                              // clipped polygons with 5+ vertices are rare
                    const QuadRec *q = quads + s_id[j];
                    for (int i = 4; i < nv; ++i) {
                        const double ax = dpx - q->e[i].sx, ay = dpy - q->e[i].sy;
                        const double cr = ax * q->e[i].ey - ay * q->e[i].ex;
                        in = in & (front ? cr > 0 : cr < 0);
                    }
                }
                const unsigned long long m = __ballot(in);
                if (!m) continue;
                if (FULL) qfrags += (unsigned int)__popcll(m);
                bool pass = true;
                if (!((allpass >> j) & 1)) {
                const double q_nx = __hiloint2double((int)p0.y, (int)p0.x), q_ny = __hiloint2double((int)p0.w, (int)p0.z);
                const double nzq = __hiloint2double((int)p1.y, (int)p1.x), q_d = __hiloint2double((int)p1.w, (int)p1.z);
                pass = quad_depth_pass(q_nx, q_ny, nzq, q_d, d2(p3.x, p3.y), d2(p3.z, p3.w), dpx, dpy, zbest, rh, in,
                                       f_plus_n, f_minus_n, two_nf);
                }
                pass = pass && in;
                if (FULL) qupd += (unsigned int)__popcll(__ballot(pass));
                if (ML) {
                    const int lt = __builtin_amdgcn_readfirstlane((int)(hb.w >> 1)), d = pass ? (front ? 1 : -1) : 0;
                    if (lt == 0) sten += d;
                    else if (lt == 1) sten_x[0] += d;
                    else if (lt == 2) sten_x[1] += d;
                    else sten_x[2] += d;
                } else {
                sten += pass ? (front ? 1 : -1) : 0;
                }
            }
        }
        if (!ML && (!CULL || q_kept) && kernargs<TileKernArgs>().ta.quad_walk != QUAD_WALK_STRIPS) {
            __syncthreads();                              // every wavefront's spans are in
            sten += s_win[lp];
        }
    }

    if (SPLIT && n_parts > 1) {
        // Leave this part's counts, then take a ticket.  Hand-off between workgroups on different CUs
        // (MI355X_MICROARCH.md, inter-workgroup visibility): plain stores, EVERY storing wave drains its
        // own stores (s_waitcnt vmcnt(0): a workgroup barrier does not wait for vector memory), the
        // barrier, ONE agent-scope release, then the relaxed ticket; the last arriver does ONE agent-scope
        // acquire (invalidates its CU's L1) behind a barrier, then plain loads.
        __shared__ uint32_t s_ticket;
        const TileArgs &ta = kernargs<TileKernArgs>().ta;
        int32_t *mine = ta.split_sten + ((size_t)entry * HEAVY_SPLIT + part) * TILE_PX;
        int l = lp;                                       // (frame-only: an untraceable copy like my_pixel's, or 4 * lp is held -- and spilled -- from phase 2 to here)
        if (!FULL) asm volatile("" : "+v"(l));
        mine[l] = sten;
        // (CULL: the part's count of staged quads behind the stencil counts, handed over the same way)
        uint32_t *kept = reinterpret_cast<uint32_t *>(ta.split_sten + (size_t)HEAVY0_MAX * HEAVY_SPLIT * TILE_PX) + (size_t)entry * HEAVY_SPLIT;
        if (CULL && tid == 0) kept[part] = q_kept;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            s_ticket = atomicAdd(&ta.split_arrive[entry], 1u);
        }
        __syncthreads();
        if (s_ticket != (uint32_t)(n_parts - 1)) return;  // not the last one: whoever is adds these counts and shades
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            ta.split_arrive[entry] = 0;                   // every part has arrived: ready for the next frame
        }
        __syncthreads();
        for (int k = 0; k < n_parts; ++k)
            if (k != part) sten += ta.split_sten[((size_t)entry * HEAVY_SPLIT + k) * TILE_PX + l];
        if (CULL)
            for (int k = 0; k < n_parts; ++k)
                if (k != part) q_kept += __atomic_load_n(&kept[k], __ATOMIC_RELAXED);
    }
    const unsigned long long t_quads = stamp();

    // ---- 4. deferred shading + finalise (kernels_shade.h; obj/core.py:640)
    const bool lit = (int16_t)sten == 0;                  // the reference's buffer is int16
    unsigned int n_lit = lit ? 1u : 0u;                   // ML: over the frame's lights
    // A supersampled frame's samples are staged in the quad area for the fused resolve at the end of this phase (see
    // there): every wavefront must have left the last quad batch first.
    const bool fused_ss = SS && !(kernargs<TileKernArgs>().fc.ss_mode & SS_SEPARATE);
    if (fused_ss) __syncthreads();
    // ML: which lights reach the pixel, and the taps of z, winner and the stencil counts right here -- shading then
    // carries one mask instead of the four counts and the depth (with them it did not fit five wavefronts' registers)
    unsigned int lit_mask = lit ? 1u : 0u;
    if (ML) {
        const TileKernArgs &ka = kernargs<TileKernArgs>();
        const int n_lights = min(max(ka.ml.lights.n, 1), MAX_LIGHTS);
#pragma unroll
        for (int k = 1; k < MAX_LIGHTS; ++k)
            if (k < n_lights && (int16_t)sten_x[k - 1] == 0) lit_mask |= 1u << k;
        if (live && ka.ta.zbuf && taps) {
            int px, py;
            my_pixel(px, py);
            const size_t at_px = (size_t)py * ka.fc.width + px;
            ka.ta.zbuf[at_px] = zbest;
            ka.ta.winner[at_px] = best;
            ka.ta.stencil[at_px] = sten;
#pragma unroll
            for (int k = 1; k < MAX_LIGHTS; ++k)
                if (k < n_lights) ka.ml.stencil[k - 1][at_px] = sten_x[k - 1];
        }
    }
    if (live) {
        const TileKernArgs &ka = kernargs<TileKernArgs>();
        const FrameConst &fc = ka.fc;
        const TileArgs &ta = ka.ta;
        const ShadeArgs &sh = ka.sh;
        const LightConst lc = frame_light(fc);
        int px, py;
        my_pixel(px, py);
        float rgb[3] = { fc.background[0], fc.background[1], fc.background[2] };
        bool ready_u8 = false;
        if (best >= 0) {
            const TriRec t = sh.tris[best];
            ShadedFace sf;
            load_shaded_face(sh, fc.pos32 != 0, best, sf);
            const Material *mp = mat_lds ? reinterpret_cast<const Material *>(s_mat) + t.material
                                         : sh.materials + t.material;
            if (ML) {
                const int n_lights = min(max(ka.ml.lights.n, 1), MAX_LIGHTS);
                n_lit = (unsigned int)__popc(lit_mask);
                Surface sp;
                shade_surface(t, sf, *mp, px, py, lit_mask != 0, sp);
                LitSurface ls = {};
                if (lit_mask) shade_lit_surface(lc.camera_pos, sp, *mp, ls);
                float acc[3] = { 0.f, 0.f, 0.f };
#pragma unroll 1
                for (int k = 0; k < n_lights; ++k) {
                    const LightConst lk = light_const(ka.ml.lights.l[k]);
                    float fk[3];
                    shade_light<true>(lk, sp, *mp, (lit_mask >> k & 1u) != 0, &ls, fk);
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[j] = acc[j] + fk[j];
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) rgb[j] = fminf(acc[j], 1.0f);
            } else {
            shade_pixel(lc, t, sf, *mp, px, py, lit, rgb);
            }
        } else if ((fc.flags & MR_FRAME_SKYBOX) && sh.sky) {
            sky_color(fc, sh.sky, px, py, rgb);
        } else if (fc.background_u8 >> 24) {
            ready_u8 = true;       // the host already finalised the colour with NumPy itself (obj/core.py:600,640)
        }
        const size_t at_px = (size_t)py * fc.width + px;
        if (sh.frame && taps) { sh.frame[at_px * 3 + 0] = rgb[0]; sh.frame[at_px * 3 + 1] = rgb[1]; sh.frame[at_px * 3 + 2] = rgb[2]; }
        if (SS) {                                         // (the output pixel is written by a resolve)
            if (fused_ss) {
                float *s_rgb = reinterpret_cast<float *>(s_quad);
#pragma unroll
                for (int j = 0; j < 3; ++j) s_rgb[lp * 3 + j] = rgb[j];
            }
        } else {
            uint8_t *o = sh.out + ((size_t)out_row(fc, py, ltr) * fc.width + px) * 3;
            if (ready_u8) {
                o[0] = (uint8_t)fc.background_u8; o[1] = (uint8_t)(fc.background_u8 >> 8); o[2] = (uint8_t)(fc.background_u8 >> 16);
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) o[j] = gamma_u8(rgb[j], s_gamma);
            }
        }
        if (!ML && ta.zbuf && taps) {                     // taps for the parity tests / per-face status / overlay
            ta.zbuf[at_px] = zbest;
            ta.winner[at_px] = best;
            ta.stencil[at_px] = sten;
        }
    }
    // Fused resolve of a supersampled frame: after shading, where the register pressure has fallen.  The live samples'
    // colours are in the quad staging area (dead since phase 3; a dead sample's block is never read), and (16 / s)^2
    // threads finalise the output pixels.  (Uncovered background samples resolve from the float background like any
    // other: a uniform block keeps its colour exactly.)  SS_SEPARATE: k_resolve_full does it from the float frame.
    static_assert(TILE_PX * 3 * sizeof(float) <= sizeof(s_quad), "resolve staging fits the quad area");
    if (fused_ss) {
        __syncthreads();
        const TileKernArgs &ka = kernargs<TileKernArgs>();
        ss_resolve_tile(ka.fc, reinterpret_cast<const float *>(s_quad), ka.sh.out, gx, gy, tid, s_gamma);
    }

    // ---- per-tile statistics and housekeeping
    if (counters) {
        const unsigned long long cov = __ballot(covered), litm = __ballot(covered && lit);
        if (ML) {                                         // lit_px: the sum over the lights
            unsigned int v = covered ? n_lit : 0u;
#pragma unroll
            for (int off = WAVE / 2; off; off >>= 1) v += (unsigned int)__shfl_xor((int)v, off);
            if (lane == 0 && v) atomicAdd(&s_cnt[4], v);
        }
        if (lane == 0) {
            if (cov) atomicAdd(&s_cnt[3], (unsigned int)__popcll(cov));
            if (!ML && litm) atomicAdd(&s_cnt[4], (unsigned int)__popcll(litm));
            if (qfrags) atomicAdd(&s_cnt[1], qfrags);
            if (qupd) atomicAdd(&s_cnt[2], qupd);
        }
    }
    if (FULL) __syncthreads();
    // per-tile partial counts, summed by k_reduce_tile_stats (thousands of workgroups adding to
    // one cache line of counters would serialise at the memory side)
    const TileArgs &ta = kernargs<TileKernArgs>().ta;
    uint32_t *rec = ta.tile_stats + (size_t)tile * TILE_REC;
    if (FULL && tid < TILE_STATS) rec[tid] = s_cnt[tid];
    if (tid == 0) {                                       // list lengths; timing for mr_debug_read_tile_records
        rec[5] = n_small_raw; rec[6] = n_big_raw; rec[7] = n_quad_raw;
        // (frame-only: no stamp; with MR_QUAD_TILE_CULL=count the shadow quads the tile staged -- CULL, 0 elsewhere.  The general
        // kernel stored its first stamp when it took it)
        if (!FULL) rec[8] = (ta.quad_cull & 2u) ? q_kept : 0u;
        rec[9] = (uint32_t)stamp();
        rec[10] = (uint32_t)t_raster; rec[11] = (uint32_t)t_quads;
        if (n_small_raw > ta.cap[0]) { atomicOr(&ta.ctr->overflow, 1u); atomicMax(&ta.ctr->max_list[0], n_small_raw); }
        if (n_big_raw > ta.cap[1]) { atomicOr(&ta.ctr->overflow, 2u); atomicMax(&ta.ctr->max_list[1], n_big_raw); }
        if (n_quad_raw > ta.cap[2]) { atomicOr(&ta.ctr->overflow, 4u); atomicMax(&ta.ctr->max_list[2], n_quad_raw); }
    }
    if (tid < BIN_CLASSES) ta.bin_count[tid * n_tiles + tile] = 0;   // cursors zeroed for the next frame
    if (tid == 0) {                                       // what the slot's next frame should know about this tile
        int cls = tile_class(cost);
        // where tiles are split, class 1 holds those whose quad walk is worth sharing
        if (SPLIT) cls = (cost >= ta.split_cost && n_quad_raw >= ta.split_quads) ? 1 : cls < 2 ? 2 : cls;
        ta.tile_class[tile] = (uint8_t)cls;
    }
}

// The frame-only kernel (FULL == false, see tile_body) ...
template <bool SPLIT, bool SS, bool ML>
__global__ void __launch_bounds__(TILE_PX, ML ? K_TILE_WAVES : K_TILE_WAVES_1L)
k_tile(const TileKernArgs)            // read through kernargs<TileKernArgs>(), phase by phase
{
    tile_body<SPLIT, SS, ML, false>();
}
// ... and the general one: counted frames, per-face status, scenes with a depth_test == False model, mr_debug_force_full.
template <bool SPLIT, bool SS, bool ML>
__global__ void __launch_bounds__(TILE_PX, ML ? K_TILE_WAVES : K_TILE_WAVES_1L)
k_tile_full(const TileKernArgs)
{
    tile_body<SPLIT, SS, ML, true>();
}

// Sums the per-tile partial counts and list lengths into the frame counters; grid-stride over
// tiles, one atomic per workgroup and counter; run only when the statistics are asked for.  `counted` == 0: the frame's
// tile kernel was the frame-only one, which leaves words 0..4 of the records alone: only the list lengths are summed.
__global__ void __launch_bounds__(256)
k_reduce_tile_stats(const uint32_t *__restrict__ tile_stats, int n_tiles, Counters *__restrict__ ctr, int counted)
{
    constexpr int NS = TILE_STATS + 2;                    // + triangle pairs, all pairs
    __shared__ unsigned long long part[NS][256 / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + tid, gsz = (size_t)gridDim.x * blockDim.x;
    unsigned long long acc[NS] = {};
    for (size_t t = gid; t < (size_t)n_tiles; t += gsz) {
        const uint32_t *rec = tile_stats + t * TILE_REC;
#pragma unroll
        for (int k = 0; k < TILE_STATS; ++k) acc[k] += counted ? rec[k] : 0u;
        acc[TILE_STATS] += (unsigned long long)rec[5] + rec[6];
        acc[TILE_STATS + 1] += (unsigned long long)rec[5] + rec[6] + rec[7];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        unsigned long long v = acc[k];
        for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) part[k][wv] = v;
    }
    __syncthreads();
    if (tid < NS) {
        unsigned long long v = 0;
        for (int w = 0; w < 256 / WAVE; ++w) v += part[tid][w];
        if (tid < TILE_STATS) {
            unsigned long long *dst = tid == 0 ? &ctr->frag_tri : tid == 1 ? &ctr->frag_quad
                                    : tid == 2 ? &ctr->stencil_updates : tid == 3 ? &ctr->covered_px : &ctr->lit_px;
            if (v) atomicAdd(dst, v);
        } else if (v) {
            atomicAdd(tid == TILE_STATS ? &ctr->tri_bin_total : &ctr->bin_total, (unsigned int)v);
        }
    }
}

// Supersampled frames, resolved from the sample grid's float frame (row = screen y) instead of inside k_tile.
// k_resolve_touched: after k_overlay, which blended its lines into the float frame only, the output pixel that holds
// each touched sample is resolved again.  Several samples of one block write the same bytes: no dedupe needed.  The
// overlay's tile mask made k_tile write the float colour of every tile with a touched sample, and a block never
// leaves its tile, so every sample read here is there.
__global__ void __launch_bounds__(256)
k_resolve_touched(const int32_t *__restrict__ touched, int n_slots, const float *__restrict__ frame, int width, int band_y1,
                  int shift, const float *__restrict__ gamma_lut, uint8_t *__restrict__ out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n_slots) return;
    const int t = touched[i];
    const int py = (t / width) & ~((1 << shift) - 1), px = (t % width) & ~((1 << shift) - 1);
    float m[3];
    ss_block_mean(frame + ((size_t)py * width + px) * 3, width * 3, shift, m);
    uint8_t *o = ss_out_pixel(out, width, band_y1, shift, px, py);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = gamma_u8(m[c], gamma_lut);
}

// k_resolve_full: every output pixel of the band [band_y0, band_y1) (sample rows) from the float frame
// (MR_RESOLVE_PATH=separate: the yardstick of the fused resolve, and its A/B).  One thread per output pixel.
__global__ void __launch_bounds__(256)
k_resolve_full(const float *__restrict__ frame, int width, int band_y0, int band_y1, int shift,
               const float *__restrict__ gamma_lut, uint8_t *__restrict__ out)
{
    const int ow = width >> shift, oh = (band_y1 - band_y0) >> shift;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)ow * oh) return;
    const int orow = (int)(i / ow), ox = (int)(i - (long long)orow * ow);
    const int py = band_y1 - ((orow + 1) << shift), px = ox << shift;
    float m[3];
    ss_block_mean(frame + ((size_t)py * width + px) * 3, width * 3, shift, m);
    uint8_t *o = out + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = gamma_u8(m[c], gamma_lut);
}

}  // namespace mr
