// kernels_tonemap.h -- k_lum_hist, k_exposure, k_tone_apply: tone mapping with an exposure metered from a luminance
// histogram (tonemap_def.h has the definition).  A metered frame runs the three, dependent, on its stream: the exposure
// reaches k_tone_apply through a cell in device memory and the host is not in between.  A frame with a fixed exposure runs
// k_tone_apply alone.
//
// k_lum_hist streams the float frame once: a thread takes four whole samples as three 16-byte loads, the samples past the
// last multiple of four go to the first threads of workgroup 0 as scalars.  The grid is capped and walks the frame in a
// grid-stride loop (as k_accum_add does).  A workgroup counts into 256 uint32 bins in LDS (1 024 bytes) with LDS atomics
// and then writes its 256 counts with PLAIN stores into its own row of the slot's slab, grid x 256 words: no global
// atomic (a uniform sky would put every workgroup on one address, 11 to 15 ns each: profiles/r03_atomic_same_address.txt),
// no memset -- every workgroup of the grid writes its whole row, whatever it counted.  Two forms, the same counts:
//
//   BALLOT = false   every lane adds 1 to its sample's bin: on a uniform frame 64 lanes hit one LDS address
//   BALLOT = true    a wavefront adds once per distinct bin: a leader's bin, the ballot of the lanes that share it, one add
//                    of the popcount by the leader -- one round on a uniform frame, up to 64 on noise
//
// k_exposure is ONE workgroup of 256 threads.  The slab's columns are summed with 16-byte loads: a wavefront reads a whole
// 1 KB row, a lane four columns of it, wavefront g the rows g, g + 4, ..., eight of them in flight a lane -- one workgroup
// has only the loads it keeps in flight to hide the memory's latency with (a thread a column and a row a trip measured
// 0.14 us a row, the latency itself: profiles/tonemap_time.txt) -- and the four wavefronts' partial sums meet in LDS, so
// that thread i holds n[i].  An inclusive scan over the 256 bins in LDS gives C_i, S and M are reduced in int64 in LDS,
// and lane 0 forms q, e_t and e, writes e to the slot's exposure cell and, for an adaptive scene, to the scene's next
// state cell.  The summed histogram (n[0] := 0) stays in the slot's 256 words.  LDS: 1 024 + 2 x 2 048 = 5 120 bytes (the
// partial sums lie where S and M are reduced later).
//
// k_tone_apply streams the float frame in place, 16 bytes a lane and access with a scalar tail; the operator is a template
// argument.  It reads e from the cell, or takes it as an argument where it is fixed (cell == nullptr).  No LDS.
//
// No scratch.  Compiled in tonemap.hip, a translation unit and a code object of its own, like the other passes' kernels
// (kernels_accum.h).
#pragma once

#include "tonemap_def.h"

namespace mr {

constexpr int TONE_BLOCK = 256;
constexpr unsigned TONE_APPLY_MAX_BLOCKS = 2048;         // k_tone_apply's, as k_accum_add's
constexpr int TONE_HIST_LDS = TONE_BINS * 4;             // bytes of LDS: k_lum_hist ...
constexpr int TONE_EXPOSURE_LDS = TONE_BINS * (4 + 8 + 8);   // ... and k_exposure
static_assert(TONE_BLOCK == TONE_BINS, "a thread a bin");

template <bool BALLOT>
__device__ inline void tone_count(uint32_t *s_n, bool live, int bin)
{
    if (!BALLOT) {
        if (live) atomicAdd(&s_n[bin], 1u);
        return;
    }
    // (every lane of the wavefront is here: the caller's loop has one trip count for the workgroup)
    const int lane = (int)(threadIdx.x & 63u);
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const int lead_bin = __shfl(bin, leader);
        const unsigned long long same = __ballot(live && bin == lead_bin);
        if (lane == leader) atomicAdd(&s_n[lead_bin], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// frame: n_samples x 3 floats, 16-byte aligned; slab: gridDim.x rows of 256 words
template <bool BALLOT>
__global__ void __launch_bounds__(TONE_BLOCK)
k_lum_hist(const float *__restrict__ frame, size_t n_samples, uint32_t *__restrict__ slab)
{
    __shared__ uint32_t s_n[TONE_BINS];
    static_assert(sizeof(s_n) == (size_t)TONE_HIST_LDS, "the LDS this header states");
    const int tid = (int)threadIdx.x;
    s_n[tid] = 0;
    __syncthreads();
    const size_t n4 = n_samples / 4, stride = (size_t)gridDim.x * TONE_BLOCK;
    const float4 *f4 = reinterpret_cast<const float4 *>(frame);
    for (size_t base = (size_t)blockIdx.x * TONE_BLOCK; base < n4; base += stride) {
        const size_t i = base + tid;
        const bool live = i < n4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
        if (live) { a = f4[3 * i]; b = f4[3 * i + 1]; c = f4[3 * i + 2]; }
        tone_count<BALLOT>(s_n, live, tone_bin(a.x, a.y, a.z));
        tone_count<BALLOT>(s_n, live, tone_bin(a.w, b.x, b.y));
        tone_count<BALLOT>(s_n, live, tone_bin(b.z, b.w, c.x));
        tone_count<BALLOT>(s_n, live, tone_bin(c.y, c.z, c.w));
    }
    const size_t t = n4 * 4 + tid;
    if (blockIdx.x == 0 && t < n_samples) atomicAdd(&s_n[tone_bin(frame[3 * t], frame[3 * t + 1], frame[3 * t + 2])], 1u);
    __syncthreads();
    slab[(size_t)blockIdx.x * TONE_BINS + tid] = s_n[tid];
}

// slab: rows x 256 words; e_prev: the scene's previous exposure, nullptr without one; hist: 256 words; e_cell: the frame's
// exposure; e_next: the scene's next state cell, nullptr where the scene keeps none
__global__ void __launch_bounds__(TONE_BLOCK)
k_exposure(const uint32_t *__restrict__ slab, int rows, ToneMeter meter, const float *__restrict__ e_prev, uint32_t *__restrict__ hist,
           float *__restrict__ e_cell, float *__restrict__ e_next)
{
    __shared__ uint32_t s_c[TONE_BINS];
    __shared__ __attribute__((aligned(16))) long long s_sm[2 * TONE_BINS];
    static_assert(sizeof(s_c) + sizeof(s_sm) == (size_t)TONE_EXPOSURE_LDS, "the LDS this header states");
    static_assert(sizeof(s_sm) == 4 * TONE_BINS * sizeof(uint32_t), "four wavefronts' partial sums fit where S and M are reduced");
    long long *s_s = s_sm, *s_m = s_sm + TONE_BINS;
    const int i = (int)threadIdx.x;
    {   // the columns' sums: lane l of wavefront g takes columns 4 l .. 4 l + 3 of the rows g, g + 4, ...
        const int quad = i & 63, wave = i >> 6;
        const uint4 *rows4 = reinterpret_cast<const uint4 *>(slab);
        uint4 acc = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 8
        for (int r = wave; r < rows; r += 4) {
            const uint4 v = rows4[(size_t)r * (TONE_BINS / 4) + quad];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        reinterpret_cast<uint4 *>(s_sm)[wave * (TONE_BINS / 4) + quad] = acc;
    }
    __syncthreads();
    const uint32_t *s_p = reinterpret_cast<const uint32_t *>(s_sm);
    uint32_t n = (s_p[i] + s_p[TONE_BINS + i]) + (s_p[2 * TONE_BINS + i] + s_p[3 * TONE_BINS + i]);
    if (i == 0) n = 0;                                       // black is metered out
    hist[i] = n;
    s_c[i] = n;
    __syncthreads();
    for (int d = 1; d < TONE_BINS; d <<= 1) {                // the inclusive scan
        const uint32_t below = i >= d ? s_c[i - d] : 0u;
        __syncthreads();
        s_c[i] += below;
        __syncthreads();
    }
    const int64_t total = s_c[TONE_BINS - 1], c = (int64_t)s_c[i] - n;
    const int64_t lo = total * meter.low_pm / 1000, hi = total * meter.high_pm / 1000;
    const int64_t u = tone_kept(c, n, lo, hi);
    s_s[i] = u * tone_centre(i);
    s_m[i] = u;
    __syncthreads();
    for (int d = TONE_BINS / 2; d >= 1; d >>= 1) {
        if (i < d) { s_s[i] += s_s[i + d]; s_m[i] += s_m[i + d]; }
        __syncthreads();
    }
    if (i == 0) {
        const float e = tone_exposure(s_s[0], s_m[0], meter, e_prev != nullptr, e_prev ? *e_prev : 1.0f);
        *e_cell = e;
        if (e_next) *e_next = e;
    }
}

// frame: n_floats floats, 16-byte aligned, rewritten in place; e: *e_cell, or e_fixed where e_cell is nullptr
template <int OP>
__global__ void __launch_bounds__(TONE_BLOCK)
k_tone_apply(float *__restrict__ frame, size_t n_floats, const float *__restrict__ e_cell, float e_fixed, float white2)
{
    const float e = e_cell ? *e_cell : e_fixed;
    const size_t n4 = n_floats / 4, stride = (size_t)gridDim.x * TONE_BLOCK;
    const size_t lane = (size_t)blockIdx.x * TONE_BLOCK + threadIdx.x;
    float4 *f4 = reinterpret_cast<float4 *>(frame);
    for (size_t i = lane; i < n4; i += stride) {
        const float4 f = f4[i];
        f4[i] = make_float4(tone_curve<OP>(f.x, e, white2), tone_curve<OP>(f.y, e, white2), tone_curve<OP>(f.z, e, white2),
                            tone_curve<OP>(f.w, e, white2));
    }
    const size_t t = n4 * 4 + lane;
    if (t < n_floats) frame[t] = tone_curve<OP>(frame[t], e, white2);
}

}  // namespace mr
