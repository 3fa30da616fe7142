// Micro-benchmark: how much straight-line code a CU of MI355X runs at full speed, and what it costs beyond that.
//   hipcc -O3 --offload-arch=gfx950 -o tools/micro/icache_footprint tools/micro/icache_footprint.hip && tools/micro/icache_footprint
// A loop whose body is FOOTPRINT bytes of independent v_add_u32 (4 bytes each, four accumulators in turn), generated
// at compile time per footprint (template parameter -> .rept), run by six wavefronts per SIMD (256-thread workgroups,
// LDS ballast so that exactly six fit a CU), some two million instructions per wavefront whatever the footprint.
// Two clocks per wavefront: s_memtime (shader cycles) and s_memrealtime (100 MHz).  Reported per footprint, for the median
// wavefront: cycles per wave-instruction AS THE WAVEFRONT SEES THEM (issue cost x wavefronts sharing the SIMD) and the SIMD
// time per wave-instruction in ns (the wavefront's time / wavefronts per SIMD) --
//   alone: one kernel, six workgroups per CU;
//   pair:  two DIFFERENT kernels of that footprint each (separate code: 2 x the bytes), three workgroups per CU each, on two
//          streams at once; "mixed" is the share of CUs that ran wavefronts of both (read from HW_ID / XCC_ID), since
//          nothing forces the dispatcher to mix them.
// The knee of the first column is the instruction cache's capacity as a CU sees it, the slope beyond it the cost of a
// miss; the second column says whether two co-resident kernels share that capacity.
// First line: the 8 KB loop with 1, 2, 4 and 6 wavefronts per SIMD.  Cycles per instruction as a wavefront sees them must
// grow in proportion to the wavefronts once the SIMD is saturated: that is the check that six are resident.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include <algorithm>
#include <set>
#include <map>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

constexpr int PER_WAVE = 1 << 21;          // wave-instructions of the body per wavefront, to within a trip of the loop
constexpr int trips(int kb) { return PER_WAVE / (kb * 256); }              // four 4-byte instructions per group, kb * 64 groups
constexpr int insts(int kb) { return trips(kb) * kb * 256; }
constexpr int WAVES_PER_SIMD = 6;

// WHICH: 0 / 1 are two copies of the same loop at different addresses.  The back edge is a computed jump: a footprint
// of 256 KB is beyond the reach of s_cbranch (+-128 KB).
template <int KB, int WHICH>
__global__ void __launch_bounds__(256) k_loop(uint32_t *out, uint64_t *out_t, uint32_t *out_id, uint32_t seed)
{
    extern __shared__ uint32_t s_ballast[];
    if (seed == 0xffffffffu) s_ballast[threadIdx.x] = seed;
    constexpr int GROUPS = KB * 1024 / 16;                 // four 4-byte instructions per group
    constexpr int TRIPS = trips(KB);
    static_assert(TRIPS >= 1 && GROUPS * 4 == KB * 256, "trips()");
    uint32_t a = seed + threadIdx.x, b = a + 1, c = a + 2, d = a + 3;
    const uint32_t k = seed | 1u;
    __syncthreads();
    const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_mov_b32 s20, %5\n"
                 "1:\n"
                 ".rept %6\n"
                 "v_add_u32 %0, %0, %4\n v_add_u32 %1, %1, %4\n v_add_u32 %2, %2, %4\n v_add_u32 %3, %3, %4\n"
                 ".endr\n"
                 "s_sub_u32 s20, s20, 1\n"
                 "s_cmp_eq_u32 s20, 0\n"
                 "s_cbranch_scc1 2f\n"
                 "s_getpc_b64 s[22:23]\n"
                 "3:\n"
                 "s_sub_u32 s22, s22, 3b-1b\n"
                 "s_subb_u32 s23, s23, 0\n"
                 "s_setpc_b64 s[22:23]\n"
                 "2:\n"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "v"(k), "i"(TRIPS), "i"(GROUPS) : "s20", "s22", "s23", "scc");
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / 64;
    out[blockIdx.x * blockDim.x + threadIdx.x] = a + b + c + d;
    if ((threadIdx.x & 63) == 0) {
        out_t[2 * wave] = t1 - t0; out_t[2 * wave + 1] = r1 - r0;
        // where it ran: XCC_ID (register 20) and SE / SH / CU of HW_ID (register 4)
        const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        out_id[wave] = ((xcc & 0xfu) << 16) | (hw & 0xff00u);      // HW_ID bits 8..11 CU, 12 SH, 13..15 SE
    }
}

struct Result { double cyc_alone, ns_alone, cyc_pair, ns_pair, mixed; };

template <int KB>
int run(Result &r, int waves = WAVES_PER_SIMD, bool pair = true)
{
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const size_t lds = waves == 1 ? (size_t)64 * 1024 : (size_t)(160 * 1024 / waves) - 1024;     // exactly `waves` workgroups fit a CU (one: more than a third of its LDS; a workgroup may take 64 KB)
    const int max_blocks = cus * waves;
    uint32_t *d_out[2], *d_id[2]; uint64_t *d_t[2];
    hipStream_t st[2];
    for (int i = 0; i < 2; ++i) {
        CK(hipMalloc(&d_out[i], (size_t)max_blocks * 256 * 4));
        CK(hipMalloc(&d_t[i], (size_t)max_blocks * 4 * 2 * 8));
        CK(hipMalloc(&d_id[i], (size_t)max_blocks * 4 * 4));
        CK(hipStreamCreate(&st[i]));
    }
    auto median_ns = [&](int which, int blocks, double &cyc, double &ns) -> int {
        std::vector<uint64_t> both((size_t)blocks * 4 * 2), t((size_t)blocks * 4), rt((size_t)blocks * 4);
        CK(hipMemcpy(both.data(), d_t[which], both.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < t.size(); ++i) { t[i] = both[2 * i]; rt[i] = both[2 * i + 1]; }
        std::sort(t.begin(), t.end()); std::sort(rt.begin(), rt.end());
        cyc = (double)t[t.size() / 2] / insts(KB);                          // s_memtime: shader cycles, as the wavefront sees them
        ns = (double)rt[rt.size() / 2] * 10.0 / insts(KB) / waves;          // s_memrealtime: 100 MHz; SIMD time
        return 0;
    };
    // alone (the first launch loads the code and is not read)
    for (int rep = 0; rep < 2; ++rep)
        hipLaunchKernelGGL((k_loop<KB, 0>), dim3(max_blocks), dim3(256), lds, st[0], d_out[0], d_t[0], d_id[0], 12345u);
    CK(hipDeviceSynchronize());
    if (median_ns(0, max_blocks, r.cyc_alone, r.ns_alone)) return 1;
    if (!pair) { for (int i = 0; i < 2; ++i) { CK(hipFree(d_out[i])); CK(hipFree(d_t[i])); CK(hipFree(d_id[i])); CK(hipStreamDestroy(st[i])); } return 0; }
    // two kernels at once, three workgroups per CU each
    const int half = cus * waves / 2;
    for (int rep = 0; rep < 2; ++rep) {
        CK(hipDeviceSynchronize());
        hipLaunchKernelGGL((k_loop<KB, 0>), dim3(half), dim3(256), lds, st[0], d_out[0], d_t[0], d_id[0], 12345u);
        hipLaunchKernelGGL((k_loop<KB, 1>), dim3(half), dim3(256), lds, st[1], d_out[1], d_t[1], d_id[1], 54321u);
    }
    CK(hipDeviceSynchronize());
    double n0 = 0, n1 = 0, c0 = 0, c1 = 0;
    if (median_ns(0, half, c0, n0) || median_ns(1, half, c1, n1)) return 1;
    r.ns_pair = 0.5 * (n0 + n1); r.cyc_pair = 0.5 * (c0 + c1);
    std::set<uint32_t> where[2];
    for (int i = 0; i < 2; ++i) {
        std::vector<uint32_t> id((size_t)half * 4);
        CK(hipMemcpy(id.data(), d_id[i], id.size() * 4, hipMemcpyDeviceToHost));
        where[i].insert(id.begin(), id.end());
    }
    size_t both = 0;
    std::set<uint32_t> any = where[0];
    any.insert(where[1].begin(), where[1].end());
    for (uint32_t c : where[0]) both += where[1].count(c);
    r.mixed = any.empty() ? 0.0 : (double)both / (double)any.size();
    for (int i = 0; i < 2; ++i) { CK(hipFree(d_out[i])); CK(hipFree(d_t[i])); CK(hipFree(d_id[i])); CK(hipStreamDestroy(st[i])); }
    return 0;
}

template <int KB>
int report()
{
    Result r = {};
    if (run<KB>(r)) return 1;
    printf("%4d KB   alone %6.2f cyc/inst/wave %6.3f ns   pair (2 x %3d KB) %6.2f cyc/inst/wave %6.3f ns   mixed CUs %3.0f %%\n",
           KB, r.cyc_alone, r.ns_alone, KB, r.cyc_pair, r.ns_pair, 100.0 * r.mixed);
    return 0;
}

int main()
{
    printf("8 KB loop, cycles per wave-instruction as a wavefront sees them, by wavefronts per SIMD:");
    for (int w : { 1, 2, 4, 6 }) {
        Result r = {};
        if (run<8>(r, w, false)) return 1;
        printf("  %d: %.2f (%.3f ns SIMD time)", w, r.cyc_alone, r.ns_alone);
    }
    printf("\nv_add_u32, %d wavefronts per SIMD, by the loop's footprint\n", WAVES_PER_SIMD);
    if (report<8>() || report<16>() || report<32>() || report<48>() || report<64>() || report<96>() || report<128>() || report<256>()) return 1;
    return 0;
}
