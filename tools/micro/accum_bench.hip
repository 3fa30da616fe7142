// The accumulation's two kernels alone (csrc/kernels_accum.h), away from the frames they follow in the library: device
// time of k_accum_add repeated back to back on one pair of buffers -- the sum it read and wrote a moment ago is as warm
// as it can be -- and of k_accum_resolve, with the bytes each moves as GB/s.  tools/time_accumulate.py reports the same
// kernels inside the real sequence (a frame's kernels between two adds).
//
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -I py-numpy-renderer_amd/csrc \
//         -o tools/micro/accum_bench tools/micro/accum_bench.hip
//   tools/micro/accum_bench [height width [shift]]          (default 1080 1920 0)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels_accum.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main(int argc, char **argv)
{
    const int height = argc > 2 ? atoi(argv[1]) : 1080, width = argc > 2 ? atoi(argv[2]) : 1920, shift = argc > 3 ? atoi(argv[3]) : 0;
    if (height <= 0 || width <= 0 || shift < 0 || shift > 2 || height % (1 << shift) || width % (1 << shift)) { printf("bad size\n"); return 1; }
    const size_t n = (size_t)height * width * 3, out_bytes = (size_t)(height >> shift) * (width >> shift) * 3;
    std::vector<float> frame(n), lut(mr::GAMMA_LUT_SIZE);
    uint32_t x = 12345u;
    for (float &f : frame) { x = x * 1664525u + 1013904223u; f = (float)(x >> 8) / 16777216.0f; }
    for (int k = 0; k < 256; ++k) lut[k] = powf((float)k / 255.0f, 1.25f);       // (near enough for a timing)
    lut[256] = INFINITY;
    float *d_frame, *d_acc, *d_lut;
    uint8_t *d_out;
    CK(hipMalloc(&d_frame, n * 4)); CK(hipMalloc(&d_acc, n * 4)); CK(hipMalloc(&d_lut, lut.size() * 4)); CK(hipMalloc(&d_out, out_bytes));
    CK(hipMemcpy(d_frame, frame.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_lut, lut.data(), lut.size() * 4, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)std::min<size_t>(mr::ACCUM_MAX_BLOCKS, std::max<size_t>(1, (n / 4 + mr::ACCUM_BLOCK - 1) / mr::ACCUM_BLOCK));
    const long long n_px = (long long)(height >> shift) * (width >> shift);
    constexpr int REPS = 50;
    hipEvent_t ev[REPS + 1];
    for (auto &mark : ev) CK(hipEventCreate(&mark));
    auto report = [&](const char *what, double bytes) {
        std::vector<float> us;
        for (int i = 0; i < REPS; ++i) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]); us.push_back(ms * 1e3f); }
        std::sort(us.begin(), us.end());
        printf("%-28s %4d x %4d shift %d: %7.1f / %7.1f us (minimum / median of %d), %6.1f MB -> %7.1f GB/s at the median\n", what, height, width,
               shift, us[0], us[REPS / 2], REPS, bytes / 1e6, bytes / (us[REPS / 2] * 1e-6) / 1e9);
    };
    // the first add writes the sum without reading it
    hipLaunchKernelGGL(mr::k_accum_add, dim3(blocks), dim3(mr::ACCUM_BLOCK), 0, 0, d_frame, d_acc, n, 0.5f, 1);
    CK(hipDeviceSynchronize());
    for (int first = 1; first >= 0; --first) {
        for (int i = 0; i < REPS; ++i) {
            CK(hipEventRecord(ev[i], 0));
            hipLaunchKernelGGL(mr::k_accum_add, dim3(blocks), dim3(mr::ACCUM_BLOCK), 0, 0, d_frame, d_acc, n, 0.001f, first);
        }
        CK(hipEventRecord(ev[REPS], 0));
        CK(hipDeviceSynchronize());
        report(first ? "k_accum_add, first (1r + 1w)" : "k_accum_add (2r + 1w)", (first ? 2.0 : 3.0) * n * 4);
    }
    // a sample of the sum against the same chain on the host
    std::vector<float> got(n);
    CK(hipMemcpy(got.data(), d_acc, n * 4, hipMemcpyDeviceToHost));
    size_t wrong = 0;
    for (size_t i = 0; i < n; i += 997) {
        float a = 0.001f * frame[i];
        for (int k = 0; k < REPS; ++k) a = a + 0.001f * frame[i];
        wrong += a != got[i];
    }
    for (size_t i = n - 5; i < n; ++i) {                                    // (the tail, where n % 4 != 0)
        float a = 0.001f * frame[i];
        for (int k = 0; k < REPS; ++k) a = a + 0.001f * frame[i];
        wrong += a != got[i];
    }
    printf("sampled sums that differ from the host's chain: %zu\n", wrong);
    for (int i = 0; i < REPS; ++i) {
        CK(hipEventRecord(ev[i], 0));
        hipLaunchKernelGGL(mr::k_accum_resolve, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, 0, d_acc, width, height, shift, 1.0f, d_lut, d_out);
    }
    CK(hipEventRecord(ev[REPS], 0));
    CK(hipDeviceSynchronize());
    report("k_accum_resolve (1r + bytes)", (double)n * 4 + (double)out_bytes);
    CK(hipGetLastError());
    return wrong ? 1 : 0;
}
