// accum.hip -- the accumulation's kernels (kernels_accum.h) and their launches, the library's second translation unit.
// They are kept out of mi355rast.hip's code object on purpose: that object then holds the frame's kernels at the
// addresses it held them at before the accumulation existed (see kernels_accum.h).  host_accum.h calls the two
// functions below; a library linked without this file refuses the accumulation (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kernels_accum.h"

namespace mr_accum {

void launch_add(hipStream_t stream, const float *frame, float *acc, size_t n_floats, float w, int first)
{
    const size_t want = std::max<size_t>(1, (n_floats / 4 + mr::ACCUM_BLOCK - 1) / mr::ACCUM_BLOCK);
    const unsigned blocks = (unsigned)std::min<size_t>(mr::ACCUM_MAX_BLOCKS, want);
    hipLaunchKernelGGL(mr::k_accum_add, dim3(blocks), dim3(mr::ACCUM_BLOCK), 0, stream, frame, acc, n_floats, w, first);
}

void launch_resolve(hipStream_t stream, const float *acc, int width, int height, int shift, float scale, const float *gamma_lut,
                    uint8_t *out)
{
    const long long n_px = (long long)(width >> shift) * (height >> shift);
    hipLaunchKernelGGL(mr::k_accum_resolve, dim3((unsigned)std::max<long long>(1, (n_px + 255) / 256)), dim3(256), 0, stream, acc,
                       width, height, shift, scale, gamma_lut, out);
}

}  // namespace mr_accum
