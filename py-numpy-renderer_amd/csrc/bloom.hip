// bloom.hip -- the bloom's three kernels (kernels_bloom.h) and their launches, the library's eighth translation unit and a
// code object of its own, like accum.hip, ao.hip, dof.hip, motion.hip, motion_faces.hip and taa.hip: mi355rast.hip's code
// object keeps the frame's kernels at the addresses it held them at before.  host_bloom.h calls the functions below; a
// library linked without this file refuses the bloom (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels_bloom.h"

namespace mr_bloom {

template <int TW, int TH>
static void down_shape(hipStream_t stream, const float *src, float *dst, int sw, int sh, int dw, int dh, float threshold, bool first)
{
    const dim3 grid((unsigned)((dw + TW - 1) / TW), (unsigned)((dh + TH - 1) / TH));
    if (first)
        hipLaunchKernelGGL((mr::k_bloom_down<true, TW, TH, TW * TH>), grid, dim3(TW * TH), 0, stream, src, dst, sw, sh, dw, dh, threshold);
    else
        hipLaunchKernelGGL((mr::k_bloom_down<false, TW, TH, TW * TH>), grid, dim3(TW * TH), 0, stream, src, dst, sw, sh, dw, dh, threshold);
}

// One level down: dst (bloom_half(sh) x bloom_half(sw)) from src (sh x sw); `first`: src is the float frame, and the bright
// pass is applied to it on the way in.  shape 0: workgroups of 32 x 8 output samples; 1: 64 x 4; 2: 16 x 16 -- 256
// threads each (MR_BLOOM_TILE, for the A/B in DESIGN.md 6n; host_env.h picks the default)
void launch_down(hipStream_t stream, const float *src, float *dst, int sw, int sh, float threshold, int first, int shape)
{
    const int dw = mr::bloom_half(sw), dh = mr::bloom_half(sh);
    if (shape == 2) down_shape<16, 16>(stream, src, dst, sw, sh, dw, dh, threshold, first != 0);
    else if (shape == 1) down_shape<64, 4>(stream, src, dst, sw, sh, dw, dh, threshold, first != 0);
    else down_shape<32, 8>(stream, src, dst, sw, sh, dw, dh, threshold, first != 0);
}

static dim3 up_grid(int w, int h)
{
    return dim3((unsigned)((w + mr::BLOOM_UP_TW - 1) / mr::BLOOM_UP_TW), (unsigned)((h + mr::BLOOM_UP_TH - 1) / mr::BLOOM_UP_TH));
}

// fine (h x w) += up(coarse), coarse (bloom_half(h) x bloom_half(w))
void launch_up(hipStream_t stream, float *fine, const float *coarse, int w, int h)
{
    hipLaunchKernelGGL(mr::k_bloom_up, up_grid(w, h), dim3(mr::BLOOM_UP_TW * mr::BLOOM_UP_TH), 0, stream, fine, coarse, w, h, mr::bloom_half(w),
                       mr::bloom_half(h));
}

// frame (h x w) += gain * up(coarse)
void launch_composite(hipStream_t stream, float *frame, const float *coarse, int w, int h, float gain)
{
    hipLaunchKernelGGL(mr::k_bloom_composite, up_grid(w, h), dim3(mr::BLOOM_UP_TW * mr::BLOOM_UP_TH), 0, stream, frame, coarse, w, h,
                       mr::bloom_half(w), mr::bloom_half(h), gain);
}

}  // namespace mr_bloom
