// shafts.hip -- the light shafts' three kernels (kernels_shafts.h) and their launches, the library's ninth translation unit
// and a code object of its own, like accum.hip, ao.hip, dof.hip, motion.hip, motion_faces.hip, taa.hip and bloom.hip:
// mi355rast.hip's code object keeps the frame's kernels at the addresses it held them at before.  host_shafts.h calls the
// functions below; a library linked without this file refuses the pass (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels_shafts.h"

namespace mr_shafts {

template <int D>
static void source_levels(hipStream_t stream, const mr::ShaftSrc &a, float *dst, int dw, int dh)
{
    // (a thread a coarse sample up to D = 2, a thread a column of four samples of the grid above: kernels_shafts.h)
    const int across = D <= 2 ? dw : (a.w + 3) / 4;
    const dim3 grid((unsigned)((across + mr::SHAFT_SRC_TW - 1) / mr::SHAFT_SRC_TW), (unsigned)((dh + mr::SHAFT_SRC_TH - 1) / mr::SHAFT_SRC_TH));
    hipLaunchKernelGGL((mr::k_shaft_source<D>), grid, dim3(mr::SHAFT_SRC_TW * mr::SHAFT_SRC_TH), 0, stream, a, reinterpret_cast<float4 *>(dst), dw, dh);
}

// S (dh x dw, 16 bytes a sample) from the float frame and the z-buffer (h x w); (dh, dw) is (h, w) halved `levels` times
void launch_source(hipStream_t stream, const float *frame, const double *zbuf, float *dst, int w, int h, int dw, int dh, float threshold, int levels)
{
    mr::ShaftSrc a;
    a.frame = frame; a.zbuf = zbuf; a.w = w; a.h = h; a.threshold = threshold;
    a.wide = w % 4 == 0 && (reinterpret_cast<uintptr_t>(frame) | reinterpret_cast<uintptr_t>(zbuf)) % 16 == 0;
    if (levels == 1) source_levels<1>(stream, a, dst, dw, dh);
    else if (levels == 2) source_levels<2>(stream, a, dst, dw, dh);
    else if (levels == 3) source_levels<3>(stream, a, dst, dw, dh);
    else source_levels<4>(stream, a, dst, dw, dh);
}

// R from S, both (h x w), 16 bytes a sample
void launch_march(hipStream_t stream, const float *src, float *dst, int w, int h, const mr::ShaftsParams &p)
{
    const dim3 grid((unsigned)((w + mr::SHAFT_MARCH_T - 1) / mr::SHAFT_MARCH_T), (unsigned)((h + mr::SHAFT_MARCH_T - 1) / mr::SHAFT_MARCH_T));
    hipLaunchKernelGGL(mr::k_shaft_march, grid, dim3(mr::SHAFT_MARCH_T * mr::SHAFT_MARCH_T), 0, stream, reinterpret_cast<const float4 *>(src),
                       reinterpret_cast<float4 *>(dst), w, h, p);
}

// frame (h x w) += gain * fetch(R), R (ch x cw)
void launch_composite(hipStream_t stream, float *frame, const float *coarse, int w, int h, int cw, int ch, int levels, float gain)
{
    const dim3 grid((unsigned)((w + mr::SHAFT_COMP_TW - 1) / mr::SHAFT_COMP_TW), (unsigned)((h + mr::SHAFT_COMP_TH - 1) / mr::SHAFT_COMP_TH));
    hipLaunchKernelGGL(mr::k_shaft_composite, grid, dim3(mr::SHAFT_COMP_TW * mr::SHAFT_COMP_TH), 0, stream, frame, reinterpret_cast<const float4 *>(coarse),
                       w, h, cw, ch, mr::shafts_inv_scale(levels), gain);
}

}  // namespace mr_shafts
