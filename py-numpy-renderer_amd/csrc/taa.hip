// taa.hip -- the temporal anti-aliasing's kernel (kernels_taa.h) and its launch, the library's seventh translation unit
// and a code object of its own, like accum.hip, ao.hip, dof.hip, motion.hip and motion_faces.hip: mi355rast.hip's code
// object keeps the frame's kernels at the addresses it held them at before.  host_taa.h calls the function below; a
// library linked without this file refuses the temporal anti-aliasing (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels_taa.h"

namespace mr_taa {

template <int TW, int TH>
static void launch_shape(hipStream_t stream, const float *frame, const float *vel, const float *hist, float *out, float *hist_out, int width,
                         int height, const mr::TaaParams &p)
{
    const dim3 grid((unsigned)((width + TW - 1) / TW), (unsigned)((height + TH - 1) / TH));
    hipLaunchKernelGGL((mr::k_taa<TW, TH, TW * TH>), grid, dim3(TW * TH), 0, stream, frame, reinterpret_cast<const float2 *>(vel), hist, out,
                       hist_out, width, height, p);
}

// shape 0: workgroups of 32 x 8 samples; 1: 64 x 4; 2: 16 x 16 -- 256 threads each (MR_TAA_TILE, for the A/B in DESIGN.md
// 6m; host_env.h picks the default).  hist may be NULL: no history
void launch(hipStream_t stream, const float *frame, const float *vel, const float *hist, float *out, float *hist_out, int width, int height,
            const mr::TaaParams &p, int shape)
{
    if (shape == 2) launch_shape<16, 16>(stream, frame, vel, hist, out, hist_out, width, height, p);
    else if (shape == 1) launch_shape<64, 4>(stream, frame, vel, hist, out, hist_out, width, height, p);
    else launch_shape<32, 8>(stream, frame, vel, hist, out, hist_out, width, height, p);
}

}  // namespace mr_taa
