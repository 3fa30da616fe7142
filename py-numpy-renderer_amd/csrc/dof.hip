// dof.hip -- the depth of field's kernel (kernels_dof.h) and its launch, the library's fourth translation unit and a
// code object of its own, like accum.hip and ao.hip: mi355rast.hip's code object keeps the frame's kernels at the
// addresses it held them at before.  host_dof.h calls the function below; a library linked without this file refuses the
// depth of field (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels_dof.h"

namespace mr_dof {

template <int TW, int TH, int BLOCK>
static void launch_shape(hipStream_t stream, const double *zbuf, const float *frame, float *out, int width, int height, const mr::DofParams &p)
{
    const dim3 grid((unsigned)((width + TW - 1) / TW), (unsigned)((height + TH - 1) / TH));
    hipLaunchKernelGGL((mr::k_dof<TW, TH, BLOCK>), grid, dim3(BLOCK), 0, stream, zbuf, frame, out, width, height, p);
}

// shape 0: workgroups of 32 x 32 samples and 1 024 threads; 1: 32 x 32 and 256, four samples a thread; 2: 16 x 16 and 256
// (MR_DOF_TILE, for the A/B in DESIGN.md 6j; host_dof.h picks the default)
void launch(hipStream_t stream, const double *zbuf, const float *frame, float *out, int width, int height, const mr::DofParams &p, int shape)
{
    if (shape == 2) launch_shape<16, 16, 256>(stream, zbuf, frame, out, width, height, p);
    else if (shape == 1) launch_shape<32, 32, 256>(stream, zbuf, frame, out, width, height, p);
    else launch_shape<32, 32, 1024>(stream, zbuf, frame, out, width, height, p);
}

}  // namespace mr_dof
