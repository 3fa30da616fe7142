// ao.hip -- the ambient obscurance's kernel (kernels_ao.h) and its launch, the library's third translation unit and a
// code object of its own, like accum.hip: mi355rast.hip's code object keeps the frame's kernels at the addresses it
// held them at before.  host_ao.h calls the function below; a library linked without this file refuses the obscurance
// (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels_ao.h"

namespace mr_ao {

template <int TW, int TH, int BLOCK>
static void launch_shape(hipStream_t stream, const double *zbuf, float *frame, int width, int height, const mr::AoParams &p)
{
    const dim3 grid((unsigned)((width + TW - 1) / TW), (unsigned)((height + TH - 1) / TH));
    hipLaunchKernelGGL((mr::k_ao<TW, TH, BLOCK>), grid, dim3(BLOCK), 0, stream, zbuf, frame, width, height, p);
}

// shape 0: workgroups of 64 x 64 samples and 1 024 threads; 1: 32 x 32 and 256; 2: 64 x 16 and 256 (MR_AO_TILE, for the
// A/B in DESIGN.md 6i; host_ao.h picks the default)
void launch(hipStream_t stream, const double *zbuf, float *frame, int width, int height, const mr::AoParams &p, int shape)
{
    if (shape == 2) launch_shape<64, 16, 256>(stream, zbuf, frame, width, height, p);
    else if (shape == 1) launch_shape<32, 32, 256>(stream, zbuf, frame, width, height, p);
    else launch_shape<64, 64, 1024>(stream, zbuf, frame, width, height, p);
}

}  // namespace mr_ao
