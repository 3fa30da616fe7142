// motion.hip -- the motion blur's two kernels (kernels_motion.h) and their launches, the library's fifth translation unit
// and a code object of its own, like accum.hip, ao.hip and dof.hip: mi355rast.hip's code object keeps the frame's kernels
// at the addresses it held them at before.  host_motion.h calls the functions below; a library linked without this file
// refuses the motion blur (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels_motion.h"

namespace mr_motion {

void launch_velocity(hipStream_t stream, const double *zbuf, const int32_t *winner, const double *tables, float *vel, int width, int height,
                     const mr::MotionParams &p)
{
    const size_t n = (size_t)width * height;
    const unsigned blocks = (unsigned)((n + mr::VELOCITY_BLOCK - 1) / mr::VELOCITY_BLOCK);
    hipLaunchKernelGGL(mr::k_velocity, dim3(blocks), dim3(mr::VELOCITY_BLOCK), 0, stream, zbuf, winner, tables, reinterpret_cast<float2 *>(vel),
                       width, height, p);
}

template <int TW, int TH, int BLOCK>
static void blur_shape(hipStream_t stream, const double *zbuf, const float *vel, const float *frame, float *out, int width, int height,
                       const mr::MotionParams &p)
{
    const dim3 grid((unsigned)((width + TW - 1) / TW), (unsigned)((height + TH - 1) / TH));
    hipLaunchKernelGGL((mr::k_mblur<TW, TH, BLOCK>), grid, dim3(BLOCK), 0, stream, zbuf, reinterpret_cast<const float2 *>(vel), frame, out,
                       width, height, p);
}

// shape 0: workgroups of 32 x 32 samples and 1 024 threads; 1: 32 x 32 and 256, four samples a thread; 2: 16 x 16 and 256
// (MR_MBLUR_TILE, for the A/B in DESIGN.md 6k; host_motion.h picks the default)
void launch_blur(hipStream_t stream, const double *zbuf, const float *vel, const float *frame, float *out, int width, int height,
                 const mr::MotionParams &p, int shape)
{
    if (shape == 2) blur_shape<16, 16, 256>(stream, zbuf, vel, frame, out, width, height, p);
    else if (shape == 1) blur_shape<32, 32, 256>(stream, zbuf, vel, frame, out, width, height, p);
    else blur_shape<32, 32, 1024>(stream, zbuf, vel, frame, out, width, height, p);
}

}  // namespace mr_motion
