// tonemap.hip -- the tone mapping's three kernels (kernels_tonemap.h) and their launches, the library's tenth translation
// unit and a code object of its own, like accum.hip, ao.hip, dof.hip, motion.hip, motion_faces.hip, taa.hip, bloom.hip and
// shafts.hip: mi355rast.hip's code object keeps the frame's kernels at the addresses it held them at before.
// host_tonemap.h calls the functions below; a library linked without this file refuses the tone mapping
// (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kernels_tonemap.h"

namespace mr_tonemap {

// the grid of k_lum_hist on n_samples samples under a cap in 1 .. TONE_MAX_BLOCKS: the slab's rows
unsigned hist_grid(size_t n_samples, unsigned cap)
{
    const size_t want = std::max<size_t>(1, (n_samples / 4 + mr::TONE_BLOCK - 1) / mr::TONE_BLOCK);
    return (unsigned)std::min<size_t>(std::min(cap, mr::TONE_MAX_BLOCKS), want);
}

// slab (grid x 256 words) from the frame; form 0: an LDS add a sample, 1: an add per distinct bin of a wavefront
void launch_hist(hipStream_t stream, const float *frame, size_t n_samples, uint32_t *slab, unsigned grid, int form)
{
    if (form) hipLaunchKernelGGL(mr::k_lum_hist<true>, dim3(grid), dim3(mr::TONE_BLOCK), 0, stream, frame, n_samples, slab);
    else hipLaunchKernelGGL(mr::k_lum_hist<false>, dim3(grid), dim3(mr::TONE_BLOCK), 0, stream, frame, n_samples, slab);
}

void launch_exposure(hipStream_t stream, const uint32_t *slab, unsigned rows, const mr::ToneMeter &meter, const float *e_prev, uint32_t *hist,
                     float *e_cell, float *e_next)
{
    hipLaunchKernelGGL(mr::k_exposure, dim3(1), dim3(mr::TONE_BLOCK), 0, stream, slab, (int)rows, meter, e_prev, hist, e_cell, e_next);
}

// the frame in place; e_cell == nullptr: e_fixed
void launch_apply(hipStream_t stream, float *frame, size_t n_floats, int op, const float *e_cell, float e_fixed, float white2)
{
    const size_t want = std::max<size_t>(1, (n_floats / 4 + mr::TONE_BLOCK - 1) / mr::TONE_BLOCK);
    const dim3 grid((unsigned)std::min<size_t>(mr::TONE_APPLY_MAX_BLOCKS, want)), block(mr::TONE_BLOCK);
    if (op == mr::TONE_ACES) hipLaunchKernelGGL(mr::k_tone_apply<mr::TONE_ACES>, grid, block, 0, stream, frame, n_floats, e_cell, e_fixed, white2);
    else if (op == mr::TONE_REINHARD) hipLaunchKernelGGL(mr::k_tone_apply<mr::TONE_REINHARD>, grid, block, 0, stream, frame, n_floats, e_cell, e_fixed, white2);
    else hipLaunchKernelGGL(mr::k_tone_apply<mr::TONE_LINEAR>, grid, block, 0, stream, frame, n_floats, e_cell, e_fixed, white2);
}

}  // namespace mr_tonemap
