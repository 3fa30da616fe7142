// layers.hip -- the kernel of the per-sample data layers (kernels_layers.h) and its launch, the library's eleventh
// translation unit and a code object of its own, like accum.hip, ao.hip, dof.hip, motion.hip and the others: the other
// code objects keep their kernels at the addresses they held them at before.  host_layers.h calls the function below; a
// library linked without this file refuses the pass (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "kernels_layers.h"

namespace mr_layers {

void launch(hipStream_t stream, const mr::LayersArgs &a, const mr::LayersParams &p, int pos32)
{
    const size_t n = (size_t)a.width * a.height;
    if (n == 0 || !(p.mask & mr::LAYER_ALL)) return;
    const unsigned blocks = (unsigned)((n + mr::LAYERS_BLOCK - 1) / mr::LAYERS_BLOCK);
    if (pos32) hipLaunchKernelGGL(mr::k_layers<true>, dim3(blocks), dim3(mr::LAYERS_BLOCK), 0, stream, a, p);
    else hipLaunchKernelGGL(mr::k_layers<false>, dim3(blocks), dim3(mr::LAYERS_BLOCK), 0, stream, a, p);
}

}  // namespace mr_layers
