// motion_faces.hip -- the two kernels of the per-face velocity (kernels_motion_faces.h) and their launches, the library's
// sixth translation unit and a code object of its own, like accum.hip, ao.hip, dof.hip and motion.hip: the other code
// objects keep their kernels at the addresses they held them at before.  host_motion_faces.h calls the functions below; a
// library linked without this file refuses the pass (MR_E_UNSUPPORTED) and is otherwise whole.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels_motion_faces.h"

namespace mr_motion_faces {

void launch_homography(hipStream_t stream, const int32_t *faces, const double *verts, const double *verts_prev, const int32_t *tables,
                       double *hom, const mr::MotionFacesParams &p)
{
    if (p.n_records <= 0) return;
    const unsigned blocks = (unsigned)((p.n_records + mr::MOTION_FACES_BLOCK - 1) / mr::MOTION_FACES_BLOCK);
    hipLaunchKernelGGL(mr::k_face_homography, dim3(blocks), dim3(mr::MOTION_FACES_BLOCK), 0, stream, faces, verts, verts_prev, tables, hom, p);
}

void launch_velocity_faces(hipStream_t stream, const int32_t *winner, const int32_t *tables, const double *hom, float *vel, int width,
                           int height, int n_models)
{
    const size_t n = (size_t)width * height;
    const unsigned blocks = (unsigned)((n + mr::MOTION_FACES_BLOCK - 1) / mr::MOTION_FACES_BLOCK);
    hipLaunchKernelGGL(mr::k_velocity_faces, dim3(blocks), dim3(mr::MOTION_FACES_BLOCK), 0, stream, winner, tables, hom,
                       reinterpret_cast<float2 *>(vel), width, height, n_models);
}

}  // namespace mr_motion_faces
