// kernels_layers.h -- k_layers<POS32>: the per-sample data layers of a frame, right behind k_tile, from the winner map and
// the scene's static face records alone (layers_def.h has the definition).  It reads no z-buffer and never touches the
// float frame.
//
// One thread per sample, 256 to a workgroup.  A thread reads its winner, finds the model as k_velocity does, reads the
// face's FacePos record (64 or 112 bytes) and, for normal and uv, its FaceAttr record (64 bytes), and stores what the mask
// asks for.  The lanes of a wavefront show a few faces only, so the records' lines are fetched once and served from cache
// to the other lanes.  Every layer is a buffer of its own: consecutive lanes store consecutive samples, 4, 8 or 12 bytes
// each, so a wavefront's stores to one layer cover one contiguous stretch of 256, 512 or 768 bytes.  The mask is a kernel
// argument, the same for every lane: a layer that was not asked for costs neither its arithmetic nor its store.  The
// arithmetic is float64 (about 150 multiplies and adds, 3 divisions, and 2 square roots and 6 divisions more for the
// normals): with every layer on the kernel is bound by it rather than by its 76 bytes of stores a sample.
//
// Registers, from the compiler's listing (tests/test_layers_layout.py reads it again and holds both to the 64 of eight
// wavefronts a SIMD): k_layers<true>: 60 VGPRs, k_layers<false>: 62 VGPRs.
//
// No LDS, no scratch, no atomics, no memset.  Compiled in layers.hip, a code object of its own (kernels_accum.h says why).
#pragma once

#include "layers_def.h"

namespace mr {

constexpr int LAYERS_BLOCK = 256;

template <bool POS32>
__global__ void __launch_bounds__(LAYERS_BLOCK)
k_layers(const LayersArgs a, const LayersParams p)
{
    typedef FacePosT<typename std::conditional<POS32, float, double>::type> FacePos;
    const size_t i = (size_t)blockIdx.x * LAYERS_BLOCK + threadIdx.x;
    if (i >= (size_t)a.width * a.height) return;
    const int32_t mask = p.mask;
    int32_t w = a.winner[i];
    if (w >= p.n_faces) w = -1;                                           // (no such face: never from k_tile)
    int32_t model = -1, face = -1, material = -1;
    LayerSample o;
    layers_background(o);
    if (w >= 0) {
        model = motion_model_of(a.face_off, p.n_models, w);
        face = w - a.face_off[model];
        const FacePos &fp = static_cast<const FacePos *>(a.face_pos)[w];
        material = fp.material;
        if (mask & ~LAYER_IDS) {
            const int y = (int)(i / (size_t)a.width), x = (int)(i - (size_t)y * a.width);
            layers_sample(fp, a.face_attr[w], p.s, mask, x, y, o);
        }
    }
    if (mask & (1 << LAYER_MODEL)) static_cast<int32_t *>(a.out[LAYER_MODEL])[i] = model;
    if (mask & (1 << LAYER_FACE)) static_cast<int32_t *>(a.out[LAYER_FACE])[i] = face;
    if (mask & (1 << LAYER_MATERIAL)) static_cast<int32_t *>(a.out[LAYER_MATERIAL])[i] = material;
    if (mask & (1 << LAYER_DEPTH)) static_cast<float *>(a.out[LAYER_DEPTH])[i] = o.depth;
    auto store3 = [&](int layer, const float *v) {
        float *dst = static_cast<float *>(a.out[layer]) + i * 3;
        dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2];
    };
    if (mask & (1 << LAYER_BARYCENTRIC)) store3(LAYER_BARYCENTRIC, o.bary);
    if (mask & (1 << LAYER_POSITION)) store3(LAYER_POSITION, o.position);
    if (mask & (1 << LAYER_FACE_NORMAL)) store3(LAYER_FACE_NORMAL, o.face_normal);
    if (mask & (1 << LAYER_NORMAL)) store3(LAYER_NORMAL, o.normal);
    if (mask & (1 << LAYER_UV)) static_cast<float2 *>(a.out[LAYER_UV])[i] = make_float2(o.uv[0], o.uv[1]);
}

}  // namespace mr
