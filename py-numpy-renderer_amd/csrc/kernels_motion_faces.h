// kernels_motion_faces.h -- k_face_homography and k_velocity_faces: the velocity of the samples of models that bend, from
// the previous frame's deformed vertices per winner face (motion_faces_def.h has the definition).
//
// k_face_homography: one thread per face of the flagged models.  The flagged models' faces are numbered one model after
// the other ("records"); a thread finds its range by a binary search over the ranges' first records (a handful), reads the
// face's three vertex indices (d_faces: 12 int32 a face, corners at 0, 4, 8), six vertices of 4 doubles and writes nine
// doubles.  The records are AoS, 72 bytes one after the other: k_velocity_faces reads all nine of one record per sample,
// and the samples of a wavefront show a few faces only -- one or two 128-byte lines a face, where nine planes would cost
// nine; the strided writes here are per face, a thousandth of the samples.
//
// k_velocity_faces: one thread per sample, behind k_velocity.  It reads the winner, finds the model as k_velocity does and,
// where the model is flagged (hom_off >= 0), overwrites U from the face's record.  Every other sample is not written.
//
// tables (int32): hom_off[n_models], face_off[n_models], range_rec0[n_ranges], range_face0[n_ranges].
// No scratch, no memset, no atomics.  Compiled in motion_faces.hip, a code object of its own (kernels_accum.h says why).
#pragma once

#include "motion_faces_def.h"

namespace mr {

constexpr int MOTION_FACES_BLOCK = 256;

__global__ void __launch_bounds__(MOTION_FACES_BLOCK)
k_face_homography(const int32_t *__restrict__ faces, const double *__restrict__ verts, const double *__restrict__ verts_prev,
                  const int32_t *__restrict__ tables, double *__restrict__ hom, const MotionFacesParams p)
{
    const int i = (int)(blockIdx.x * MOTION_FACES_BLOCK + threadIdx.x);
    if (i >= p.n_records) return;
    const int32_t *rec0 = tables + 2 * p.n_models, *face0 = rec0 + p.n_ranges;
    const int r = motion_model_of(rec0, p.n_ranges, i);
    const int32_t *f = faces + (size_t)(face0[r] + (i - rec0[r])) * 12;
    const size_t a = (size_t)f[0] * 4, b = (size_t)f[4] * 4, c = (size_t)f[8] * 4;
    double H[MOTION_H];
    motion_face_homography(verts + a, verts + b, verts + c, verts_prev + a, verts_prev + b, verts_prev + c, p.s_now, p.s_prev, H);
    double *out = hom + (size_t)i * MOTION_H;
#pragma unroll
    for (int k = 0; k < MOTION_H; ++k) out[k] = H[k];
}

__global__ void __launch_bounds__(MOTION_FACES_BLOCK)
k_velocity_faces(const int32_t *__restrict__ winner, const int32_t *__restrict__ tables, const double *__restrict__ hom,
                 float2 *__restrict__ vel, int width, int height, int n_models)
{
    const size_t i = (size_t)blockIdx.x * MOTION_FACES_BLOCK + threadIdx.x;
    if (i >= (size_t)width * height) return;
    const int32_t w = winner[i];
    if (w < 0) return;
    const int32_t *hom_off = tables, *face_off = tables + n_models;
    const int m = motion_model_of(face_off, n_models, w);
    const int32_t h0 = hom_off[m];
    if (h0 < 0) return;
    const int y = (int)(i / (size_t)width), x = (int)(i - (size_t)y * width);
    const double *src = hom + (size_t)(h0 + (w - face_off[m])) * MOTION_H;
    double H[MOTION_H];
#pragma unroll
    for (int k = 0; k < MOTION_H; ++k) H[k] = src[k];
    float ux, uy;
    motion_faces_velocity(H, x, y, ux, uy);
    vel[i] = make_float2(ux, uy);
}

}  // namespace mr
