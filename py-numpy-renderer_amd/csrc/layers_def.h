// layers_def.h -- per-sample data layers (ids, barycentrics, depth, position, normals, uv) from the winner map and the
// static face records: the definition, once, for the kernel (kernels_layers.h) and for the host mirror (host_layers.h),
// which both include this file; tests/layers_ref.py restates it in NumPy.  No kernel lives here: mi355rast.hip includes
// this header and its code object must not grow (kernels_accum.h says why).
//
// On the sample grid (Hs, Ws), rows bottom-up, at integer screen coordinates (x, y), with w the winner map
// (mr_read_winner), V_k the three corners of face w as its record holds them (FacePos32 / FacePos64; x, y, z read, the
// fourth coordinate taken as 1), n_k and uv_k the corners' float32 normals and texture coordinates (FaceAttr), and S the
// 4 x 4 matrix of the description (row vectors, row-major): its columns 0, 1, 2 are x, y, w of view . projection .
// viewport on the sample grid AS RENDERED (the sub-sample offset of a temporal anti-aliasing included), column 3 maps a
// world point to its eye depth e, > 0 in front of the camera.  float64, left to right, every operation rounded on its own
// (-ffp-contract=off), IEEE divisions and square roots, one rounding to float32 at the end:
//
//   model    = the last m with face_off[m] <= w (motion_model_of);   face = w - face_off[model];   material = the record's
//   c_k[j]   = ((V_k.x*S[0][j] + V_k.y*S[1][j]) + V_k.z*S[2][j]) + S[3][j]      j = 0 .. 3:  X_k, Y_k, W_k, E_k
//   A[0] = Y x W,  A[1] = W x X,  A[2] = X x Y        each component  a*b - c*d   (X, Y, W: the vectors over k), exactly
//                                                     as in motion_face_homography: A is the adjugate of [X Y W]
//   b_k      = (x*A[0][k] + y*A[1][k]) + A[2][k]
//   sigma    = (b_0 + b_1) + b_2;     lambda_k = b_k / sigma
//   degenerate: sigma or a lambda_k is not finite, or sigma == 0
//   barycentric = (lambda_0, lambda_1, lambda_2)
//   depth       = (lambda_0*E_0 + lambda_1*E_1) + lambda_2*E_2
//   position[j] = (lambda_0*V_0[j] + lambda_1*V_1[j]) + lambda_2*V_2[j]
//   g = (V_1 - V_0) x (V_2 - V_0)   (each component a*b - c*d);   l = sqrt((g.x*g.x + g.y*g.y) + g.z*g.z)
//   face_normal = g / l      where l is finite and > 0, else (0, 0, 0)
//   m[j] = (lambda_0*n_0[j] + lambda_1*n_1[j]) + lambda_2*n_2[j];   q = sqrt((m.x*m.x + m.y*m.y) + m.z*m.z)
//   normal      = m / q      where FF_HAS_NORMALS is set and q is finite and > 0, else face_normal
//   uv[j]       = (lambda_0*uv_0[j] + lambda_1*uv_1[j]) + lambda_2*uv_2[j]      where FF_HAS_UV is set, else 0
//
// A sample with w < 0 takes the background fill: ids -1, depth +inf, every other float 0.  A degenerate sample keeps its
// ids and takes the background fill in every other layer.  (x, y, 1) . A are the un-normalised perspective-correct
// barycentrics of the sample on the face's plane, so every layer is exact on that plane, also on a face that straddles the
// camera plane: no TriRec, no float32 tri_bary, no z-buffer.
//
// ERROR AGAINST EXACT ARITHMETIC (what tests/test_layers_cpu.py holds the mirror to on faces whose coordinates are not
// dyadic).  u = 2^-53.  For an expression evaluated as above write bar(.) for the same expression over the absolute values
// of its terms.  Counting roundings along the longest chain: c_k 4 (given exact V and S), a component of A 4 + 4 + 2 = 10,
// b_k 13, sigma 15.  With gamma_n = n u / (1 - n u) <= 1.01 n u here:
//   |fl(b_k) - b_k| <= gamma_13 bar(b_k),   |fl(sigma) - sigma| <= gamma_15 bar(sigma),   bar(sigma) = sum bar(b_k)
// and for the quotient, while 16 u bar(sigma) / |sigma| <= 1/2 (so that 1 / (1 - delta) <= 2 for the denominator),
//   |fl(lambda_k) - lambda_k| <= E_k = 32 u kappa_k,   kappa_k = (bar(b_k) + |lambda_k| bar(sigma)) / |sigma|
// kappa_k is the face's conditioning at the sample: 1 to 3 on a face seen square on, large on a sliver or near the
// camera plane.  A sum t = (lambda_0 a_0 + lambda_1 a_1) + lambda_2 a_2 with terms a_k known to within d_k has
//   |fl(t) - t| <= sum (E_k |a_k| + |lambda_k| d_k) + 4 u sum (|lambda_k| + E_k)(|a_k| + d_k)
// with d_k = gamma_4 bar(E_k) for the depth and d_k = 0 for position and uv; the rounding to float32 adds 2^-24 |t|
// (2^-149 where the float is subnormal).  A sample whose 16 u bar(sigma) / |sigma| exceeds 1/2 has no bound.
#pragma once

#include <cmath>

#include "motion_def.h"
#include "rast_types.h"

namespace mr {

// the layers, as bits of a mask and as indices of mr_read_layers
enum : int32_t { LAYER_MODEL = 0, LAYER_FACE, LAYER_MATERIAL, LAYER_BARYCENTRIC, LAYER_DEPTH, LAYER_POSITION, LAYER_FACE_NORMAL,
                 LAYER_NORMAL, LAYER_UV, N_LAYERS };
constexpr int32_t LAYER_ALL = (1 << N_LAYERS) - 1;
constexpr int32_t LAYER_IDS = (1 << LAYER_MODEL) | (1 << LAYER_FACE) | (1 << LAYER_MATERIAL);

// 32-bit words a sample has in layer i
MR_AO_HD inline int layer_words(int i)
{
    return i <= LAYER_MATERIAL || i == LAYER_DEPTH ? 1 : i == LAYER_UV ? 2 : 3;
}

// What k_layers takes by value beside its pointers.
struct LayersParams {
    double s[16];                // S, row-major
    int32_t mask, n_models, n_faces, pad;
};

// The kernel's pointers: out[i] is layer i's buffer (read only where the mask names it).
struct LayersArgs {
    const int32_t *winner;
    const void *face_pos;        // FacePos32[] or FacePos64[]
    const FaceAttr *face_attr;
    const int32_t *face_off;
    void *out[N_LAYERS];
    int32_t width, height;
};

// What one sample has in every layer; the ids are the caller's.
struct LayerSample {
    float bary[3], depth, position[3], face_normal[3], normal[3], uv[2];
    bool degenerate;
};

MR_AO_HD inline void layers_background(LayerSample &o)
{
    for (int j = 0; j < 3; ++j) o.bary[j] = o.position[j] = o.face_normal[j] = o.normal[j] = 0.0f;
    o.uv[0] = o.uv[1] = 0.0f;
    o.depth = __builtin_inff();
    o.degenerate = false;
}

// The float layers of sample (x, y) of a face; `mask` names the layers somebody reads (the others' fields are unspecified).
template <class T>
MR_AO_HD inline void layers_sample(const FacePosT<T> &fp, const FaceAttr &fa, const double *S, int32_t mask, int x, int y, LayerSample &o)
{
    layers_background(o);
    double V[3][3], c[3][4];
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) V[k][j] = (double)fp.v[k][j];
        for (int j = 0; j < 4; ++j) c[k][j] = ((V[k][0] * S[j] + V[k][1] * S[4 + j]) + V[k][2] * S[8 + j]) + S[12 + j];
    }
    const double X[3] = { c[0][0], c[1][0], c[2][0] }, Y[3] = { c[0][1], c[1][1], c[2][1] }, W[3] = { c[0][2], c[1][2], c[2][2] };
    const double *a[3] = { Y, W, X }, *b[3] = { W, X, Y };            // A[r] = a[r] x b[r]
    double A[3][3];
    for (int r = 0; r < 3; ++r) {
        A[r][0] = a[r][1] * b[r][2] - a[r][2] * b[r][1];
        A[r][1] = a[r][2] * b[r][0] - a[r][0] * b[r][2];
        A[r][2] = a[r][0] * b[r][1] - a[r][1] * b[r][0];
    }
    const double xd = (double)x, yd = (double)y;
    double bk[3], lam[3];
    for (int k = 0; k < 3; ++k) bk[k] = (xd * A[0][k] + yd * A[1][k]) + A[2][k];
    const double sigma = (bk[0] + bk[1]) + bk[2];
    for (int k = 0; k < 3; ++k) lam[k] = bk[k] / sigma;
    if (!(__builtin_isfinite(sigma) && sigma != 0.0 && __builtin_isfinite(lam[0]) && __builtin_isfinite(lam[1]) && __builtin_isfinite(lam[2]))) {
        o.degenerate = true;
        return;
    }
    for (int k = 0; k < 3; ++k) o.bary[k] = (float)lam[k];
    o.depth = (float)((lam[0] * c[0][3] + lam[1] * c[1][3]) + lam[2] * c[2][3]);
    for (int j = 0; j < 3; ++j) o.position[j] = (float)((lam[0] * V[0][j] + lam[1] * V[1][j]) + lam[2] * V[2][j]);
    if (mask & ((1 << LAYER_FACE_NORMAL) | (1 << LAYER_NORMAL))) {
        const double p[3] = { V[1][0] - V[0][0], V[1][1] - V[0][1], V[1][2] - V[0][2] };
        const double q[3] = { V[2][0] - V[0][0], V[2][1] - V[0][1], V[2][2] - V[0][2] };
        const double g[3] = { p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0] };
        const double l = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        if (__builtin_isfinite(l) && l > 0.0)
            for (int j = 0; j < 3; ++j) o.face_normal[j] = (float)(g[j] / l);
        for (int j = 0; j < 3; ++j) o.normal[j] = o.face_normal[j];
        if ((mask & (1 << LAYER_NORMAL)) && (fp.flags & FF_HAS_NORMALS)) {
            double m[3];
            for (int j = 0; j < 3; ++j) m[j] = (lam[0] * (double)fa.n[0][j] + lam[1] * (double)fa.n[1][j]) + lam[2] * (double)fa.n[2][j];
            const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            if (__builtin_isfinite(len) && len > 0.0)
                for (int j = 0; j < 3; ++j) o.normal[j] = (float)(m[j] / len);
        }
    }
    if ((mask & (1 << LAYER_UV)) && (fp.flags & FF_HAS_UV))
        for (int j = 0; j < 2; ++j) o.uv[j] = (float)((lam[0] * (double)fa.uv[0][j] + lam[1] * (double)fa.uv[1][j]) + lam[2] * (double)fa.uv[2][j]);
}

}  // namespace mr
