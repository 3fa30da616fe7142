// motion_faces_def.h -- the velocity of the samples of models that bend (bones, morph weights): the definition, once, for
// the kernels (kernels_motion_faces.h) and for the host mirrors (host_motion_faces.h), which both include this file;
// tests/motion_faces_ref.py restates it in NumPy.  No kernel lives here: mi355rast.hip includes this header and its code
// object must not grow (kernels_accum.h says why).
//
// For one face let V_k be the corners' current world positions (d_verts after morph -> skin -> pose) and P_k their positions
// at the previous frame (the snapshot d_verts_prev).  Sn and Sp are the (x, y, w) columns of the current and the previous
// frame's S = view . projection . viewport on the sample grid, 4 x 3 each, row vectors, row-major.  float64, left to right,
// every operation rounded on its own (-ffp-contract=off):
//
//   X_k = ((V_k.x*Sn[0][0] + V_k.y*Sn[1][0]) + V_k.z*Sn[2][0]) + Sn[3][0]     likewise Y_k, W_k (columns 1, 2): c_k
//   q_k[c] = ((P_k.x*Sp[0][c] + P_k.y*Sp[1][c]) + P_k.z*Sp[2][c]) + Sp[3][c]
//   A[0] = Y x W,  A[1] = W x X,  A[2] = X x Y             each component  a*b - c*d   (X, Y, W: the vectors over k)
//   det  = (X_0*A[0][0] + X_1*A[0][1]) + X_2*A[0][2]
//   H[r][c] = (A[r][0]*q_0[c] + A[r][1]*q_1[c]) + A[r][2]*q_2[c]
//   s = max |H[r][c]|                                      (not a number as soon as one entry is none)
//   H = 0 (all nine) unless det and s are finite, det != 0 and s > 0;  else  H[r][c] = (det < 0 ? -H[r][c] : H[r][c]) / s
//
// (x, y, 1) . A are the un-normalised perspective-correct barycentrics of sample (x, y) on the face's plane -- A is the
// adjugate of [X Y W] -- so u = (x, y, 1) . H is det / w_now times the previous homogeneous screen position of the surface
// point the sample shows: the sign of det is folded into H, the scale s is positive, and the background branch of
// motion_velocity (motion_def.h) turns u into U: front = u_2 > 0, U = (x - u_0/u_2, y - u_1/u_2), one rounding to float32,
// (0, 0) unless both are finite.  H = 0 gives u_2 = 0, not in front, U = (0, 0): the answer for a degenerate face and for a
// vertex that is no number.  No z-buffer, no division per corner, no clipping: H belongs to the face's plane, and every
// sample the frame shows on it maps exactly, also on a face that straddles the camera plane.
#pragma once

#include "motion_def.h"

namespace mr {

constexpr int MOTION_H = 9;                  // doubles of a face's record: H, 3 x 3 row-major, one after the other (AoS)

// What k_face_homography takes by value: Sn, Sp (4 x 3 row-major) and the table's sizes.
struct MotionFacesParams {
    double s_now[12], s_prev[12];
    int32_t n_models, n_ranges, n_records;
};

// (v, 1) . S, S 4 x 3 row-major
MR_AO_HD inline void motion_faces_project(const double *v, const double *S, double *out)
{
    for (int c = 0; c < 3; ++c) out[c] = ((v[0] * S[c] + v[1] * S[3 + c]) + v[2] * S[6 + c]) + S[9 + c];
}

// H of one face; v0 .. v2 the current corners, p0 .. p2 the previous ones (x, y, z read)
MR_AO_HD inline void motion_face_homography(const double *v0, const double *v1, const double *v2, const double *p0, const double *p1,
                                            const double *p2, const double *Sn, const double *Sp, double *H)
{
    double c[3][3], q[3][3];
    motion_faces_project(v0, Sn, c[0]); motion_faces_project(v1, Sn, c[1]); motion_faces_project(v2, Sn, c[2]);
    motion_faces_project(p0, Sp, q[0]); motion_faces_project(p1, Sp, q[1]); motion_faces_project(p2, Sp, q[2]);
    const double X[3] = { c[0][0], c[1][0], c[2][0] }, Y[3] = { c[0][1], c[1][1], c[2][1] }, W[3] = { c[0][2], c[1][2], c[2][2] };
    const double *a[3] = { Y, W, X }, *b[3] = { W, X, Y };            // A[r] = a[r] x b[r]
    double A[3][3];
    for (int r = 0; r < 3; ++r) {
        A[r][0] = a[r][1] * b[r][2] - a[r][2] * b[r][1];
        A[r][1] = a[r][2] * b[r][0] - a[r][0] * b[r][2];
        A[r][2] = a[r][0] * b[r][1] - a[r][1] * b[r][0];
    }
    const double det = (X[0] * A[0][0] + X[1] * A[0][1]) + X[2] * A[0][2];
    double s = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            const double h = (A[r][0] * q[0][k] + A[r][1] * q[1][k]) + A[r][2] * q[2][k];
            const double m = __builtin_fabs(h);
            H[r * 3 + k] = h;
            if (m > s || m != m) s = m;                                // (once no number, s stays none)
        }
    const bool ok = __builtin_isfinite(det) && __builtin_isfinite(s) && det != 0.0 && s > 0.0;
    for (int i = 0; i < MOTION_H; ++i) H[i] = ok ? (det < 0.0 ? -H[i] : H[i]) / s : 0.0;
}

// U of one sample of a face with record H
MR_AO_HD inline void motion_faces_velocity(const double *H, int x, int y, float &ux, float &uy)
{
    motion_velocity(H, H, __builtin_inf(), x, y, ux, uy);             // (the background branch: u = (x, y, 1) . H)
}

}  // namespace mr
