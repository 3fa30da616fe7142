"""The per-face velocity's definition (include/mi355rast.h, csrc/motion_faces_def.h) in NumPy: float64,
every operation an array operation of its own (NumPy fuses nothing), left to right as pinned, one rounding to float32 at
the end.  The yardstick of ``mr_host_face_homographies`` and ``mr_host_velocity_faces``, which in turn are the yardsticks
of ``k_face_homography`` and ``k_velocity_faces``.  ``exact_*`` is the same mathematics over ``fractions.Fraction`` --
every float64 input is a rational, so the answer has no rounding at all -- for the known answers and the accuracy bound."""
from fractions import Fraction

import numpy as np

import motion_ref

F32 = np.float32
F64 = np.float64


def project(v, S):
    """``(v, 1) . S`` for vertices ``(n, >= 3)`` and S ``(4, 3)``: ``((x S0 + y S1) + z S2) + S3`` per column, ``(n, 3)``."""
    v = np.asarray(v, dtype=F64)
    S = np.asarray(S, dtype=F64).reshape(4, 3)
    with np.errstate(all="ignore"):
        cols = []
        for c in range(3):
            a = v[:, 0] * S[0, c]
            a = a + v[:, 1] * S[1, c]
            a = a + v[:, 2] * S[2, c]
            cols.append(a + S[3, c])
    return np.stack(cols, axis=1)


def _cross(a, b):
    """Rows of ``a x b`` for ``(n, 3)`` arrays, each component ``a*b - c*d``."""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                    axis=1)


def homographies(verts_now, verts_prev, corners, s_now, s_prev):
    """H, float64 ``(n_faces, 3, 3)``, of faces given by their ``(n_faces, 3)`` vertex indices."""
    corners = np.asarray(corners, dtype=np.int64).reshape(-1, 3)
    now, prev = project(verts_now, s_now), project(verts_prev, s_prev)
    c = now[corners]                                     # (n, corner k, component x / y / w)
    q = prev[corners]                                    # (n, corner k, c)
    X, Y, W = c[:, :, 0], c[:, :, 1], c[:, :, 2]         # (n, k) each
    with np.errstate(all="ignore"):
        A = np.stack([_cross(Y, W), _cross(W, X), _cross(X, Y)], axis=1)        # (n, r, k)
        det = X[:, 0] * A[:, 0, 0] + X[:, 1] * A[:, 0, 1]
        det = det + X[:, 2] * A[:, 0, 2]
        H = np.empty((len(corners), 3, 3), dtype=F64)
        for r in range(3):
            for col in range(3):
                h = A[:, r, 0] * q[:, 0, col] + A[:, r, 1] * q[:, 1, col]
                H[:, r, col] = h + A[:, r, 2] * q[:, 2, col]
        s = np.abs(H).reshape(len(corners), 9).max(axis=1) if len(corners) else np.zeros(0)      # (NaN propagates)
        ok = np.isfinite(det) & np.isfinite(s) & (det != 0) & (s > 0)
        signed = np.where((det < 0)[:, None, None], -H, H) / s[:, None, None]
    return np.where(ok[:, None, None], signed, 0.0)


def velocity_faces(winner, face_off, hom_off, H, velocity):
    """A copy of *velocity* ``(Hs, Ws, 2)`` float32 in which the samples of the flagged models (``hom_off >= 0``) hold the U
    of their face's record; every other float keeps its bits."""
    winner = np.asarray(winner, dtype=np.int32)
    out = np.array(velocity, dtype=F32)
    hom_off = np.asarray(hom_off, dtype=np.int64)
    face_off = np.asarray(face_off, dtype=np.int64)
    H = np.asarray(H, dtype=F64).reshape(-1, 3, 3)
    covered = winner >= 0
    if not covered.any():
        return out
    model = np.zeros(winner.shape, dtype=np.int64)
    model[covered] = motion_ref.model_of(face_off, winner[covered])
    take = covered & (hom_off[model] >= 0)
    if not take.any():
        return out
    ys, xs = np.nonzero(take)
    h = H[hom_off[model[take]] + (winner[take].astype(np.int64) - face_off[model[take]])]
    x, y = xs.astype(F64), ys.astype(F64)
    with np.errstate(all="ignore"):
        u = []
        for c in range(3):
            b = x * h[:, 0, c]
            b = b + y * h[:, 1, c]
            u.append(b + h[:, 2, c])
        front = u[2] > 0
        ux = (x - u[0] / u[2]).astype(F32)
        uy = (y - u[1] / u[2]).astype(F32)
    ok = front & np.isfinite(ux) & np.isfinite(uy)
    out[ys, xs, 0] = np.where(ok, ux, F32(0))
    out[ys, xs, 1] = np.where(ok, uy, F32(0))
    return out


# ---------------------------------------------------------------------------- exact arithmetic
def _frac_project(v, S):
    S = [[Fraction(float(S[r][c])) for c in range(3)] for r in range(4)]
    x, y, z = (Fraction(float(t)) for t in v[:3])
    return [x * S[0][c] + y * S[1][c] + z * S[2][c] + S[3][c] for c in range(3)]


def exact_previous_position(v, p, s_now, s_prev, x, y):
    """Where the surface point that sample (x, y) shows on the face with current corners *v* (3 vertices) and previous
    corners *p* was on the previous frame's sample grid, exactly: ``(x_prev, y_prev, in_front)`` as Fractions and a bool,
    or ``None`` for a face that has no area on the screen."""
    c = [_frac_project(v[k], s_now) for k in range(3)]
    q = [_frac_project(p[k], s_prev) for k in range(3)]
    X, Y, W = ([c[k][i] for k in range(3)] for i in range(3))
    x, y = Fraction(x), Fraction(y)
    a = [X[k] - x * W[k] for k in range(3)]
    b = [Y[k] - y * W[k] for k in range(3)]
    lam = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    det = sum(lam[k] * W[k] for k in range(3))
    if det == 0:
        return None
    u = [sum(lam[k] * q[k][i] for k in range(3)) / det for i in range(3)]      # 1 / w_now times the previous position
    if u[2] == 0:
        return None
    return u[0] / u[2], u[1] / u[2], u[2] > 0


def exact_velocity(v, p, s_now, s_prev, x, y):
    """The exact U of sample (x, y), as two floats (the Fractions rounded once), or ``None``."""
    at = exact_previous_position(v, p, s_now, s_prev, x, y)
    if at is None or not at[2]:
        return None
    return float(Fraction(x) - at[0]), float(Fraction(y) - at[1])
