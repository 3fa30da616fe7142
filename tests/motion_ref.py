"""The motion blur's definition (include/mi355rast.h, csrc/motion_def.h) in NumPy: the velocity in
float64 with one rounding to float32, the blur in float32, every operation an array operation of its own (NumPy fuses
nothing), the 33 x 33 taps in an explicit loop, dy ascending and dx ascending inside it.  The yardstick of
``mr_host_velocity`` and ``mr_host_motion_blur``, which in turn are the yardsticks of ``k_velocity`` and ``k_mblur``."""
import numpy as np

import ao_ref

F32 = np.float32
F64 = np.float64
MAX_HALF = 16
FLT_MAX = np.finfo(np.float32).max


def model_of(face_off, winner):
    """The model of every face index of *winner* (>= 0): the last m with ``face_off[m] <= w``."""
    face_off = np.asarray(face_off, dtype=np.int64)
    return np.searchsorted(face_off, np.asarray(winner, dtype=np.int64), side="right") - 1


def velocity(z, winner, face_off, matrices, background, class_of_model):
    """U, float32 ``(Hs, Ws, 2)``: *matrices* ``(n_classes, 4, 3)`` and *background* ``(3, 3)`` float64."""
    z = np.asarray(z, dtype=F64)
    winner = np.asarray(winner, dtype=np.int32)
    T = np.asarray(matrices, dtype=F64).reshape(-1, 4, 3)
    B = np.asarray(background, dtype=F64).reshape(3, 3)
    class_of_model = np.asarray(class_of_model, dtype=np.int64)
    h, w = z.shape
    cls = np.zeros((h, w), dtype=np.int64)
    covered = winner >= 0
    if len(class_of_model) and covered.any():
        cls[covered] = class_of_model[model_of(face_off, winner[covered])]
    ys, xs = np.mgrid[0:h, 0:w]
    x, y = xs.astype(F64), ys.astype(F64)
    finite = np.isfinite(z)
    t = T[cls]                                           # (h, w, 4, 3)
    with np.errstate(all="ignore"):
        xz, yz = x * z, y * z
        u = []
        for c in range(3):
            a = xz * t[..., 0, c]
            a = a + yz * t[..., 1, c]
            a = a + z * t[..., 2, c]
            a = a + t[..., 3, c]
            b = x * B[0, c]
            b = b + y * B[1, c]
            b = b + B[2, c]
            u.append(np.where(finite, a, b))
        front = np.where(finite, u[2] * z, u[2]) > 0
        ux = (x - u[0] / u[2]).astype(F32)
        uy = (y - u[1] / u[2]).astype(F32)
    ok = front & np.isfinite(ux) & np.isfinite(uy)
    return np.stack([np.where(ok, ux, F32(0)), np.where(ok, uy, F32(0))], axis=-1).astype(F32)


def segment(vel, shutter):
    """(h, d_x, d_y, inv), float32, of the velocity buffer."""
    vel = np.asarray(vel, dtype=F32)
    s = F32(shutter)
    with np.errstate(all="ignore"):
        vx, vy = (s * vel[..., 0]).astype(F32), (s * vel[..., 1]).astype(F32)
        L = np.sqrt(((vx * vx).astype(F32) + (vy * vy).astype(F32)).astype(F32)).astype(F32)
        moving = (L >= F32(0.5)) & (L <= FLT_MAX)
        half = (L * F32(0.5)).astype(F32)
        h = np.where(moving, np.where(half < F32(MAX_HALF), half, F32(MAX_HALF)), F32(0)).astype(F32)
        dx = np.where(moving, (vx / L).astype(F32), F32(1)).astype(F32)
        dy = np.where(moving, (vy / L).astype(F32), F32(0)).astype(F32)
        inv = (F32(1) / ((F32(2) * h).astype(F32) + F32(1)).astype(F32)).astype(F32)
    return h, dx, dy, inv


def blur(z, vel, frame, m, shutter):
    """F' (float32 (Hs, Ws, 3)) of the z-buffer, the velocity buffer and the float frame."""
    e = ao_ref.eye_depth(z, m)                           # +inf where background
    frame = np.asarray(frame, dtype=F32)
    hh, ww = e.shape
    h, dx_, dy_, inv = segment(vel, shutter)
    W = np.zeros((hh, ww), dtype=F32)
    S = np.zeros((hh, ww, 3), dtype=F32)
    with np.errstate(all="ignore"):
        for dy in range(-MAX_HALF, MAX_HALF + 1):
            py = slice(max(0, -dy), min(hh, hh - dy))            # the rows of p whose tap's row lies inside the frame
            qy = slice(py.start + dy, py.stop + dy)
            if py.start >= py.stop:
                continue
            for dx in range(-MAX_HALF, MAX_HALF + 1):
                px = slice(max(0, -dx), min(ww, ww - dx))
                qx = slice(px.start + dx, px.stop + dx)
                if px.start >= px.stop:
                    continue
                ox, oy = F32(-dx), F32(-dy)
                dqx, dqy = dx_[qy, qx], dy_[qy, qx]
                along = ((ox * dqx).astype(F32) + (oy * dqy).astype(F32)).astype(F32)
                perp = ((ox * dqy).astype(F32) - (oy * dqx).astype(F32)).astype(F32)
                own = (e[qy, qx] > e[py, px]) & (h[py, px] < h[qy, qx])
                h_t = np.where(own, h[py, px], h[qy, qx]).astype(F32)
                passes = (np.abs(along) <= (h_t + F32(0.5)).astype(F32)) & (np.abs(perp) <= F32(0.5))
                if not passes.any():
                    continue
                wt = (F32(1) / ((F32(2) * h_t).astype(F32) + F32(1)).astype(F32)).astype(F32)
                W[py, px] = np.where(passes, (W[py, px] + wt).astype(F32), W[py, px])
                term = (wt[..., None] * frame[qy, qx]).astype(F32)
                S[py, px] = np.where(passes[..., None], (S[py, px] + term).astype(F32), S[py, px])
        return (S / W[..., None]).astype(F32)


def apply(z, winner, frame, face_off, m, shutter, matrices, background, class_of_model):
    """(U, F') of one frame."""
    u = velocity(z, winner, face_off, matrices, background, class_of_model)
    return u, blur(z, u, frame, m, shutter)
