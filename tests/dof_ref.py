"""The depth of field's definition (include/mi355rast.h) in NumPy: ao_ref's float64 eye depth,
float32 from there on, every operation an array operation of its own (NumPy fuses nothing), the 33 x 33 taps in an
explicit loop, dy ascending and dx ascending inside it.  The yardstick of ``mr_host_dof``, which in turn is the yardstick
of ``k_dof``."""
import numpy as np

import ao_ref

F32 = np.float32
MAX_RADIUS = 16


def circle(z, m, kf, perspective, focus):
    """The signed circle of confusion ``s`` (float32) of a float64 z-buffer; background: kf under perspective, +inf
    without."""
    e = ao_ref.eye_depth(z, m)                       # +inf where background
    kf, focus = F32(kf), F32(focus)
    with np.errstate(all="ignore"):
        if perspective:
            t = (focus / e).astype(F32)
            t = (F32(1) - t).astype(F32)
            return (kf * t).astype(F32)
        t = (e - focus).astype(F32)
        return (kf * t).astype(F32)


def squared_radius(s):
    """``rr = max(min(|s|, 16) ** 2, 0.25)``, float32."""
    a = np.abs(s).astype(F32)
    c = np.where(a < F32(MAX_RADIUS), a, F32(MAX_RADIUS)).astype(F32)
    rr = (c * c).astype(F32)
    return np.where(rr > F32(0.25), rr, F32(0.25)).astype(F32)


def apply_to_circle(s, frame):
    """F' (float32 (Hs, Ws, 3)) from the circles *s* and the float frame."""
    s = np.asarray(s, dtype=F32)
    frame = np.asarray(frame, dtype=F32)
    h, w = s.shape
    rr = squared_radius(s)
    W = np.zeros((h, w), dtype=F32)
    S = np.zeros((h, w, 3), dtype=F32)
    with np.errstate(all="ignore"):
        for dy in range(-MAX_RADIUS, MAX_RADIUS + 1):
            py = slice(max(0, -dy), min(h, h - dy))              # the rows of p whose tap's row lies inside the frame
            qy = slice(py.start + dy, py.stop + dy)
            if py.start >= py.stop:
                continue
            for dx in range(-MAX_RADIUS, MAX_RADIUS + 1):
                px = slice(max(0, -dx), min(w, w - dx))
                qx = slice(px.start + dx, px.stop + dx)
                if px.start >= px.stop:
                    continue
                s_p, s_q, rr_p, rr_q = s[py, px], s[qy, qx], rr[py, px], rr[qy, qx]
                behind = s_q > s_p
                rr_t = np.where(behind, np.where(rr_p < rr_q, rr_p, rr_q), rr_q).astype(F32)
                passes = F32(dx * dx + dy * dy) <= rr_t
                if not passes.any():
                    continue
                wt = (F32(1) / rr_t).astype(F32)
                W[py, px] = np.where(passes, (W[py, px] + wt).astype(F32), W[py, px])
                term = (wt[..., None] * frame[qy, qx]).astype(F32)
                S[py, px] = np.where(passes[..., None], (S[py, px] + term).astype(F32), S[py, px])
        return (S / W[..., None]).astype(F32)


def apply(z, frame, m, kf, perspective, focus):
    """F' of the z-buffer *z* (float64 (Hs, Ws)) and the float frame *frame*."""
    return apply_to_circle(circle(z, m, kf, perspective, focus), frame)
