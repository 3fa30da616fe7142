"""The temporal anti-aliasing's definition (include/mi355rast.h, csrc/taa_def.h) in NumPy: float32
arrays throughout, so every operation is rounded on its own as in the kernel and the host mirror; and the jitter's
sequence (``_pack.taa_jitter``) restated.

``apply`` also builds the named MUTANTS of the definition -- each a plausible slip of an implementation -- so that the
tests can show that the synthetic cases tell them apart."""
import numpy as np

F32 = np.float32

MUTANTS = ("x1_unclamped", "neighbourhood_wrapped", "clamp_order_swapped", "lerp_weights", "round_nearest", "u_added", "no_corners")


def halton(i, base):
    """The radical inverse of *i* in *base*, float64, digit by digit from the lowest."""
    f, r = 1.0, 0.0
    while i > 0:
        f /= base
        r += f * (i % base)
        i //= base
    return r


def jitter(k, n):
    """``_pack.taa_jitter`` restated."""
    if n == 0 or k % n == 0:
        return 0.0, 0.0
    return halton(k % n, 2) - 0.5, halton(k % n, 3) - 0.5


def neighbourhood(frame, wrapped=False, corners=True):
    """(mn, mx) of *frame* over the 3 x 3 samples round every sample: coordinates clamped to the frame, rows then columns
    ascending, fminf / fmaxf from the first of them.  *wrapped*, *corners*: the mutants."""
    h, w = frame.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    mn = mx = None
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if not corners and dx and dy:
                continue
            if wrapped:
                v = frame[(ys + dy) % h, (xs + dx) % w]
            else:
                v = frame[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]
            mn = v if mn is None else np.fmin(mn, v)
            mx = v if mx is None else np.fmax(mx, v)
    return mn, mx


def apply(frame, velocity, history, blend, mutant=None, detail=False):
    """F' (which is also the new history P') of the definition; ``history`` None: no history.  With *detail* also the
    boolean maps (fetched, clamped from below, clamped from above) per float."""
    assert mutant is None or mutant in MUTANTS, mutant
    frame = np.ascontiguousarray(frame, dtype=F32)
    out = frame.copy()
    h, w = frame.shape[:2]
    none = np.zeros(frame.shape, dtype=bool)
    if history is None:
        return (out, none, none, none) if detail else out
    u = np.ascontiguousarray(velocity, dtype=F32)
    p = np.ascontiguousarray(history, dtype=F32)
    a = F32(blend)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        if mutant == "u_added":
            rx, ry = xs.astype(F32) + u[..., 0], ys.astype(F32) + u[..., 1]
        else:
            rx, ry = xs.astype(F32) - u[..., 0], ys.astype(F32) - u[..., 1]
        ok = (rx >= 0) & (rx <= F32(w - 1)) & (ry >= 0) & (ry <= F32(h - 1))
        rx, ry = np.where(ok, rx, F32(0)), np.where(ok, ry, F32(0))
        whole = np.rint if mutant == "round_nearest" else np.floor
        x0, y0 = whole(rx).astype(np.int64), whole(ry).astype(np.int64)
        fx, fy = (rx - x0.astype(F32))[..., None], (ry - y0.astype(F32))[..., None]
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        flat = p.reshape(-1, 3)

        def tap(row, col, col_unclamped):
            # (the unclamped mutant reads the next texel in memory: the first of the next row; past the end, the last)
            if mutant == "x1_unclamped" and col_unclamped:
                return flat[np.minimum(row * w + (x0 + 1), h * w - 1)]
            return p[row, col]

        def lerp(lo, hi, f):
            if mutant == "lerp_weights":
                return (F32(1) - f) * lo + f * hi
            return lo + f * (hi - lo)

        t0 = lerp(tap(y0, x0, False), tap(y0, x1, True), fx)
        t1 = lerp(tap(y1, x0, False), tap(y1, x1, True), fx)
        fetched = lerp(t0, t1, fy)
        mn, mx = neighbourhood(frame, wrapped=mutant == "neighbourhood_wrapped", corners=mutant != "no_corners")
        if mutant == "clamp_order_swapped":
            hk = np.fmax(np.fmin(fetched, mx), mn)
        else:
            hk = np.fmin(np.fmax(fetched, mn), mx)
        blended = hk + a * (frame - hk)
        below, above = ~(fetched >= mn), fetched > mx
    use = np.broadcast_to(ok[..., None], frame.shape)
    out = np.where(use, blended, frame).astype(F32)
    return (out, use, use & below, use & above) if detail else out
