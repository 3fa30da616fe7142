"""The ambient obscurance's definition (include/mi355rast.h) in NumPy: float64 for the eye depth,
float32 from there on, every operation an array operation of its own (NumPy fuses nothing), the eight pairs in an
explicit loop.  The yardstick of ``mr_host_ao``, which in turn is the yardstick of ``k_ao``."""
import numpy as np

F32 = np.float32
# u_i = (cos(i pi / 8), sin(i pi / 8)) * (1 for even i, 0.5 for odd i), the float32 literals of csrc/ao_def.h
TAPS = np.array([[1.0, 0.0], [0.46193977, 0.19134172], [0.70710678, 0.70710678], [0.19134172, 0.46193977],
                 [0.0, 1.0], [-0.19134172, 0.46193977], [-0.70710678, 0.70710678], [-0.46193977, 0.19134172]], dtype=F32)
MAX_RADIUS = 32


def params(radius=0.1, strength=1.0, depth_range=None, bias=None):
    """The defaults of ``AmbientOcclusion``: ``depth_range = 3 * radius``, ``bias = depth_range / 32``."""
    depth_range = 3.0 * radius if depth_range is None else depth_range
    bias = depth_range / 32.0 if bias is None else bias
    return dict(radius=float(radius), strength=float(strength), depth_range=float(depth_range), bias=float(bias))


def eye_depth(z, m):
    """float32 eye depth of a float64 z-buffer; +inf where the sample is background (Z or e not finite)."""
    z = np.asarray(z, dtype=np.float64)
    m0, m1, m2, m3 = (np.float64(x) for x in m)
    with np.errstate(all="ignore"):
        num = m0 * z
        num = num + m1
        den = m2 * z
        den = den + m3
        e = (num / den).astype(F32)
    return np.where(np.isfinite(z) & np.isfinite(e), e, F32(np.inf)).astype(F32)


def factor_from_depth(e, k, perspective, radius, strength, depth_range, bias):
    """The factor ``ao`` (float32, 1 at background samples) from the float32 eye depths *e* (+inf = background)."""
    e = np.asarray(e, dtype=F32)
    h, w = e.shape
    covered = np.isfinite(e)
    k, rng, bias, strength = F32(k), F32(depth_range), F32(bias), F32(strength)
    inv_fall = F32(1.0 / float(radius))
    with np.errstate(all="ignore"):
        rp = (k / e) if perspective else np.full_like(e, k)
        rp = np.where(rp > F32(1), rp, F32(1)).astype(F32)
        rp = np.where(rp < F32(MAX_RADIUS), rp, F32(MAX_RADIUS)).astype(F32)
        ys, xs = np.mgrid[0:h, 0:w]
        total = np.zeros((h, w), dtype=F32)
        for i in range(8):
            dx = np.rint(TAPS[i, 0] * rp).astype(np.int64)          # ties to even, like rintf
            dy = np.rint(TAPS[i, 1] * rp).astype(np.int64)

            def tap(sx, sy):
                inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
                v = e[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
                return np.where(inside, v, F32(np.inf)).astype(F32)
            a, b = tap(xs + dx, ys + dy), tap(xs - dx, ys - dy)
            da, db = (e - a).astype(F32), (e - b).astype(F32)
            valid = covered & np.isfinite(a) & np.isfinite(b) & (np.abs(da) <= rng) & (np.abs(db) <= rng)
            c = (da + db).astype(F32)
            t = ((c - bias).astype(F32) * inv_fall).astype(F32)
            occ = np.where(t < 0, F32(0), np.where(t > 1, F32(1), t)).astype(F32)
            total = (total + np.where(valid, occ, F32(0)).astype(F32)).astype(F32)
        ao = (F32(1) - (strength * (total * F32(0.125)).astype(F32)).astype(F32)).astype(F32)
        ao = np.where(ao < 0, F32(0), ao).astype(F32)
    return np.where(covered, ao, F32(1)).astype(F32)


def factor(z, m, k, perspective, radius, strength, depth_range, bias):
    return factor_from_depth(eye_depth(z, m), k, perspective, radius, strength, depth_range, bias)


def apply(z, frame, m, k, perspective, radius, strength, depth_range, bias):
    """F' = F * ao at covered samples, F itself at background samples: float32 (Hs, Ws, 3)."""
    frame = np.asarray(frame, dtype=F32)
    e = eye_depth(z, m)
    ao = factor_from_depth(e, k, perspective, radius, strength, depth_range, bias)
    return np.where(np.isfinite(e)[..., None], (frame * ao[..., None]).astype(F32), frame).astype(F32)
