"""The light shafts' definition (csrc/shafts_def.h, include/mi355rast.h) restated in NumPy float32, every operation rounded
on its own, and named mutants of it: each is a way the kernels or the mirror could go wrong that the fields of
shafts_fields.py must tell from the definition (tests/test_shafts_cpu.py).

    reference(frame, zbuf, light, intensity, density, decay, samples, threshold, levels, mutant=None) -> (out, S, R)

with ``light`` the light's ``(lx, ly)`` on level ``levels``, ``S`` the march's source and ``R`` its result, both
``(H_d, W_d, 3)``, rows bottom-up like the frame."""
import numpy as np

F32 = np.float32
QUARTER, HALF = F32(0.25), F32(0.5)

MUTANTS = ("clamped_taps",            # a tap outside the level reads the nearest sample instead of nothing
           "mask_inverted",           # the covered samples are the source, not the sky
           "columns_first",           # the tree adds the two samples of a column first
           "floor_sizes",             # H_l = H_{l-1} // 2 (at least 1), not the ceiling
           "weights_unnormalised",    # w_i = decay^i, not divided by their sum
           "step_n_minus_1",          # step = density / (n - 1)
           "no_half_offset",          # the composite reads R at x * 2^-d, not (x + 0.5) * 2^-d - 0.5
           "from_the_light")          # tap i lies at light + (sample - light) * step * i


def weights(decay, samples, mutant=None):
    """w_0 = 1, w_{i+1} = w_i * decay in float64, divided by their sum, rounded to float32."""
    w, value = [], np.float64(1.0)
    for _ in range(samples):
        w.append(value)
        value = value * np.float64(decay)
    w = np.array(w, dtype=np.float64)
    if mutant != "weights_unnormalised":
        w = w / w.sum()
    return w.astype(F32)


def step(density, samples, mutant=None):
    n = max(samples - 1, 1) if mutant == "step_n_minus_1" else samples
    return F32(np.float64(density) / np.float64(n))


def level_size(height, width, levels, mutant=None):
    for _ in range(levels):
        if mutant == "floor_sizes":
            height, width = max(height // 2, 1), max(width // 2, 1)
        else:
            height, width = (height + 1) // 2, (width + 1) // 2
    return height, width


def bright(frame, threshold):
    """bloom_def.h's bright factor times the frame."""
    m = np.maximum(np.maximum(frame[..., 0], frame[..., 1]), frame[..., 2])
    t = F32(threshold)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(m > t, (m - t) / m, F32(0.0)).astype(F32)
    return frame * k[..., None]


def source0(frame, zbuf, threshold, mutant=None):
    sky = ~np.isfinite(zbuf)
    if mutant == "mask_inverted":
        sky = ~sky
    return np.where(sky[..., None], bright(frame, threshold), F32(0.0)).astype(F32)


def halve(level, mutant=None):
    """One level up the tree; what lies beyond the level counts +0."""
    h, w = level.shape[:2]
    nh, nw = level_size(h, w, 1, mutant)
    padded = np.zeros((2 * nh, 2 * nw, 3), dtype=F32)
    hh, ww = min(h, 2 * nh), min(w, 2 * nw)
    padded[:hh, :ww] = level[:hh, :ww]
    a00, a01, a10, a11 = padded[0::2, 0::2], padded[0::2, 1::2], padded[1::2, 0::2], padded[1::2, 1::2]
    if mutant == "columns_first":
        return ((a00 + a10) + (a01 + a11)) * QUARTER
    return ((a00 + a01) + (a10 + a11)) * QUARTER


def fetch(level, qx, qy, mutant=None):
    """fetch(A, qx, qy) at arrays of positions: ``(value, inside)``; the value is +0 where the position is outside."""
    h, w = level.shape[:2]
    qx, qy = np.asarray(qx, dtype=F32), np.asarray(qy, dtype=F32)
    with np.errstate(invalid="ignore"):
        inside = (qx >= F32(-0.5)) & (qx <= F32(w) - HALF) & (qy >= F32(-0.5)) & (qy <= F32(h) - HALF)
        take = inside | (np.isfinite(qx) & np.isfinite(qy)) if mutant == "clamped_taps" else inside
        ux = np.where(take, np.minimum(np.maximum(qx, F32(0.0)), F32(w - 1)), F32(0.0)).astype(F32)
        uy = np.where(take, np.minimum(np.maximum(qy, F32(0.0)), F32(h - 1)), F32(0.0)).astype(F32)
    x0, y0 = ux.astype(np.int32), uy.astype(np.int32)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (ux - x0.astype(F32))[..., None], (uy - y0.astype(F32))[..., None]
    a00, a01, a10, a11 = level[y0, x0], level[y0, x1], level[y1, x0], level[y1, x1]
    h0 = a00 + fx * (a01 - a00)
    h1 = a10 + fx * (a11 - a10)
    v = h0 + fy * (h1 - h0)
    return np.where(take[..., None], v, F32(0.0)).astype(F32), take


def march(S, light, step_, w, mutant=None):
    h, wd = S.shape[:2]
    cy, cx = np.meshgrid(np.arange(h, dtype=F32), np.arange(wd, dtype=F32), indexing="ij")
    lx, ly = F32(light[0]), F32(light[1])
    with np.errstate(over="ignore", invalid="ignore"):
        if mutant == "from_the_light":
            dx, dy = (cx - lx) * step_, (cy - ly) * step_
            ox, oy = np.full_like(cx, lx), np.full_like(cy, ly)
        else:
            dx, dy = (lx - cx) * step_, (ly - cy) * step_
            ox, oy = cx, cy
        acc = np.zeros((h, wd, 3), dtype=F32)
        for i in range(len(w)):
            v, inside = fetch(S, ox + dx * F32(i), oy + dy * F32(i), mutant)
            acc = np.where(inside[..., None], acc + w[i] * v, acc).astype(F32)
    return acc


def reference(frame, zbuf, light, intensity, density, decay, samples, threshold, levels, mutant=None):
    frame = np.ascontiguousarray(frame, dtype=F32)
    level = source0(frame, np.asarray(zbuf, dtype=np.float64), threshold, mutant)
    for _ in range(levels):
        level = halve(level, mutant)
    S = level.astype(F32)
    R = march(S, light, step(density, samples, mutant), weights(decay, samples, mutant), mutant)
    inv = F32(1.0 / (1 << levels))
    y, x = np.meshgrid(np.arange(frame.shape[0], dtype=F32), np.arange(frame.shape[1], dtype=F32), indexing="ij")
    if mutant == "no_half_offset":
        qx, qy = x * inv, y * inv
    else:
        qx, qy = (x + HALF) * inv - HALF, (y + HALF) * inv - HALF
    glow, _ = fetch(R, qx, qy)
    out = frame + F32(intensity) * glow
    return out.astype(F32), S, R
