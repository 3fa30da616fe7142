"""The bloom's definition (csrc/bloom_def.h, include/mi355rast.h) restated in NumPy float32, every operation rounded on
its own, and named mutants of it: each is a way the kernels or the mirror could go wrong that the fields of
bloom_fields.py must tell from the definition (tests/test_bloom_cpu.py).

    reference(frame, threshold, intensity, levels, mutant=None) -> (out, D, U)

with ``D[l - 1]`` the level ``D_l`` and ``U[l - 1]`` the level ``U_l`` (``U[-1]`` is ``D[-1]``), rows bottom-up like the frame."""
import numpy as np

F32 = np.float32
THREE = F32(3.0)

MUTANTS = ("zero_padding",        # taps outside a level read 0, not the nearest sample
           "floor_sizes",         # H_l = H_{l-1} // 2 (at least 1), not the ceiling
           "columns_first",       # the down filter sums the four rows of a column first
           "threshold_on_mean",   # the bright pass compares the channels' mean, not their maximum
           "far_wrong_side",      # far = near + 1 for even fine indices and near - 1 for odd ones
           "missing_level",       # the up chain starts at U_{L-1} = D_{L-1}: the coarsest level is never added
           "gain_undivided")      # gain = intensity, not intensity / levels


def gain(intensity, levels, mutant=None):
    """What the packer sends as ``gain``: float32(intensity / levels), evaluated in float64."""
    if mutant == "gain_undivided":
        return F32(intensity)
    return F32(np.float64(intensity) / np.float64(levels))


def level_sizes(height, width, levels, mutant=None):
    sizes = []
    for _ in range(levels):
        if mutant == "floor_sizes":
            height, width = max(height // 2, 1), max(width // 2, 1)
        else:
            height, width = (height + 1) // 2, (width + 1) // 2
        sizes.append((height, width))
    return sizes


def bright(frame, threshold, mutant=None):
    r, g, b = frame[..., 0], frame[..., 1], frame[..., 2]
    if mutant == "threshold_on_mean":
        m = ((r + g) + b) / THREE
    else:
        m = np.maximum(np.maximum(r, g), b)
    t = F32(threshold)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(m > t, (m - t) / m, F32(0.0)).astype(F32)
    return frame * k[..., None]


def _four(a0, a1, a2, a3):
    return (a0 + a3) + THREE * (a1 + a2)


def down(src, size, mutant=None):
    """One level down: *src* ``(h, w, 3)`` onto *size* ``(dh, dw)``."""
    h, w = src.shape[:2]
    dh, dw = size
    rows = 2 * np.arange(dh)[:, None] - 1 + np.arange(4)[None, :]          # (dh, 4) source rows, ascending
    cols = 2 * np.arange(dw)[:, None] - 1 + np.arange(4)[None, :]
    inside = ((rows >= 0) & (rows < h))[:, :, None, None] & ((cols >= 0) & (cols < w))[None, None, :, :]
    taps = src[np.clip(rows, 0, h - 1)[:, :, None, None], np.clip(cols, 0, w - 1)[None, None, :, :]]      # (dh, 4, dw, 4, 3)
    if mutant == "zero_padding":
        taps = np.where(inside[..., None], taps, F32(0.0))
    if mutant == "columns_first":
        c = _four(taps[:, 0], taps[:, 1], taps[:, 2], taps[:, 3])          # (dh, dw, 4, 3)
        v = _four(c[:, :, 0], c[:, :, 1], c[:, :, 2], c[:, :, 3])
    else:
        r = _four(taps[:, :, :, 0], taps[:, :, :, 1], taps[:, :, :, 2], taps[:, :, :, 3])      # (dh, 4, dw, 3)
        v = _four(r[:, 0], r[:, 1], r[:, 2], r[:, 3])
    return (v * F32(1.0 / 64.0)).astype(F32)


def _near_far(n_fine, n_coarse, mutant=None):
    i = np.arange(n_fine)
    near = i // 2
    step = np.where(i % 2 == 0, -1, 1)
    if mutant == "far_wrong_side":
        step = -step
    return np.minimum(near, n_coarse - 1), np.clip(near + step, 0, n_coarse - 1)


def up(coarse, size, mutant=None):
    """up(C) onto a finer grid *size* ``(H, W)``."""
    ch, cw = coarse.shape[:2]
    ny, fy = _near_far(size[0], ch, mutant)
    nx, fx = _near_far(size[1], cw, mutant)
    h = THREE * coarse[:, nx] + coarse[:, fx]                               # (ch, W, 3)
    v = THREE * h[ny] + h[fy]
    return (v * F32(1.0 / 16.0)).astype(F32)


def reference(frame, threshold, intensity, levels, mutant=None):
    frame = np.ascontiguousarray(frame, dtype=F32)
    sizes = level_sizes(frame.shape[0], frame.shape[1], levels, mutant)
    level, D = bright(frame, threshold, mutant), []
    for size in sizes:
        level = down(level, size, mutant)
        D.append(level)
    U = [None] * levels
    U[-1] = D[-1]
    for l in range(levels - 2, -1, -1):
        if mutant == "missing_level" and l == levels - 2:
            U[l] = D[l]
        else:
            U[l] = D[l] + up(U[l + 1], D[l].shape[:2], mutant)
    out = frame + gain(intensity, levels, mutant) * up(U[0], frame.shape[:2], mutant)
    return out.astype(F32), D, U
