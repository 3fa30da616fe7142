"""What an accumulation must be, restated in NumPy (the contract of ``Scene.accumulate`` / ``mr_accum_*``).

    A_0 = w_0 * F_0,   A_k = A_{k-1} + (w_k * F_k)          float32, every operation rounded on its own
    M   = mean of A over each s x s block                   summed row by row from the block's bottom-left sample, times 1 / s^2
    R   = min(M * scale, 1)
    out = uint8(R ** 0.8 * 255), rows flipped

The block sum is the explicit ``j, i`` loop: ``mean(axis=...)`` adds in another order."""
import numpy as np


def default_scale(weights):
    """``float32(1 / sum of the weights as given)``, the sum and the division in float64."""
    return np.float32(1.0 / float(np.sum(np.asarray(weights, dtype=np.float64))))


def accumulate(frames, weights):
    """A: float32 (Hs, Ws, 3) from frames (n, Hs, Ws, 3) and one weight each."""
    acc = None
    for frame, weight in zip(frames, weights):
        part = np.float32(weight) * np.asarray(frame, dtype=np.float32)
        acc = part if acc is None else acc + part
    assert acc.dtype == np.float32
    return acc


def block_mean(acc, s):
    """M: float32 (Hs / s, Ws / s, 3).  Rows stay bottom-up; row j of a block is j rows above its bottom-left sample."""
    acc = np.asarray(acc, dtype=np.float32)
    h, w = acc.shape[0] // s, acc.shape[1] // s
    total = np.zeros((h, w, 3), dtype=np.float32)
    for j in range(s):
        for i in range(s):
            total = total + acc[j::s, i::s]
    return total * np.float32(1.0 / (s * s))


def finalise(acc, s=1, scale=1.0):
    """uint8 (H, W, 3), row 0 = top."""
    r = np.minimum(block_mean(acc, s) * np.float32(scale), np.float32(1.0))
    assert r.dtype == np.float32
    return (r ** 0.8 * 255).astype(np.uint8)[::-1]


def result(frames, weights, s=1, scale=None):
    """(A, bytes) of the definition; *scale* defaults like ``Accumulation.result``'s."""
    acc = accumulate(frames, weights)
    return acc, finalise(acc, s, default_scale(weights) if scale is None else scale)
