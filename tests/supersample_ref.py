"""What a supersampled frame must be, restated in NumPy (the contract of ``Scene.supersample``).

Ordered-grid supersampling is *defined* as upstream's frame on an s-times finer grid, box-filtered before
upstream's finalise: the oracle renders the sample grid -- a twin of the scene at ``(s*H, s*W)`` whose camera
offsets are multiplied by s -- and three lines of NumPy give the expected output."""
import numpy as np

import scenes


def resolve(frame_f32, s):
    """float32 (s*H, s*W, 3) sample grid, rows bottom-up like the reference's buffers -> uint8 (H, W, 3), row 0 = top."""
    f = np.asarray(frame_f32, dtype=np.float32)
    h, w = f.shape[0] // s, f.shape[1] // s
    fr = f.reshape(h, s, w, s, 3).mean(axis=(1, 3))
    return (fr[::-1] ** 0.8 * 255).astype(np.uint8)


def pair(api, name, s, offsets=(0, 0), **kw):
    """(scene at its recipe's resolution with supersample = s, twin at (s*H, s*W) with the offsets times s)."""
    fn = getattr(scenes, name)
    scene = fn(api, **kw)
    h, w = scene.resolution
    twin = fn(api, **{**kw, "resolution": (s * h, s * w)})
    scene.supersample = s
    scene.camera.x_offset, scene.camera.y_offset = offsets
    twin.camera.x_offset, twin.camera.y_offset = offsets[0] * s, offsets[1] * s
    return scene, twin


def max_diff(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, (a.shape, b.shape)
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return int(d.max()), int((d == 1).any(axis=-1).sum())
