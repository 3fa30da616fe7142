"""Synthetic inputs for the temporal anti-aliasing's kernel and mirror: seeded float frames F, velocity fields U that no
camera produces and histories P.  ``mr_debug_taa_post`` (the device), ``mr_host_taa`` (the mirror) and taa_ref.py (NumPy)
all take a ``Case``.  tests/test_taa_cpu.py and tests/test_taa_fields_gpu.py share the cases."""
import numpy as np

import taa_ref

F32 = np.float32
FLT_MIN = F32(np.finfo(np.float32).tiny)

# workgroup shapes as mr_debug_taa_post numbers them (csrc/taa.hip): samples (wide, high), 256 threads each
TAA_TILES = ((32, 8), (64, 4), (16, 16))


def _sizes():
    """(rows, cols): the degenerate frames; for every shape one sample less than its rectangle, the rectangle and one more,
    in each direction and in both; one odd size of a few rectangles of every shape."""
    sizes = [(1, 1), (1, 7), (7, 1)]
    for tw, th in TAA_TILES:
        sizes += [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (th - 1, tw + 1), (th + 1, tw - 1)]
    return tuple(sizes + [(37, 130)])


SIZES = _sizes()
ODD = (37, 130)


class Case:
    """One frame for the pass: F, U, P (None: no history) and the blend."""

    def __init__(self, name, frame, velocity, history, blend):
        self.name = name
        self.frame = np.ascontiguousarray(frame, dtype=F32)
        self.velocity = np.ascontiguousarray(velocity, dtype=F32)
        self.history = None if history is None else np.ascontiguousarray(history, dtype=F32)
        self.blend = float(blend)
        assert self.velocity.shape == self.frame.shape[:2] + (2,)
        assert self.history is None or self.history.shape == self.frame.shape

    @property
    def shape(self):
        return self.frame.shape[:2]

    def __repr__(self):
        return f"Case({self.name!r}, {self.shape}, blend={self.blend})"

    def reference(self, mutant=None, detail=False):
        return taa_ref.apply(self.frame, self.velocity, self.history, self.blend, mutant=mutant, detail=detail)

    def mirror(self, native):
        return native.host_taa(self.frame, self.velocity, self.history, self.blend)

    def device(self, native, handle, shape=0):
        return native.debug_taa_post(handle, self.frame, self.velocity, self.history, self.blend, shape)


def bits(a, b):
    """Floats of *a* whose bits are not *b*'s."""
    return int((np.ascontiguousarray(a, dtype=F32).view(np.uint32) != np.ascontiguousarray(b, dtype=F32).view(np.uint32)).sum())


def colours(shape, seed):
    """(F, P): F in [0.25, 0.75], P in [0, 1], so a fetched history lies below the neighbourhood's minimum about as often as
    above its maximum: both sides of the clamp bind."""
    rng = np.random.default_rng(seed)
    f = F32(0.25) + F32(0.5) * rng.random(tuple(shape) + (3,), dtype=np.float32)
    return f, rng.random(tuple(shape) + (3,), dtype=np.float32)


def constant(shape, ux, uy):
    u = np.empty(tuple(shape) + (2,), dtype=F32)
    u[..., 0], u[..., 1] = ux, uy
    return u


def _above(v):
    """The float32 next above *v* >= 0, without a subnormal: the smallest normal above 0."""
    return FLT_MIN if v == 0 else np.nextafter(F32(v), F32(np.inf))


def to_last_column(shape):
    """Every sample's target lies exactly on column Ws - 1 (x1 = x0 + 1 is clamped there, fx = 0), on its own row."""
    h, w = shape
    u = constant(shape, 0.0, 0.0)
    u[..., 0] = np.arange(w, dtype=F32)[None, :] - F32(w - 1)
    return u


def to_last_row(shape):
    h, w = shape
    u = constant(shape, 0.0, 0.0)
    u[..., 1] = np.arange(h, dtype=F32)[:, None] - F32(h - 1)
    return u


def ulp_outside(shape):
    """Targets one float32 outside each of the four borders: column 0 looks just left of 0, column Ws - 1 just right of
    Ws - 1, row 0 just below 0, row Hs - 1 just above Hs - 1 (the corners both ways); every other sample is at rest.  All
    of these are off the frame: out = C."""
    h, w = shape
    u = constant(shape, 0.0, 0.0)
    u[:, 0, 0] = FLT_MIN                                           # rx = 0 - FLT_MIN < 0
    u[:, w - 1, 0] = F32(w - 1) - _above(w - 1)                    # rx = (Ws - 1) + one ulp, exactly
    u[0, :, 1] = FLT_MIN
    u[h - 1, :, 1] = F32(h - 1) - _above(h - 1)
    return u


def wild(shape, seed):
    """Every component drawn from: far outside either way (1e30), no number, either infinity, zero, half a sample."""
    rng = np.random.default_rng(seed)
    menu = np.array([1e30, -1e30, np.nan, np.inf, -np.inf, 0.0, 0.5, -0.5], dtype=F32)
    return menu[rng.integers(0, len(menu), tuple(shape) + (2,))]


def scattered(shape, seed, reach=20.0):
    """Seeded displacements of up to *reach* samples either way on both axes: the fetches cross workgroup borders in every
    direction (and many leave the frame)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-reach, reach, tuple(shape) + (2,)).astype(F32)


def rotation(shape, rate=0.3):
    """A turn round the frame's centre: smooth, fractional, every direction, growing towards the borders."""
    h, w = shape
    ys, xs = np.mgrid[0:h, 0:w]
    u = constant(shape, 0.0, 0.0)
    u[..., 0], u[..., 1] = -rate * (ys - (h - 1) / 2), rate * (xs - (w - 1) / 2)
    return u


def checker(shape, seed):
    """(F, P) that bind neither side of the clamp: F alternates 0.1 / 0.9 from sample to sample, so every neighbourhood of
    a frame with two columns or rows spans [0.1, 0.9]; P lies in [0.2, 0.8], and so does anything interpolated from it."""
    h, w = shape
    ys, xs = np.mgrid[0:h, 0:w]
    f = np.where(((ys + xs) & 1)[..., None] == 0, F32(0.1), F32(0.9)) * np.ones(3, dtype=F32)
    p = F32(0.2) + F32(0.6) * np.random.default_rng(seed).random(tuple(shape) + (3,), dtype=np.float32)
    return f.astype(F32), p


def cases(shape):
    """Every case at one size."""
    h, w = shape
    f, p = colours(shape, 11)
    out = [Case("zero", f, constant(shape, 0, 0), p, 0.1),
           Case("zero_same", f, constant(shape, 0, 0), f.copy(), 0.1),
           Case("no_history", f, scattered(shape, 12, 3.0), None, 0.1),
           Case("whole", f, constant(shape, 2.0, -1.0), p, 0.1),
           Case("fraction", f, constant(shape, 0.37, -1.62), p, 0.1),
           Case("fraction_blend1", f, constant(shape, -2.25, 0.5), p, 1.0),
           Case("last_column", f, to_last_column(shape), p, 0.1),
           Case("last_row", f, to_last_row(shape), p, 0.25),
           Case("ulp_outside", f, ulp_outside(shape), p, 0.1),
           Case("wild", f, wild(shape, 13), p, 0.1),
           Case("scattered", f, scattered(shape, 14), p, 0.05),
           Case("rotation_blend1", f, rotation(shape), p, 1.0)]
    cf, cp = checker(shape, 15)
    out.append(Case("neither_binds", cf, constant(shape, 0.5, -0.25), cp, 0.1))
    # a history with texels that are no number: H is mn there (taa_def.h).  Column 0 of every row but the first is one --
    # the texel behind column Ws - 1 in memory, which a fetch on the last column must not touch
    holes = p.copy()
    if w > 1:
        holes[1:, 0] = np.nan
    out.append(Case("last_column_holes", f, to_last_column(shape), holes, 0.1))
    sprinkled = p.copy()
    sprinkled[np.random.default_rng(16).random(shape) < 0.2] = np.nan
    out.append(Case("sprinkled_holes", f, scattered(shape, 17, 4.0), sprinkled, 0.1))
    return out
