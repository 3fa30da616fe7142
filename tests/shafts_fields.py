"""Synthetic inputs for the light shafts' kernels and mirror: seeded float frames in [0, 1] with a sky mask in the z-buffer,
at the sizes where the tree, the march or the composite can go wrong and no larger, and lights inside, on and outside the
frame.  ``mr_debug_light_shafts_post`` (the device), ``mr_host_light_shafts`` (the mirror) and shafts_ref.py (NumPy) all take
a ``Case``.  tests/test_shafts_cpu.py and tests/test_shafts_fields_gpu.py share the cases."""
import numpy as np

import shafts_ref

F32 = np.float32

LEVELS = (1, 2, 3, 4)                 # the library's d: every field runs at each
SOURCE_BLOCK = (4, 64)                # k_shaft_source's workgroup in coarse samples (rows, columns) up to d = 2; above, 64 columns of four samples: the width of d = 2
MARCH_BLOCK = 16                      # k_shaft_march's, 16 x 16 coarse samples

# the degenerate frames, two odd ones and a tall one
SMALL_SIZES = ((1, 1), (1, 2), (2, 3), (3, 5), (17, 33), (130, 9))
# 2^d k +- 1 on each axis, k = 3: a partial 2^d block at the top and the right border, or one sample into the next
TREE_SIZES = tuple(size for d in LEVELS for size in (((3 << d) - 1, (3 << d) + 1), ((3 << d) + 1, (3 << d) - 1)))
# the source kernel's block extent on the sample grid, +- 1 on both axes, for every d
BLOCK_SIZES = tuple(((SOURCE_BLOCK[0] << d) + a, (SOURCE_BLOCK[1] << d) + a) for d in LEVELS for a in (-1, 1))
# widths that are multiples of four samples -- rows on 16-byte boundaries, the wide loads of k_shaft_source -- with a lane
# whose block ends inside the row, with more than one workgroup across, and with nothing partial
ALIGNED_SIZES = ((18, 36), (10, 520), (64, 128))
FIELD = (66, 94)                      # what the masks and the lights are shown on: neither side a multiple of 4


def inside(fy, fx):
    """A light at that share of the level's extent."""
    return lambda h, w: (fx * (w - 1), fy * (h - 1))


def on_sample(y, x):
    """Exactly on the coarse sample nearest to that share of the extent: its ray has step 0."""
    return lambda h, w: (float(round(x * (w - 1))), float(round(y * (h - 1))))


def offset(fy, fx, dy=0.0, dx=0.0):
    """That share of the extent and a distance in coarse samples beyond it."""
    return lambda h, w: (fx * (w - 1) + dx, fy * (h - 1) + dy)


# name -> where the light stands on a level of (h, w)
LIGHTS = {
    "inside": inside(0.61, 0.37),
    "on a sample": on_sample(0.5, 0.25), "on the centre sample": on_sample(0.5, 0.5),
    "on the left border": offset(0.4, 0.0, dx=-0.5), "on the right border": offset(0.4, 1.0, dx=0.5),
    "on the bottom border": offset(0.0, 0.7, dy=-0.5), "on the top border": offset(1.0, 0.7, dy=0.5),
    "just left": offset(0.3, 0.0, dx=-0.75), "just right": offset(0.3, 1.0, dx=0.75),
    "just below": offset(0.0, 0.6, dy=-0.75), "just above": offset(1.0, 0.6, dy=0.75),
    "past the bottom left corner": offset(0.0, 0.0, dy=-1.25, dx=-1.5), "past the top right corner": offset(1.0, 1.0, dy=1.5, dx=1.25),
    "past the top left corner": offset(1.0, 0.0, dy=2.0, dx=-0.75), "past the bottom right corner": offset(0.0, 1.0, dy=-0.75, dx=2.0),
    "far outside": offset(0.5, 0.5, dy=3.0e6, dx=-7.0e6),
}


class Case:
    """One frame and z-buffer for the pass, the light as a rule for its place on the level, and the parameters as a
    ``LightShafts`` states them, but ``levels``: the library's d."""

    def __init__(self, name, frame, zbuf, light="inside", intensity=0.75, density=0.9, decay=0.97, samples=64, threshold=0.125, levels=2):
        self.name = name
        self.frame = np.ascontiguousarray(frame, dtype=F32)
        self.zbuf = np.ascontiguousarray(zbuf, dtype=np.float64)
        assert self.frame.ndim == 3 and self.frame.shape[2] == 3 and self.zbuf.shape == self.frame.shape[:2]
        self.light_name = light
        self.intensity, self.density, self.decay, self.samples = float(intensity), float(density), float(decay), int(samples)
        self.threshold, self.levels = float(threshold), int(levels)

    @property
    def shape(self):
        return self.frame.shape[:2]

    def __repr__(self):
        return (f"Case({self.name!r}, {self.shape}, light {self.light_name!r}, n={self.samples}, density={self.density}, t={self.threshold}, "
                f"d={self.levels})")

    def at(self, levels):
        """The same field at another d."""
        return Case(self.name, self.frame, self.zbuf, self.light_name, self.intensity, self.density, self.decay, self.samples, self.threshold, levels)

    @property
    def light(self):
        """(lx, ly) on level d, as the float32 the description carries."""
        lx, ly = LIGHTS[self.light_name](*shafts_ref.level_size(*self.shape, self.levels))
        return float(F32(lx)), float(F32(ly))

    def reference(self, mutant=None):
        return shafts_ref.reference(self.frame, self.zbuf, self.light, self.intensity, self.density, self.decay, self.samples, self.threshold,
                                    self.levels, mutant=mutant)

    def desc(self, native):
        return native.fill_light_shafts_desc(*self.light, self.threshold, float(F32(self.intensity)), float(shafts_ref.step(self.density, self.samples)),
                                             self.samples, self.levels, shafts_ref.weights(self.decay, self.samples))

    def mirror(self, native):
        return native.host_light_shafts(self.frame, self.zbuf, self.desc(native), fields=True)

    def device(self, native, handle):
        return native.debug_light_shafts_post(handle, self.frame, self.zbuf, self.desc(native), fields=True)


def bits(a, b):
    """Floats of *a* whose bits are not *b*'s."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def all_bits(got, want):
    """Floats of (out, S, R) *got* whose bits are not *want*'s, one count each."""
    return tuple(bits(a, b) for a, b in zip(got, want))


def seeded(size, seed=0):
    """A frame in [0, 1] with smooth parts and sharp ones."""
    rng = np.random.default_rng(1000 * size[0] + size[1] + seed)
    frame = rng.random(size + (3,), dtype=F32)
    dark = rng.random(size) < 0.5
    frame[dark] *= F32(0.5)
    frame[0, 0, 0] = F32(0.875)
    return frame


def zbuffer(sky):
    """A z-buffer whose *sky* samples are empty -- +inf, as a left-handed camera's k_tile leaves them, and -inf, a right-handed
    one's, in turn -- and whose others hold a depth."""
    sky = np.asarray(sky, dtype=bool)
    z = np.full(sky.shape, 0.5, dtype=np.float64)
    yy, xx = np.indices(sky.shape)
    z[sky] = np.where((yy + xx)[sky] % 3 == 0, -np.inf, np.inf)
    return z


def mask(size, kind, seed=0):
    h, w = size
    yy, xx = np.indices(size)
    if kind == "none":
        return np.zeros(size, bool)
    if kind == "all":
        return np.ones(size, bool)
    if kind == "bar":                                            # an occluder across the middle of a sky
        return ~((yy >= h // 3) & (yy < h // 3 + max(h // 6, 1)))
    if kind == "comb":                                           # teeth of three samples, five apart, from the bottom to two thirds up
        return ~((xx % 5 < 3) & (yy < 2 * h // 3))
    if kind == "corners":                                        # single sky samples in the corners
        m = np.zeros(size, bool)
        m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = True
        return m
    if kind == "random":
        return np.random.default_rng(77 * h + w + seed).random(size) < 0.6
    raise ValueError(kind)


def field(name, size, kind="random", seed=0, **kw):
    return Case(name, seeded(size, seed), zbuffer(mask(size, kind, seed)), **kw)


def cases():
    """Every field; each runs at every d."""
    out = [field(f"seeded {h}x{w}", (h, w)) for h, w in SMALL_SIZES + TREE_SIZES + BLOCK_SIZES + ALIGNED_SIZES]
    out += [field(f"mask {kind}", FIELD, kind, light="inside" if kind != "corners" else "past the top right corner") for kind in ("none", "all", "bar", "comb", "corners")]
    out += [field(f"light {name}", FIELD, "comb", light=name, density=1.0) for name in LIGHTS]
    out += [field(f"overshoot, light {name}", FIELD, "all", light=name, density=1.5) for name in ("inside", "on the right border", "past the top left corner")]
    out += [field(f"n = {n}", FIELD, "bar", samples=n, density=1.0) for n in (1, 2, 128)]
    out += [field(f"density {density}", FIELD, "comb", density=density, light="just above") for density in (0.25, 1.0, 1.5)]
    out.append(field("threshold 0", (17, 33), "random", threshold=0.0, decay=1.0))
    out.append(uniform())
    out.append(below())
    return out


def uniform(k=(3, 5), levels=2, light="inside", samples=64, density=1.0, decay=0.97):
    """A sky of 0.75 everywhere over a threshold of 0.375 -- k = 0.5 and S = 0.375, both dyadic -- on a grid whose sides are
    multiples of 2^4."""
    size = (16 * k[0], 16 * k[1])
    return Case("uniform sky", np.full(size + (3,), 0.75, dtype=F32), zbuffer(mask(size, "all")), light=light, intensity=1.0, density=density, decay=decay,
                samples=samples, threshold=0.375, levels=levels)


def below(size=(19, 35)):
    """No sky sample exceeds the threshold; the covered samples do."""
    sky = mask(size, "comb")
    frame = seeded(size)
    frame[sky] *= F32(0.5)
    return Case("below the threshold", frame, zbuffer(sky), threshold=0.5)


def occluder(levels=2):
    """A uniform sky with one block in it, left of a light on the grid's centre sample: a coarse sample left of the block
    marches through it, its mirror image right of the light through open sky."""
    size = (16 * 5, 16 * 9)
    sky = np.ones(size, bool)
    sky[32:48, 32:48] = False
    return Case("an occluder", np.full(size + (3,), 0.75, dtype=F32), zbuffer(sky), light="on the centre sample", density=1.0, samples=64, threshold=0.375, levels=levels)
