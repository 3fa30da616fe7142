"""Synthetic inputs for the bloom's kernels and mirror: seeded float frames in [0, 1] at the sizes where a pyramid can go
wrong and no larger, impulses, a uniform field and a field below the threshold.  ``mr_debug_bloom_post`` (the device),
``mr_host_bloom`` (the mirror) and bloom_ref.py (NumPy) all take a ``Case``.  tests/test_bloom_cpu.py and
tests/test_bloom_fields_gpu.py share the cases."""
import numpy as np

import bloom_ref

F32 = np.float32

# workgroup shapes as mr_debug_bloom_post numbers them (csrc/bloom.hip): output samples (wide, high), 256 threads each
BLOOM_TILES = ((32, 8), (64, 4), (16, 16))

# the degenerate frames, two odd ones and a tall one: 1 x 1 levels, levels of one row, sizes that halve with rounding
SMALL_SIZES = ((1, 1), (1, 2), (2, 3), (3, 5), (17, 33), (130, 9))


def _straddling():
    """For every shape (TW, TH): 2 TH +- 1 rows by 2 TW +- 1 columns, so that level 0 (staged by the first k_bloom_down)
    and level 1 (TH or TH + 1 rows by TW or TW + 1 columns: what it writes and the second one stages) both straddle a
    workgroup's edge."""
    sizes = []
    for tw, th in BLOOM_TILES:
        sizes += [(2 * th + a, 2 * tw + b) for a in (-1, 1) for b in (-1, 1)]
    return tuple(sizes)


STRADDLING = _straddling()
LEVELS = (1, 2, 3, 8)           # what the device test runs every field at
MASS_SIZE, MASS_AT = (96, 96), ((48, 47), (48, 48), (47, 47), (40, 44))


class Case:
    """One frame for the pass and its three parameters as a ``Bloom`` states them."""

    def __init__(self, name, frame, threshold=0.5, intensity=0.75, levels=4):
        self.name = name
        self.frame = np.ascontiguousarray(frame, dtype=F32)
        self.threshold, self.intensity, self.levels = float(threshold), float(intensity), int(levels)
        assert self.frame.ndim == 3 and self.frame.shape[2] == 3

    @property
    def shape(self):
        return self.frame.shape[:2]

    def __repr__(self):
        return f"Case({self.name!r}, {self.shape}, t={self.threshold}, i={self.intensity}, L={self.levels})"

    def at(self, levels):
        """The same frame at another number of levels."""
        return Case(self.name, self.frame, self.threshold, self.intensity, levels)

    def reference(self, mutant=None):
        return bloom_ref.reference(self.frame, self.threshold, self.intensity, self.levels, mutant=mutant)

    def desc(self, native):
        return native.fill_bloom_desc(self.threshold, float(bloom_ref.gain(self.intensity, self.levels)), self.levels)

    def mirror(self, native):
        return native.host_bloom(self.frame, self.desc(native), pyramid=True)

    def device(self, native, handle, shape=0):
        return native.debug_bloom_post(handle, self.frame, self.desc(native), shape, pyramid=True)


def bits(a, b):
    """Floats of *a* whose bits are not *b*'s."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def all_bits(got, want):
    """Floats of (frame, D, U) *got* whose bits are not *want*'s, as (frame, pyramid)."""
    pyramid = sum(bits(a, b) for a, b in zip(got[1], want[1])) + sum(bits(a, b) for a, b in zip(got[2], want[2]))
    assert len(got[1]) == len(want[1]) and len(got[2]) == len(want[2])
    return bits(got[0], want[0]), pyramid


def seeded(size, seed=0):
    """A frame in [0, 1] with smooth parts and sharp ones: about a third of its samples exceed 0.5."""
    rng = np.random.default_rng(1000 * size[0] + size[1] + seed)
    frame = rng.random(size + (3,), dtype=F32)
    dark = rng.random(size) < 0.5
    frame[dark] *= F32(0.5)
    frame[0, 0, 0] = F32(0.875)          # (the corner sample glows at any size, the 1 x 1 frame's only one too)
    return frame


def impulse(size, at, value=(1.0, 0.5, 0.25)):
    frame = np.zeros(size + (3,), dtype=F32)
    frame[at] = value
    return frame


def cases():
    """Every field, at the levels its name gives a reason for."""
    out = [Case(f"seeded {h}x{w}", seeded((h, w)), levels=4) for h, w in SMALL_SIZES + STRADDLING]
    # its levels are 1 x 2, 1 x 1, 1 x 1, ...: 1 x 1 halves to 1 x 1 before the levels are used up
    out.append(Case("levels run out", seeded((2, 3), seed=7), threshold=0.25, levels=6))
    odd = (17, 33)
    out += [Case("impulse in a corner", impulse(odd, (0, 0))), Case("impulse in the far corner", impulse(odd, (16, 32))),
            Case("impulse on an edge", impulse(odd, (9, 0))), Case("impulse on the top edge", impulse(odd, (16, 11))),
            Case("impulse in the interior", impulse(odd, (8, 15)))]
    out.append(uniform())
    out.append(below())
    out.append(mass(3))
    return out


def uniform(size=(21, 38), levels=4):
    """0.75 everywhere over a threshold of 0.375: k = 0.5 and the bright value b = 0.375, both dyadic."""
    return Case("uniform", np.full(size + (3,), 0.75, dtype=F32), threshold=0.375, intensity=1.0, levels=levels)


def below(size=(19, 35)):
    """No sample exceeds the threshold."""
    return Case("below the threshold", seeded(size) * F32(0.5), threshold=0.5, levels=4)


def mass(levels, at=MASS_AT[0]):
    """One bright sample far from every border (at L <= 3 its glow reaches 15 samples: it ends 25 samples short of them) whose bright value is a
    power of two in every channel: (1, 0.5, 0.25) over a threshold of 0.5 is k = 0.5 and B0 = (0.5, 0.25, 0.125).
    intensity = levels makes the gain 1."""
    return Case("interior mass", impulse(MASS_SIZE, at, (1.0, 0.5, 0.25)), threshold=0.5, intensity=float(levels), levels=levels)
