"""Seeded float frames for the tone mapping's tests, each with the description it is metered under.

Sizes: 1 x 1, 1 x 3, 2 x 3, 3 x 5, 7 x 13, 64 x 65, 37 x 53 and 128 x 130 -- sample counts of 0, 1, 2 and 3 modulo 4 (a thread
of ``k_lum_hist`` takes four samples, the rest is a scalar tail), one workgroup's worth and less, five workgroups and
seventeen.  The fields:

* uniform frames (luminance 0.18; a dim one whose target exposure the clamp cuts);
* an all-black frame, with and without a previous exposure (nothing is metered: M == 0);
* the ramp: one sample in the middle of each of the bins 1 .. 255, the bit patterns on both sides of every octave boundary
  from 2^-24 (its predecessor is black) to 2^8, denormals, 0, values above 2^8 (all bin 255);
* samples whose bin depends on the order the luminance is summed in;
* log-uniform noise over 2^-10 .. 2^3, also scaled by 2^-3 and 2^2, at the trims (0, 1000), (500, 950), (0, 1), adapting
  from a previous exposure, under Reinhard's curve;
* a trim that keeps no sample (M == 0 though the frame is not black).
"""
import numpy as np

import tonemap_ref as ref

f32 = np.float32
SIZES = ((1, 1), (1, 3), (2, 3), (3, 5), (7, 13), (64, 65), (37, 53))
LARGE = (128, 130)
GRID_CAPS = (1, 2, 3, 0)               # of k_lum_hist: the stride loop, a few slab rows, the library's default
# two samples whose luminance lies in bin 176 summed as the definition says and in bin 175 summed the other way, and
# the reverse (found by search; test_tonemap_cpu.py checks that they still do)
ORDER_BITS = ((1044085607, 1049683314, 1039533985), (1053258889, 1046666451, 1039638956))


def bits(a, b):
    """How many 32-bit words of two arrays differ."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


class Case:
    def __init__(self, name, frame, params=None, e_prev=None):
        self.name, self.frame = name, np.ascontiguousarray(frame, dtype=f32)
        self.params, self.e_prev = params or ref.Params(), e_prev
        assert self.frame.ndim == 3 and self.frame.shape[2] == 3

    shape = property(lambda self: self.frame.shape[:2])

    def at(self, e_prev="same", **over):
        """The same frame under a description with *over* replaced, and another previous exposure."""
        return Case(self.name, self.frame, self.params.replace(**over), self.e_prev if isinstance(e_prev, str) else e_prev)

    def desc(self, native):
        p = self.params
        return native.fill_tone_map_desc(ref.OPERATORS.index(p.operator), int(p.exposure is not None), 1.0 if p.exposure is None else p.exposure,
                                         p.key, p.white, p.speed, p.min_exposure, p.max_exposure, p.low_pm, p.high_pm, ref.EXP2)

    def reference(self, mutant=None):
        return ref.tone_map(self.frame, self.params, self.e_prev, mutant)

    def mirror(self, native):
        return native.host_tone_map(self.frame, self.desc(native), self.e_prev)

    def device(self, native, handle, grid_cap=0, form=-1):
        return native.debug_tone_map_post(handle, self.frame, self.desc(native), self.e_prev, grid_cap, form)

    def __repr__(self):
        return f"{self.name} {self.shape[0]}x{self.shape[1]} {self.params!r} e_prev={self.e_prev!r}"


def same(got, want):
    """(floats of the frame, counts of the histogram, 0 or 1 for the exposure) that are not the other's bits."""
    return bits(got[0], want[0]), bits(got[1], want[1]), bits(np.asarray([got[2]], f32), np.asarray([want[2]], f32))


def uniform(size, value=0.18):
    return np.full(size + (3,), value, f32)


def noise(size, seed=11, k=0):
    """Log-uniform luminance over 2^-10 .. 2^3 with a tint of 1/2 .. 1 a channel, times 2^k (exact)."""
    rng = np.random.default_rng(seed)
    lum = np.exp2(rng.uniform(-10.0, 3.0, size + (1,)))
    return np.ldexp((lum * rng.uniform(0.5, 1.0, size + (3,))).astype(f32), k).astype(f32)


def ramp():
    values = [np.ldexp(1.0 + ((i & 7) + 0.5) / 8.0, (i >> 3) - 24) for i in range(1, 256)]
    for k in range(-24, 9):
        edge = f32(np.ldexp(1.0, k))
        values += [edge, np.nextafter(edge, f32(0))]
    values += [0.0, 1e-40, float(np.nextafter(f32(0), f32(1))), 300.0, 1000.0, 65504.0]
    values = np.asarray(values, f32)
    width = 37
    grey = np.zeros(-(-len(values) // width) * width, f32)
    grey[:len(values)] = values
    return np.repeat(grey.reshape(-1, width, 1), 3, axis=2)


def order_pair():
    """(the first sample twice: the two alone would only swap their bins)"""
    return np.asarray((ORDER_BITS[0],) + ORDER_BITS, np.uint32).view(f32).reshape(1, 3, 3)


def cases():
    P = ref.Params
    out = [Case(f"uniform {h}x{w}", uniform((h, w))) for h, w in SIZES]
    out += [Case(f"noise {h}x{w}", noise((h, w), seed=h * 100 + w)) for h, w in SIZES + (LARGE,)]
    out += [
        Case("dim uniform, the clamp cuts", uniform((3, 5), 2.0 ** -12)),
        Case("bright uniform, the clamp cuts", uniform((3, 5), 200.0), P(operator="reinhard")),
        Case("black", np.zeros((7, 13, 3), f32)),
        Case("black with a previous exposure", np.zeros((7, 13, 3), f32), P(speed=0.5), e_prev=2.5),
        Case("ramp", ramp()),
        Case("ramp, linear", ramp(), P(operator="linear")),
        Case("ramp, trimmed", ramp(), P(low_pm=100, high_pm=900, operator="reinhard", white=2.0)),
        Case("summation order", order_pair(), P(operator="linear")),
        Case("noise / 8", noise((37, 53), k=-3)),
        Case("noise * 4", noise((37, 53), k=2)),
        Case("noise, trims 500 950", noise((37, 53)), P(low_pm=500, high_pm=950)),
        Case("noise, trims 0 1", noise((37, 53)), P(low_pm=0, high_pm=1)),
        Case("noise, no sample kept", noise((7, 13)), P(low_pm=0, high_pm=1)),
        Case("noise, no sample kept, previous", noise((7, 13)), P(low_pm=0, high_pm=1, speed=0.25), e_prev=0.75),
        Case("noise, adapting", noise((37, 53)), P(speed=0.25), e_prev=2.0),
        Case("noise, adapting down, reinhard", noise((64, 65)), P(speed=0.0625, operator="reinhard", key=0.5), e_prev=0.01),
        Case("noise, fixed", noise((37, 53)), P(exposure=0.7, operator="aces")),
        Case("noise, narrow bounds", noise((37, 53)), P(min_exposure=0.9, max_exposure=1.1, key=0.09)),
    ]
    return out
