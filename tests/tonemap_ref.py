"""The tone mapping's definition (csrc/tonemap_def.h) restated in NumPy, and its named mutants.

float32 throughout with every operation rounded on its own, or Python integers::

    luminance   Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b
    bin         b = clamp((bits(Y) >> 20) - ((127 - 24) << 3), 0, 255)
    histogram   n[i] = samples in bin i;  n[0] := 0
    trim        N = sum n;  lo = N*low_pm // 1000;  hi = N*high_pm // 1000;  C_i = n[1] + .. + n[i-1]
                u_i = max(0, min(C_i + n[i], hi) - max(C_i, lo))
    centre      c_i = ((i >> 3) - 24) * 256 + FRAC[i & 7]
    mean        S = sum u_i*c_i;  M = sum u_i;  q = floor((2S + M) / (2M))
    target      -q = 256*a + f;  e_t = clamp(ldexp(key * EXP2[f], a), min_exposure, max_exposure)
    adapt       e = e_prev + speed * (e_t - e_prev) with a previous exposure, else e_t;  M == 0: e_prev, else 1
    curve       x = F * e;  linear x;  reinhard (x * (1 + x / (white*white))) / (1 + x);
                aces min((x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f), 1)

``tone_map(frame, params, e_prev, mutant)`` returns ``(frame, histogram, exposure)``.  A mutant is the definition with one
mistake; tests/test_tonemap_cpu.py shows that each is told apart from the definition by a field of tonemap_fields.py.
"""
import numpy as np

f32 = np.float32
FRAC = (22, 63, 100, 134, 165, 193, 220, 244)
OPERATORS = ("linear", "reinhard", "aces")
EXP2 = np.exp2(np.arange(256, dtype=np.float64) / 256.0).astype(np.float32)

MUTANTS = {
    "luminance_order": "luminance summed in another order: 0.2126 r + (0.7152 g + 0.0722 b)",
    "shift_21": "the shift by 21 instead of 20",
    "bin0_metered": "bin 0 metered in",
    "hi_inclusive": "hi inclusive: the sample of rank hi is kept too",
    "trunc_div": "truncating division for q",
    "frac_shift": "FRAC off by one entry",
    "clamp_first": "the clamp before ldexp",
    "adapt_reversed": "adaptation from e_t towards e_prev",
    "aces_no_min": "the ACES min left out",
    "white_unsquared": "Reinhard's white not squared",
}


class Params:
    """A description as the library takes it: the operator's name, a fixed exposure or None, the meter."""

    def __init__(self, operator="aces", exposure=None, key=0.18, low_pm=0, high_pm=1000, speed=1.0, white=4.0, min_exposure=2.0 ** -6,
                 max_exposure=2.0 ** 6):
        self.operator, self.exposure, self.key, self.low_pm, self.high_pm = operator, exposure, key, int(low_pm), int(high_pm)
        self.speed, self.white, self.min_exposure, self.max_exposure = speed, white, min_exposure, max_exposure

    def replace(self, **over):
        new = Params.__new__(Params)
        new.__dict__.update(self.__dict__)
        new.__dict__.update(over)
        return new

    def __repr__(self):
        return "Params(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


def luminance(frame, mutant=None):
    frame = np.asarray(frame, dtype=f32)
    r, g, b = frame[..., 0], frame[..., 1], frame[..., 2]
    if mutant == "luminance_order":
        return f32(0.2126) * r + (f32(0.7152) * g + f32(0.0722) * b)
    return (f32(0.2126) * r + f32(0.7152) * g) + f32(0.0722) * b


def bins(y, mutant=None):
    shift = 21 if mutant == "shift_21" else 20
    b = ((np.ascontiguousarray(y, dtype=f32).view(np.uint32) & np.uint32(0x7fffffff)) >> np.uint32(shift)).astype(np.int64) - ((127 - 24) << 3)
    return np.clip(b, 0, 255)


def histogram(frame, mutant=None):
    n = np.bincount(bins(luminance(frame, mutant), mutant).ravel(), minlength=256).astype(np.uint32)
    if mutant != "bin0_metered":
        n[0] = 0
    return n


def centre(i, mutant=None):
    m = (i + 1) & 7 if mutant == "frac_shift" else i & 7
    return ((i >> 3) - 24) * 256 + FRAC[m]


def sums(n, low_pm, high_pm, mutant=None):
    """(S, M) of the counts between the trims, Python integers."""
    total = int(n.astype(np.int64).sum())
    lo, hi = total * low_pm // 1000, total * high_pm // 1000
    if mutant == "hi_inclusive":
        hi += 1
    c = s = m = 0
    for i in range(256):
        u = max(0, min(c + int(n[i]), hi) - max(c, lo))
        s += u * centre(i, mutant)
        m += u
        c += int(n[i])
    return s, m


def mean_q(s, m, mutant=None):
    num, den = 2 * s + m, 2 * m
    if mutant == "trunc_div" and num < 0:
        return -((-num) // den)
    return num // den


def target(q, p, mutant=None):
    a, f = divmod(-q, 256)
    v = f32(p.key) * EXP2[f]
    lo, hi = f32(p.min_exposure), f32(p.max_exposure)
    clamp = lambda x: lo if x < lo else (hi if x > hi else x)
    with np.errstate(over="ignore", under="ignore"):
        if mutant == "clamp_first":
            return f32(np.ldexp(clamp(v), a))
        return clamp(f32(np.ldexp(v, a)))


def exposure(frame, p, e_prev=None, mutant=None):
    """(histogram, e) of a metered frame."""
    n = histogram(frame, mutant)
    s, m = sums(n, p.low_pm, p.high_pm, mutant)
    if m == 0:
        return n, f32(1.0) if e_prev is None else f32(e_prev)
    e_t = target(mean_q(s, m, mutant), p, mutant)
    if e_prev is None:
        return n, e_t
    e_prev, speed = f32(e_prev), f32(p.speed)
    if mutant == "adapt_reversed":
        return n, f32(e_t + f32(speed * f32(e_prev - e_t)))
    return n, f32(e_prev + f32(speed * f32(e_t - e_prev)))


def curve(frame, e, p, mutant=None):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x = np.asarray(frame, dtype=f32) * f32(e)
        if p.operator == "linear":
            return x
        if p.operator == "reinhard":
            white = f32(p.white)
            w2 = white if mutant == "white_unsquared" else f32(white * white)
            return (x * (f32(1) + x / w2)) / (f32(1) + x)
        v = (x * (f32(2.51) * x + f32(0.03))) / (x * (f32(2.43) * x + f32(0.59)) + f32(0.14))
        return v if mutant == "aces_no_min" else np.fmin(v, f32(1))


def tone_map(frame, p, e_prev=None, mutant=None):
    """``(frame, histogram, exposure)`` of the definition, or of one of ``MUTANTS``."""
    assert mutant is None or mutant in MUTANTS, mutant
    frame = np.asarray(frame, dtype=f32)
    if p.exposure is not None:
        n, e = np.zeros(256, np.uint32), f32(p.exposure)
    else:
        n, e = exposure(frame, p, e_prev, mutant)
    out = curve(frame, e, p, mutant)
    assert out.dtype == f32
    return out, n, f32(e)
