"""Synthetic fields for the post-frame kernels: plain NumPy, no GPU.

``k_ao``, ``k_dof``, ``k_accum_add`` and ``k_accum_resolve`` only ever see what a rendered scene hands them: z-buffers of a
cube or a statue, colours in [0, 1), widths that are multiples of 4.  ``mr_debug_post`` runs them on any buffers, so the
cases below show them what no camera produces: widths of every residue mod 4 with several workgroup columns, taps on the
halo's last ring, exact ties of ``rintf``, depth steps at the range's edge, single blurred samples ("beacons") whose circle
crosses workgroup borders, plateaus and signed zeroes of the circle of confusion, colours that are zero, denormal, huge,
infinite or NaN, every threshold of the finalise step function with the floats beside it, and a sum longer than
``k_accum_add``'s capped grid.  The references are ao_ref.py, dof_ref.py and accumulate_ref.py; the mirrors
(``mr_host_ao``, ``mr_host_dof``, ``mr_host_accum``) are held to them in tests/test_post_fields_cpu.py, and the kernels to the
mirrors in tests/test_post_fields_gpu.py.  The same CPU file checks that the cases have the properties they were made for
(``ao_row_split``, ``dof_r2``) and that they tell the mutants at the end of this file from the definitions."""
import math
from types import SimpleNamespace

import numpy as np

import accumulate_ref
import ao_ref
import dof_ref

F32 = np.float32
MOEBIUS = (-0.05, 0.001, -1.0, -0.0106)          # a real depth map: the float64 part of the eye depth is exercised
IDENTITY = (1.0, 0.0, 0.0, 1.0)                  # e = float32(Z): the depth field is given directly

# workgroup shapes as mr_debug_post numbers them (csrc/ao.hip, csrc/dof.hip)
AO_SHAPES = ((64, 64), (32, 32), (64, 16))       # (TW, TH) samples
DOF_TILES = (32, 32, 16)                         # square; shapes 0 and 1 differ in the threads per workgroup only
# (17, 129) .. (66, 132): every width residue mod 4 with two or more workgroup columns in every shape, a last column of 1, 2,
# 3 and 4 samples, partial rows of workgroups
AO_SIZES = ((5, 7), (1, 200), (200, 1), (17, 129), (33, 130), (65, 131), (66, 132))
DOF_SIZES = ((5, 7), (1, 100), (100, 1), (33, 65), (47, 49), (70, 101))
# k_accum_add's grid is capped at 2048 blocks of 256 lanes of 16 bytes (csrc/kernels_accum.h)
ACCUM_GRID_LANES = 2048 * 256
SUM_BIG = (70, 10001)                            # 2 100 210 floats: n4 = 525 052 lanes' worth, a second trip; a tail of 2

AO_SETTINGS = (dict(k=9.0, perspective=1), dict(k=70.0, perspective=1, radius=0.5, strength=3.0),
               dict(k=5.5, perspective=0, radius=0.2, bias=0.0), dict(k=0.25, perspective=1, strength=8.0, depth_range=10.0),
               dict(k=40.0, perspective=0, radius=0.5))          # rp: middling; up to the clamp; orthographic; 1 everywhere; 32 everywhere
DOF_SETTINGS = ((0.1, 1), (4.0, 1), (60.0, 1), (1.5, 0), (30.0, 0))              # (kf, perspective)
HILLS_FOCUS = 2.2

POISON = (0.0, -0.0, 1e-45, 1e-38, 1e38, np.inf)                 # zero, its negative, the smallest denormal, a denormal, huge, +inf


class Case:
    """One call of ``mr_debug_post``: *frames* ``(n, h, w, 3)`` float32, *z* ``(h, w)`` float64, the obscurance's and the
    depth of field's settings (dicts, or None), weights or None, shift and scale of the finalise."""

    def __init__(self, name, z, frames, ao=None, dof=None, weights=None, shift=0, scale=1.0):
        frames = np.ascontiguousarray(frames, dtype=F32)
        self.name, self.z = name, np.ascontiguousarray(z, dtype=np.float64)
        self.frames = frames[None] if frames.ndim == 3 else frames
        self.ao, self.dof, self.weights, self.shift, self.scale = ao, dof, weights, shift, scale
        assert self.frames.shape[1:3] == self.z.shape and (weights is not None or len(self.frames) == 1)

    @property
    def shape(self):
        return self.z.shape

    def __repr__(self):
        return f"Case({self.name!r})"


def ao_setting(m, k, perspective, **kw):
    return dict(m=m, k=k, perspective=perspective, **ao_ref.params(**kw))


def dof_setting(m, kf, perspective, focus):
    return dict(m=m, kf=kf, perspective=perspective, focus=focus)


# ---------------------------------------------------------------------------- depth fields
def z_of(depth, m):
    """The map's inverse: the Z whose eye depth is *depth*."""
    return (m[3] * depth - m[1]) / (m[0] - m[2] * depth)


def _holes(z, rng, shares):
    for share, value in zip(shares, (np.inf, -np.inf, np.nan)):
        z[rng.random(z.shape) < share] = value
    return z


def ao_hills(shape, seed, m=MOEBIUS):
    """(Z, F): smooth hills with steps, holes of +inf, -inf and NaN, uniform colours -- the synthetic field of
    test_ao_cpu.py at any size and under any map."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    depth = 2.0 + 0.4 * np.sin(xs / 3.1) * np.cos(ys / 2.3) + 0.3 * (rng.random(shape) < 0.2) + 0.05 * rng.random(shape)
    z = _holes(z_of(depth, m), rng, (0.1, 0.02, 0.02))
    return z, rng.random(shape + (3,), dtype=np.float32)


def dof_hills(shape, seed, m=MOEBIUS, focus=HILLS_FOCUS):
    """(Z, F): hills with steps across the plane in focus, a patch that lies in it, holes -- the synthetic field of
    test_dof_cpu.py at any size and under any map."""
    rng = np.random.default_rng(seed)
    h, w = shape
    ys, xs = np.mgrid[0:h, 0:w]
    depth = focus + 0.5 * np.sin(xs / 3.1) * np.cos(ys / 2.3) + 0.9 * (rng.random(shape) < 0.2) - 0.8 * (rng.random(shape) < 0.15)
    depth[h // 3:h // 3 + 5, w // 4:w // 4 + 6] = focus * (1 + 1e-4)
    z = _holes(z_of(depth, m), rng, (0.1, 0.03, 0.02))
    return z, rng.random(shape + (3,), dtype=np.float32)


def poisoned(frame, seed, share=0.003):
    """*frame* with each of POISON sprinkled over *share* of its floats."""
    rng = np.random.default_rng(seed)
    out = frame.copy()
    for value in POISON:
        out[rng.random(out.shape) < share] = F32(value)
    return out


def with_nans(frame, seed, share):
    out = frame.copy()
    out[np.random.default_rng(seed).random(out.shape) < share] = np.nan           # (quiet NaNs)
    return out


# ---------------------------------------------------------------------------- the obscurance's cases
def ao_cases():
    cases = []
    for i, shape in enumerate(AO_SIZES):
        for j, st in enumerate(AO_SETTINGS):
            m = MOEBIUS if (i + j) % 2 == 0 else IDENTITY
            z, frame = ao_hills(shape, 100 + i, m)
            cases.append(Case(f"ao hills {shape} k={st['k']} {'persp' if st['perspective'] else 'ortho'} {'moebius' if m is MOEBIUS else 'identity'}",
                              z, frame, ao=ao_setting(m, **st)))
    cases += ao_tie_cases() + [ao_range_case()]
    z, frame = ao_hills((65, 131), 120)
    cases.append(Case("ao poisoned colours (65, 131)", z, poisoned(frame, 121), ao=ao_setting(MOEBIUS, 9.0, 1)))
    # NaN colours are compared as NaN, not by their bits, so that the mirror keeps a background sample's colour while k_ao
    # multiplies it by 1.0f (which differs for a signalling NaN only) is not seen; the fields hold quiet NaNs
    z, frame = ao_hills((33, 130), 122)
    cases.append(Case("ao NaN colours (33, 130)", z, with_nans(frame, 123, 0.02), ao=ao_setting(MOEBIUS, 9.0, 1)))
    return cases


AO_TIE_K = (1.5, 2.5, 3.5, 30.5)


def ao_tie_cases():
    """Orthographic: rp = k at every sample, and the products with the taps (1, 0) and (0, 1) are exact halves."""
    z, frame = ao_hills((33, 130), 130, IDENTITY)
    return [Case(f"ao ties k={k}", z, frame, ao=ao_setting(IDENTITY, k, 0, radius=0.5)) for k in AO_TIE_K]


def ao_ties(case):
    """Products TAPS[i][j] * rp of the case's covered samples that lie exactly halfway between two integers."""
    st = case.ao
    e = ao_ref.eye_depth(case.z, st["m"])
    with np.errstate(all="ignore"):
        rp = (F32(st["k"]) / e) if st["perspective"] else np.full_like(e, F32(st["k"]))
    rp = np.minimum(np.maximum(rp, F32(1)), F32(ao_ref.MAX_RADIUS)).astype(F32)[np.isfinite(e)]
    prod = (ao_ref.TAPS.reshape(-1)[:, None] * rp[None, :]).astype(F32)
    return int((np.abs(prod - np.floor(prod)) == F32(0.5)).sum())


RANGE_LEVELS = (1.0, 3.0, float(np.nextafter(F32(3), F32(4))))      # steps of 0, of exactly 2, of nextafter(2, 3), and of one ulp


def ao_range_case():
    """Eye depths 1, 3 and the float after 3 under the identity map, depth_range 2: a pair is valid up to a step of exactly
    2 and not one float beyond."""
    rng = np.random.default_rng(140)
    shape = (17, 129)
    z = np.asarray(RANGE_LEVELS)[rng.integers(0, 3, shape)]
    return Case("ao range edge", z, rng.random(shape + (3,), dtype=np.float32),
                ao=ao_setting(IDENTITY, 3.0, 0, radius=4.0, strength=1.0, depth_range=2.0, bias=0.0))


def ao_range_steps(case):
    """(pairs of a sample and a tap at a step of exactly depth_range, pairs at the float after it)."""
    e = ao_ref.eye_depth(case.z, case.ao["m"])
    k = int(case.ao["k"])
    d = np.abs(e[:, k:] - e[:, :-k]).astype(F32)                   # the tap (1, 0) * k
    rng = F32(case.ao["depth_range"])
    return int((d == rng).sum()), int((d == np.nextafter(rng, F32(np.inf))).sum())


# ---------------------------------------------------------------------------- the depth of field's cases
FOCUS = 64.0                                     # identity map, orthographic, kf = 1: s = Z - 64
BEACON_COLOUR = (0.5, 0.25, 1.0)                 # powers of two: (w * F) / w == F for any w, the beacon keeps its bits
# c -> samples a single beacon changes: the lattice points within rr = max(min(c, 16) ** 2, 0.25) of it, itself not counted
BEACON_COUNTS = {0.4: 0, 0.5: 0, 0.75: 0, 1.0: 4, 1.41: 4, 1.42: 8, 2.0: 12, 3.0: 28, 15.99: 792, 16.0: 796, 40.0: 796}
# the sweep: with the table's, every loop bound 0 .. 16, and rr just below a perfect square
BEACON_SWEEP = tuple(BEACON_COUNTS) + tuple(float(b) for b in range(4, 16)) + (1.99, 2.99, 3.99, 8.99)
BEACON_FRAME = (40, 40)
BEACON_AT = (20, 20)
BEACON_BIG = (70, 101)
BEACON_PLACES = ((31, 31), (15, 15), (32, 32), (16, 16), (0, 0), (69, 100))      # last of workgroup (0, 0), first of (1, 1), corners


def beacon_case(shape, at, c, behind=False, seed=7):
    """Every sample in focus but one at ``focus - c`` (``+ c``: behind the plane), uniform colours round it."""
    z = np.full(shape, FOCUS)
    z[at] = FOCUS + c if behind else FOCUS - c
    frame = np.random.default_rng(seed).random(shape + (3,), dtype=np.float32)
    frame[at] = BEACON_COLOUR
    return Case(f"dof beacon {shape} at {at} c={c}{' behind' if behind else ''}", z, frame, dof=dof_setting(IDENTITY, 1.0, 0, FOCUS))


def beacon_disc(shape, at, c):
    """The samples the definition lets a foreground beacon change: inside the frame, within its rr, not itself."""
    s = F32(1.0) * F32(F32(FOCUS - c) - F32(FOCUS))                # kf * (e - focus), float32
    rr = dof_ref.squared_radius(np.asarray([[s]], dtype=F32))[0, 0]
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    d2 = (ys - at[0]) ** 2 + (xs - at[1]) ** 2
    return (d2.astype(F32) <= rr) & (d2 > 0)


def changed(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1)


def dof_beacon_cases():
    """[(case, expected mask of changed samples)]"""
    out = [(beacon_case(BEACON_FRAME, BEACON_AT, c), beacon_disc(BEACON_FRAME, BEACON_AT, c)) for c in BEACON_SWEEP]
    for at in BEACON_PLACES:
        out.append((beacon_case(BEACON_BIG, at, 16.0), beacon_disc(BEACON_BIG, at, 16.0)))
    for at in ((31, 31), (0, 0)):
        out.append((beacon_case(BEACON_BIG, at, 16.0, behind=True), np.zeros(BEACON_BIG, dtype=bool)))
    return out


# the cells a workgroup of k_dof parks its reduction in are the first of its halo's first row (csrc/kernels_dof.h): for the
# workgroups (1, 1) of 32 x 32 and (1, 1), (2, 2) of 16 x 16 samples these samples
PARKING = ((16, 16), (16, 17), (0, 0), (0, 1), (0, 3), (16, 19), (16, 31))


def dof_sparse_case(shape, seed):
    """Gentle hills round the plane in focus, about 2 % of the samples far in front of it with c from 0.5 to 20, the
    parking cells among them."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    z = FOCUS + 2.0 * np.sin(xs / 3.1) * np.cos(ys / 2.3)
    lit = rng.random(shape) < 0.02
    z[lit] = FOCUS - rng.uniform(0.5, 20.0, int(lit.sum()))
    for at in PARKING:
        if at[0] < shape[0] and at[1] < shape[1]:
            z[at] = FOCUS - 20.0
    return Case(f"dof sparse beacons {shape}", z, rng.random(shape + (3,), dtype=np.float32), dof=dof_setting(IDENTITY, 1.0, 0, FOCUS))


def dof_plateau_case():
    """Blocks of 6 x 6 samples of equal s: ``behind`` is false between equals."""
    rng = np.random.default_rng(160)
    shape = (47, 49)
    levels = np.asarray([-3.0, -1.5, 0.0, 2.0, 5.0])[rng.integers(0, 5, (8, 9))]
    z = FOCUS + np.kron(levels, np.ones((6, 6)))[:shape[0], :shape[1]]
    return Case("dof plateaus", z, rng.random(shape + (3,), dtype=np.float32), dof=dof_setting(IDENTITY, 1.0, 0, FOCUS))


def dof_signed_zero_case():
    """kf the smallest denormal: every product with a depth difference below one half rounds to a zero of that difference's
    sign, +0 beside -0."""
    rng = np.random.default_rng(161)
    shape = (33, 65)
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    z = FOCUS + 0.4 * np.sin(xs / 3.1) * np.cos(ys / 2.3)
    return Case("dof signed zeroes", z, rng.random(shape + (3,), dtype=np.float32), dof=dof_setting(IDENTITY, 1e-45, 0, FOCUS))


def dof_cases():
    """Everything but the beacons (dof_beacon_cases)."""
    cases = []
    for i, shape in enumerate(DOF_SIZES):
        for j, (kf, perspective) in enumerate(DOF_SETTINGS):
            m = MOEBIUS if (i + j) % 2 == 0 else IDENTITY
            z, frame = dof_hills(shape, 200 + i, m)
            cases.append(Case(f"dof hills {shape} kf={kf} {'persp' if perspective else 'ortho'} {'moebius' if m is MOEBIUS else 'identity'}",
                              z, frame, dof=dof_setting(m, kf, perspective, HILLS_FOCUS)))
    cases += [dof_sparse_case((70, 101), 150), dof_sparse_case((47, 49), 151), dof_plateau_case(), dof_signed_zero_case()]
    z, frame = dof_hills((47, 49), 220)
    cases.append(Case("dof poisoned colours (47, 49)", z, poisoned(frame, 221), dof=dof_setting(MOEBIUS, 4.0, 1, HILLS_FOCUS)))
    z, frame = dof_hills((33, 65), 222)
    cases.append(Case("dof NaN colours (33, 65)", z, with_nans(frame, 223, 0.005), dof=dof_setting(MOEBIUS, 4.0, 1, HILLS_FOCUS)))
    return cases


def composition_case():
    """The obscurance, then the depth of field, in one call."""
    z, frame = ao_hills((65, 131), 300)
    return Case("ao then dof (65, 131)", z, frame, ao=ao_setting(MOEBIUS, 9.0, 1), dof=dof_setting(MOEBIUS, 4.0, 1, 2.0))


def circle(case):
    st = case.dof
    return dof_ref.circle(case.z, st["m"], st["kf"], st["perspective"], st["focus"])


# ---------------------------------------------------------------------------- the sum's cases
SUM_SMALL = ((1, 1), (1, 2), (1, 3), (1, 4), (3, 3))             # 3, 6, 9, 12 and 27 floats: every n_floats % 4, and n4 == 0
SUM_WEIGHTS = (2.5, 1e-30, 0.75)                                  # above 1, tiny, ordinary


def sum_cases():
    rng = np.random.default_rng(400)
    return [Case(f"sum {shape}", np.zeros(shape), rng.random((3,) + shape + (3,), dtype=np.float32), weights=SUM_WEIGHTS, scale=0.3)
            for shape in SUM_SMALL]


def sum_big_case():
    rng = np.random.default_rng(401)
    return Case(f"sum {SUM_BIG}", np.zeros(SUM_BIG), rng.random((3,) + SUM_BIG + (3,), dtype=np.float32), weights=(0.5, 2.0, 1e-3), scale=0.4)


# ---------------------------------------------------------------------------- the step function's cases
STEP_EXTRAS = (0.0, 1e-45, float(np.nextafter(F32(1), F32(0))), 1.0, float(np.nextafter(F32(1), F32(2))), 2.0, 1e30, np.inf)


def _bytes_of(native, values):
    """The mirror's byte of every float32 in *values*: one frame, weight 1, scale 1."""
    v = np.ascontiguousarray(values, dtype=F32).ravel()
    pad = (-len(v)) % 3
    frame = np.concatenate([v, np.zeros(pad, F32)]).reshape(1, 1, -1, 3)
    return native.host_accum(frame, [1.0], shift=0, scale=1.0, want_acc=False)[1].reshape(-1)[:len(v)]


def step_thresholds(native):
    """For k = 1 .. 255 the smallest float32 the mirror finalises to k or more, by bisection over the bit patterns."""
    ks = np.arange(1, 256)
    lo = np.zeros(255, np.uint32)                                  # byte(0) = 0 < k <= 255 = byte(1)
    hi = np.full(255, F32(1.0).view(np.uint32), np.uint32)
    while (hi - lo > 1).any():
        mid = lo + (hi - lo) // 2
        up = _bytes_of(native, mid.view(F32)) >= ks
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    return hi.view(F32)


def step_values(native):
    """Each threshold with its two neighbours on either side, ascending, then STEP_EXTRAS."""
    bits = step_thresholds(native).view(np.uint32).astype(np.int64)
    around = (bits[:, None] + np.arange(-2, 3)[None, :]).astype(np.uint32).view(F32).reshape(-1)
    return np.concatenate([around, np.asarray(STEP_EXTRAS, dtype=F32)])


def step_cases(native):
    """The values as one row of samples, and as uniform 2 x 2 and 4 x 4 blocks for the block mean of shift 1 and 2.  The
    mean of a uniform block may lie a few floats off its value (((v + v) + v) + v rounds), so each shift has a second case
    whose blocks hold s * s * v in one sample and zeroes in the others: their mean is v exactly."""
    v = step_values(native)
    row = np.concatenate([v, np.zeros((-len(v)) % 3, F32)]).reshape(1, -1, 3)
    cases = [Case("steps shift 0", np.zeros(row.shape[:2]), row)]
    for shift in (1, 2):
        s = 1 << shift
        frame = np.repeat(np.repeat(row, s, axis=0), s, axis=1)
        cases.append(Case(f"steps shift {shift}", np.zeros(frame.shape[:2]), frame, shift=shift))
        alone = np.zeros_like(frame)
        alone[s - 1::s, 1::s] = row * F32(s * s)
        cases.append(Case(f"steps shift {shift}, one sample to a block", np.zeros(frame.shape[:2]), alone, shift=shift))
    return cases


# ---------------------------------------------------------------------------- a case through the reference, the mirror, the device
def _ao_desc(native, st):
    return native.fill_ao_desc(SimpleNamespace(**{n: st[n] for n in ("radius", "strength", "depth_range", "bias")}), st["m"], st["k"], st["perspective"])


def _dof_desc(native, st):
    return native.fill_dof_desc(st["m"], st["kf"], st["perspective"], st["focus"])


def reference(case, want_bytes=True):
    """(float frame, bytes) by ao_ref, dof_ref and accumulate_ref."""
    outs = []
    for f in case.frames:
        if case.ao:
            st = case.ao
            f = ao_ref.apply(case.z, f, st["m"], st["k"], st["perspective"], st["radius"], st["strength"], st["depth_range"], st["bias"])
        if case.dof:
            st = case.dof
            f = dof_ref.apply(case.z, f, st["m"], st["kf"], st["perspective"], st["focus"])
        outs.append(f)
    acc = outs[0] if case.weights is None else accumulate_ref.accumulate(outs, case.weights)
    with np.errstate(all="ignore"):
        return acc, accumulate_ref.finalise(acc, 1 << case.shift, case.scale) if want_bytes else None


def mirror(native, case):
    """(float frame, bytes) by mr_host_ao, mr_host_dof and mr_host_accum."""
    outs = []
    for f in case.frames:
        if case.ao:
            f = native.host_ao(case.z, f, _ao_desc(native, case.ao))
        if case.dof:
            f = native.host_dof(case.z, f, _dof_desc(native, case.dof))
        outs.append(f)
    if case.weights is None:
        return outs[0], native.host_accum(outs[0][None], [1.0], shift=case.shift, scale=case.scale, want_acc=False)[1]
    return native.host_accum(np.stack(outs), case.weights, shift=case.shift, scale=case.scale)


def device(native, handle, case, ao_shape=0, dof_shape=0):
    """(float frame, bytes) by mr_debug_post."""
    return native.debug_post(handle, case.frames, case.z, ao=_ao_desc(native, case.ao) if case.ao else None, ao_shape=ao_shape,
                             dof=_dof_desc(native, case.dof) if case.dof else None, dof_shape=dof_shape, weights=case.weights,
                             shift=case.shift, scale=case.scale)


def float_mismatches(got, want):
    """Floats of *got* that are not *want*'s: the same bits wherever *want* is not NaN, a NaN where it is.  Returns
    (mismatches, floats compared bit for bit, floats required to be NaN)."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
    return int(bad.sum()), int((~nan).sum()), int(nan.sum())


def byte_mask(acc, shift):
    """Output bytes whose whole block of *acc* is non-negative and not NaN, (h >> shift, w >> shift, 3), row 0 = top: the
    mirror's cast of anything else to uint8 is undefined."""
    s = 1 << shift
    ok = np.asarray(acc) >= 0
    h, w = ok.shape[0] // s, ok.shape[1] // s
    return ok.reshape(h, s, w, s, 3).all(axis=(1, 3))[::-1]


def byte_mismatches(got, want, acc, shift):
    """(mismatches, bytes compared) over byte_mask."""
    mask = byte_mask(acc, shift)
    assert got.shape == want.shape == mask.shape
    return int((got[mask] != want[mask]).sum()), int(mask.sum())


# ---------------------------------------------------------------------------- what the kernels will do with a case
def ao_row_split(height, width, tw):
    """k_ao step 3 (csrc/kernels_ao.h) for every row of every workgroup column: (x0, head, n4, tail) -- single floats in
    front of the first 16-byte boundary, 16-byte pieces, single floats behind them."""
    out = []
    for y in range(height):
        for x0 in range(0, width, tw):
            first = (y * width + x0) * 3
            nf = 3 * min(tw, width - x0)
            head = min((4 - (first & 3)) & 3, nf)
            n4 = (nf - head) >> 2
            out.append((x0, head, n4, nf - head - 4 * n4))
    return out


def dof_r2(s, tile, halo=True):
    """{(y0, x0): r2} per workgroup of tile x tile samples: the integer part of the largest rr among the samples it stages
    (its rectangle and, with *halo*, 16 samples round it), which bounds its gather (csrc/kernels_dof.h); the loop bound is
    ``math.isqrt(r2)``.  Computed as test_dof_gpu.py's lh_gl_digest does."""
    rr = dof_ref.squared_radius(np.asarray(s, dtype=F32))
    r = dof_ref.MAX_RADIUS if halo else 0
    return {(y0, x0): min(int(rr[max(y0 - r, 0):y0 + tile + r, max(x0 - r, 0):x0 + tile + r].max()), 256)
            for y0 in range(0, s.shape[0], tile) for x0 in range(0, s.shape[1], tile)}


def dof_r2_map(s, tile, halo=True):
    """dof_r2 per sample."""
    out = np.zeros(s.shape, dtype=np.int64)
    for (y0, x0), r2 in dof_r2(s, tile, halo).items():
        out[y0:y0 + tile, x0:x0 + tile] = r2
    return out


def dof_bounds(s, tile, halo=True):
    return {math.isqrt(r2) for r2 in dof_r2(s, tile, halo).values()}


# ---------------------------------------------------------------------------- the definitions with a hook each: the mutants
def dof_variant(s, frame, r2_limit=None, behind_ge=False):
    """dof_ref.apply_to_circle restated with two hooks.  Without them it is the definition (the CPU test holds it to
    dof_ref bit for bit).  *r2_limit* (per sample) skips the taps whose squared distance exceeds it, as a workgroup's loop
    bounds do: with dof_r2_map(s, tile) no bit changes, with dof_r2_map(s, tile, halo=False) the gather is bounded by the
    workgroup's own rectangle.  *behind_ge* tests ``behind`` with >=."""
    s, frame = np.asarray(s, dtype=F32), np.asarray(frame, dtype=F32)
    h, w = s.shape
    rr = dof_ref.squared_radius(s)
    W, S = np.zeros((h, w), dtype=F32), np.zeros((h, w, 3), dtype=F32)
    R = dof_ref.MAX_RADIUS
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            py = slice(max(0, -dy), min(h, h - dy))
            qy = slice(py.start + dy, py.stop + dy)
            if py.start >= py.stop:
                continue
            for dx in range(-R, R + 1):
                px = slice(max(0, -dx), min(w, w - dx))
                qx = slice(px.start + dx, px.stop + dx)
                if px.start >= px.stop:
                    continue
                s_p, s_q, rr_p, rr_q = s[py, px], s[qy, qx], rr[py, px], rr[qy, qx]
                behind = (s_q >= s_p) if behind_ge else (s_q > s_p)
                rr_t = np.where(behind, np.where(rr_p < rr_q, rr_p, rr_q), rr_q).astype(F32)
                passes = F32(dx * dx + dy * dy) <= rr_t
                if r2_limit is not None:
                    passes &= (dx * dx + dy * dy) <= r2_limit[py, px]
                if not passes.any():
                    continue
                wt = (F32(1) / rr_t).astype(F32)
                W[py, px] = np.where(passes, (W[py, px] + wt).astype(F32), W[py, px])
                term = (wt[..., None] * frame[qy, qx]).astype(F32)
                S[py, px] = np.where(passes[..., None], (S[py, px] + term).astype(F32), S[py, px])
        return (S / W[..., None]).astype(F32)


def rint_away(x):
    """Ties away from zero, where rintf takes them to even."""
    return (np.sign(x) * np.floor(np.abs(x) + F32(0.5))).astype(F32)


def ao_variant(z, frame, st, rint=np.rint, per_tap=False):
    """ao_ref.apply restated with two hooks.  Without them it is the definition (the CPU test holds it to ao_ref bit for
    bit).  *rint* rounds the taps' offsets; *per_tap* judges a pair tap by tap: a tap outside the range adds nothing, the
    other one still does."""
    frame = np.asarray(frame, dtype=F32)
    e = ao_ref.eye_depth(z, st["m"])
    h, w = e.shape
    covered = np.isfinite(e)
    k, rng, bias, strength = F32(st["k"]), F32(st["depth_range"]), F32(st["bias"]), F32(st["strength"])
    inv_fall = F32(1.0 / float(st["radius"]))
    with np.errstate(all="ignore"):
        rp = (k / e) if st["perspective"] else np.full_like(e, k)
        rp = np.where(rp > F32(1), rp, F32(1)).astype(F32)
        rp = np.where(rp < F32(ao_ref.MAX_RADIUS), rp, F32(ao_ref.MAX_RADIUS)).astype(F32)
        ys, xs = np.mgrid[0:h, 0:w]
        total = np.zeros((h, w), dtype=F32)
        for i in range(8):
            dx = rint((ao_ref.TAPS[i, 0] * rp).astype(F32)).astype(np.int64)
            dy = rint((ao_ref.TAPS[i, 1] * rp).astype(F32)).astype(np.int64)

            def tap(sx, sy):
                inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
                return np.where(inside, e[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], F32(np.inf)).astype(F32)
            a, b = tap(xs + dx, ys + dy), tap(xs - dx, ys - dy)
            da, db = (e - a).astype(F32), (e - b).astype(F32)
            va, vb = covered & np.isfinite(a) & (np.abs(da) <= rng), covered & np.isfinite(b) & (np.abs(db) <= rng)
            if per_tap:
                valid = va | vb
                c = (np.where(va, da, F32(0)) + np.where(vb, db, F32(0))).astype(F32)
            else:
                valid = va & vb
                c = (da + db).astype(F32)
            t = ((c - bias).astype(F32) * inv_fall).astype(F32)
            occ = np.where(t < 0, F32(0), np.where(t > 1, F32(1), t)).astype(F32)
            total = (total + np.where(valid, occ, F32(0)).astype(F32)).astype(F32)
        ao = (F32(1) - (strength * (total * F32(0.125)).astype(F32)).astype(F32)).astype(F32)
        ao = np.where(ao < 0, F32(0), ao).astype(F32)
        return np.where(covered[..., None], (frame * ao[..., None]).astype(F32), frame).astype(F32)


def step_off_by_one(native, acc):
    """A step function whose thresholds lie one float too high: the byte of the float before each value."""
    acc = np.asarray(acc, dtype=F32)
    return _bytes_of(native, np.where(acc > 0, np.nextafter(acc, F32(0)), acc)).reshape(acc.shape)[::-1]


def sum_one_trip(frames, weights):
    """A sum whose grid-stride loop takes one trip: the 16-byte pieces past the capped grid's lanes are never written and
    keep the 0xFF bytes the buffer was filled with."""
    acc = accumulate_ref.accumulate(frames, weights)
    flat = acc.reshape(-1).copy()
    flat[4 * ACCUM_GRID_LANES:4 * (len(flat) // 4)] = np.uint32(0xFFFFFFFF).view(F32)
    return flat.reshape(acc.shape)
