"""Synthetic statement lists for the debug-frustum overlay: plain NumPy, no GPU, no library.

``frustums.OverlayOps`` only ever produces the lists of a frustum's edges: lines of a few hundred points with about
three distinct targets per point.  ``mr_scene_set_overlay`` accepts any lists that are well formed, and ``k_overlay``
(csrc/kernels_overlay.h) has code that lines never reach: segments longer than its LDS table serves, segments that
touch more pixels than the table may hold, a table probed around its end, thousands of bidders on one pixel.  ``make``
builds an ``OverlayOps`` from per-segment pixel lists, so ``OverlayOps.replay`` -- the statement-by-statement
restatement of upstream -- is the reference for them too; the generators below are the cases of
tests/test_overlay_lists_cpu.py and tests/test_overlay_lists_gpu.py."""
import numpy as np

from py_numpy_renderer_amd.frustums import OverlayOps

# csrc/kernels_overlay.h: OVERLAY_LDS_POINTS, OVERLAY_TABLE, OVERLAY_LDS_TARGETS (three quarters of the table),
# OVERLAY_MAX_SEGMENT
LDS_POINTS, TABLE, LDS_TARGETS, MAX_SEGMENT = 4096, 16384, 12288, 32768
LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 32768)
# depths() arguments under which a point passes against the z-buffer it was drawn from (z0 * (1 - u) * sign >= 0 with
# u >= 1 in the scenes of the tests, whose z has the sign of -sign; the tests check that the points are kept)
ALL_KEPT = dict(factor=(1.0, 1.4), background_finite=1.0)
BACKGROUND_FINITE = 0.6      # share of the points on background pixels (z = +-inf) that get a finite depth: see depths()


def make(height, width, segments):
    """An ``OverlayOps`` of the given segments, each a ``(rows, cols)`` pair of integer arrays (raw indices, as the
    line walk leaves them: -H <= row < H, -W <= col < W).  The centre wraps like a Python index and the neighbours are
    clipped from the raw index, exactly as in ``OverlayOps.__init__``; ``next`` is not built (the device does not
    take it)."""
    ops = OverlayOps.__new__(OverlayOps)
    ops.height, ops.width = int(height), int(width)
    segments = [(np.asarray(r, np.int64).ravel(), np.asarray(c, np.int64).ravel()) for r, c in segments]
    assert all(len(r) == len(c) > 0 for r, c in segments)
    row = np.concatenate([r for r, _ in segments])
    col = np.concatenate([c for _, c in segments])
    assert (row >= -height).all() and (row < height).all() and (col >= -width).all() and (col < width).all()
    ops.seg_count = np.asarray([len(r) for r, _ in segments], np.int32)
    ops.seg_first = (np.cumsum(ops.seg_count) - ops.seg_count).astype(np.int32)
    wrow, wcol = row % height, col % width
    sets = ((wrow, wcol), (np.clip(row - 1, 0, height - 1), wcol), (wrow, np.clip(col - 1, 0, width - 1)),
            (np.clip(row + 1, 0, height - 1), wcol), (wrow, np.clip(col + 1, 0, width - 1)))
    ops.target = np.ascontiguousarray(np.stack([r * width + c for r, c in sets]).astype(np.int32))
    ops.z = np.zeros(len(row), np.float64)
    ops.touched = np.unique(ops.target).astype(np.int32)
    return ops


def depths(ops, z0, rng, factor=(0.7, 1.4), background_finite=BACKGROUND_FINITE):
    """``z0[centre] * U(0.7, 1.4)`` per point: some points pass and some fail against the buffer, and later points on a
    pixel see what an earlier segment left there.  Where the buffer holds the background's infinity the product is
    infinite too, its difference with the buffer a NaN, and such a point is never kept (on the device as in NumPy); so
    BACKGROUND_FINITE of the points on the background take a finite depth of the same buffer instead and are drawn
    over it, as a line is -- of the points that follow on such a pixel, those pass or fail like any other.
    (*factor*, *background_finite*: for the one case that wants every point kept.)"""
    flat = np.asarray(z0, np.float64).reshape(-1)
    base = flat[ops.target[0]].copy()
    bad = ~np.isfinite(base) & (rng.uniform(size=len(base)) < background_finite)
    if bad.any():
        finite = flat[np.isfinite(flat)]
        base[bad] = rng.choice(finite, size=int(bad.sum())) if len(finite) else 1.0
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(base * rng.uniform(factor[0], factor[1], size=len(base)))


def with_depths(ops, z0, rng, **kw):
    ops.z = depths(ops, z0, rng, **kw)
    return ops


# --------------------------------------------------------------------------- what the kernel will do with a segment
def key_hash(pixel):
    """The LDS table's hash of a state index (csrc/kernels_overlay.h, k_overlay: ``key = X + 1``,
    ``hash = (key * 2654435761u) >> (32 - 14)``)."""
    return (((np.asarray(pixel, np.int64) + 1) * 2654435761) % (1 << 32)) >> 18


def distinct_targets(ops):
    """Distinct target pixels of every segment."""
    return np.asarray([len(np.unique(ops.target[:, f:f + n])) for f, n in zip(ops.seg_first, ops.seg_count)])


def takes_global_path(ops):
    """Per segment: True where the kernel keeps the bidding words in global memory -- the segment is longer than
    OVERLAY_LDS_POINTS, or touches more pixels than OVERLAY_LDS_TARGETS (host_overlay.h, mark_overlay_segments)."""
    return (ops.seg_count > LDS_POINTS) | (distinct_targets(ops) > LDS_TARGETS)


def kept(ops, z0, sign):
    """The replay's keep flag of every point (what phase A of the kernel computes), by replaying on a copy."""
    z = np.array(z0, np.float64).reshape(-1)
    f = np.zeros((z.size, 3), np.float32)
    keep = np.zeros(ops.n_points, bool)
    one = OverlayOps.__new__(OverlayOps)
    one.height, one.width = ops.height, ops.width
    with np.errstate(invalid="ignore"):             # (an infinite depth on the background: NaN >= 0 is False)
        for first, count in zip(ops.seg_first, ops.seg_count):
            sl = slice(first, first + count)
            keep[sl] = (z[ops.target[0, sl]] - ops.z[sl]) * sign >= 0
            one.seg_first, one.seg_count = np.asarray([0], np.int32), np.asarray([count], np.int32)
            one.target, one.z = ops.target[:, sl], ops.z[sl]
            one.replay(f, z, sign)
    return keep


def shared_pixels(ops, keep):
    """Pixels that kept points of two different target sets of ONE segment write."""
    n = 0
    for first, count in zip(ops.seg_first, ops.seg_count):
        k = keep[first:first + count]
        t = ops.target[:, first:first + count][:, k]
        sets = np.zeros(ops.height * ops.width, np.uint8)
        for j in range(5):
            np.bitwise_or.at(sets, t[j], np.uint8(1 << j))
        n += int(np.count_nonzero(sets & (sets - 1)))
    return n


# --------------------------------------------------------------------------- the cases
def _pixels(rng, height, width, n, pool=None):
    """n pixels drawn (with repeats) from the frame, or from a pool of *pool* of its pixels: the fewer pixels, the
    more points bid for each and the fewer entries the segment needs in the table."""
    if pool is None:
        lin = rng.integers(0, height * width, size=n)
    else:
        lin = rng.choice(rng.choice(height * width, size=pool, replace=False), size=n)
    return lin // width, lin % width


def segment_lengths(height, width, rng, lengths=LENGTHS, pair=4097):
    """Random pixels in segments of every length around the block size (1024 points per step), the LDS limit and the
    maximum.  Segments the LDS table serves (up to 4096 points, drawn from a pool of 2000 pixels: at most 10 000
    targets) alternate with segments that bid in global memory, as far as the lengths go round; two global segments
    over the same pixels stand back to back in the middle: the second must find the words the first left zero and
    the z it wrote."""
    short = [n for n in lengths if n <= LDS_POINTS]
    long_ = [n for n in lengths if n > LDS_POINTS]
    segments = []
    twice = _pixels(rng, height, width, pair)
    while short or long_:
        if short:
            segments.append(_pixels(rng, height, width, short.pop(0), pool=min(2000, height * width // 4)))
        if long_:
            segments.append(_pixels(rng, height, width, long_.pop(0)))
            if not long_:
                segments += [twice, (twice[0][::-1].copy(), twice[1][::-1].copy())]
    return make(height, width, segments)


def duplicates(height, width, rng, counts=(4097, 2000)):
    """Segments whose points all lie on the same 7 pixels of the top row: thousands of bidders per pixel, pixels that
    are one point's centre and another's neighbour (columns 0, 1, 2), both corners of the row (clipping makes a corner
    point its own row and column neighbour) and two pixels that share one neighbour (columns 60 and 62)."""
    cols = np.asarray([0, 1, 2, 60, 62, width - 2, width - 1])
    segments = []
    for n in counts:
        c = cols[rng.integers(0, len(cols), size=n)]
        segments.append((np.zeros(n, np.int64), c))
    return make(height, width, segments)


def plus_lattice(height, width):
    """(rows, cols) of the interior pixels with (row + 2 * col) % 5 == 0, row-major: their plus shapes (centre and four
    neighbours) tile the plane, so n points have 5 * n distinct targets."""
    r, c = np.mgrid[1:height - 1, 1:width - 1]
    on = (r + 2 * c) % 5 == 0
    return r[on], c[on]


def lattice_prefix():
    """Points of the longest prefix of the lattice with at most OVERLAY_LDS_TARGETS distinct targets."""
    return LDS_TARGETS // 5


def table_load(height, width, n_points=None):
    """The first *n_points* (None: all) of the plus lattice as ONE segment, between two short runs along a row (an LDS
    segment before and after it: the table must be empty again; neighbouring points of a run share pixels)."""
    r, c = plus_lattice(height, width)
    n = len(r) if n_points is None else n_points
    run = (np.full(65, height // 2), np.arange(10, 75))
    return make(height, width, [run, (r[:n], c[:n]), (run[0] + 1, run[1] + 1)])


def probe_wrap(height, width):
    """One segment around the pixels whose key hashes into the last 64 entries of the LDS table: each of them as a
    centre, then each of their neighbours as a centre, so that nearly every one of them is the target of SOME kept
    point and enters the table; there are more of them than entries from their hash to the table's end, so probes
    wrap to entry 0.  Returns (ops, number of such pixels)."""
    lin = np.arange(height * width)
    tail = lin[key_hash(lin) >= TABLE - 64]
    r, c = tail // width, tail % width
    rows = np.concatenate([r, np.clip(r - 1, 0, height - 1), r, np.clip(r + 1, 0, height - 1), r])
    cols = np.concatenate([c, c, np.clip(c - 1, 0, width - 1), c, np.clip(c + 1, 0, width - 1)])
    return make(height, width, [(rows, cols)]), len(tail)


def table_entries(ops, keep, segment):
    """Distinct pixels the kept points of a segment target: the entries it needs in the LDS table."""
    first, n = ops.seg_first[segment], ops.seg_count[segment]
    return len(np.unique(ops.target[:, first:first + n][:, keep[first:first + n]]))


def tail_entries(ops, keep):
    """Distinct pixels with a key hash in the table's last 64 entries that kept points of the first segment target."""
    n = ops.seg_count[0]
    t = np.unique(ops.target[:, :n][:, keep[:n]])
    return int(np.count_nonzero(key_hash(t) >= TABLE - 64))


def fewer_pixels(height, width, rng):
    """Lists that touch roughly two thirds of the frame, for a split frame that drew ``segment_lengths`` before: a
    4097-point segment (global memory) of random pixels, between LDS segments."""
    return make(height, width, [_pixels(rng, height, width, 300, pool=200), _pixels(rng, height, width, 4097),
                                _pixels(rng, height, width, 1025, pool=500)])


def cases(height, width, seed):
    """name -> lists (depths still zero: ``with_depths`` needs the z-buffer they are drawn on) of every case at this
    frame size."""
    rng = np.random.default_rng(seed)
    prefix = lattice_prefix()
    return {
        "segment_lengths": segment_lengths(height, width, rng),
        "duplicates": duplicates(height, width, rng),
        "table_at_limit": table_load(height, width, prefix),
        "table_at_limit_all_kept": table_load(height, width, prefix),     # (drawn with ALL_KEPT depths: the table three quarters full)
        "table_one_past_limit": table_load(height, width, prefix + 1),
        "table_overfull": table_load(height, width),
        "probe_wrap": probe_wrap(height, width)[0],
        "fewer_pixels": fewer_pixels(height, width, rng),
    }
