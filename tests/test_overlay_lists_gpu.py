"""k_overlay (csrc/kernels_overlay.h) held to the statement replay on synthetic lists (tests/overlay_lists.py).

The camera-built lists of the other overlay tests are lines: a few hundred points a segment, about three distinct
targets per point.  They never reach the kernel's global-memory half (segments of more than 4096 points, or of more
pixels than its LDS table may hold), the scratch that half needs, the table's wrap-around and its load limit, or a
pixel with thousands of bidders.  The explicit-lists entry (``mr_scene_set_overlay``) takes any well-formed lists, and
``OverlayOps.replay`` -- the statement-by-statement restatement of upstream -- says exactly what they must draw on the
device's own z-buffer and float frame: z and the float frame bit for bit, no tolerance."""
import numpy as np
import pytest

import overlay_lists as ol
import scenes
from supersample_ref import resolve

pytestmark = pytest.mark.gpu

SCENES = {"cube_small": lambda api: scenes.cube_small(api),                                   # 120 x 160, RH: sign +1
          "diablo_floor_lh_gl": lambda api: scenes.diablo_floor_lh_gl(api, resolution=(136, 152))}    # LH: sign -1, no multiple of 16


class Base:
    """A scene rendered once without the overlay: the buffers the overlay is then drawn on, as the device left them."""

    def __init__(self, scene):
        self.scene, self.backend = scene, scene._backend()
        self.sign = int(scene.system)
        self.plain = self.backend.render(scene, counters=True, keep_float=True).copy()
        self.z0, self.f0 = self.backend.read_z().copy(), self.backend.read_frame_f32().copy()
        self.height, self.width = self.z0.shape


@pytest.fixture(scope="module", params=list(SCENES))
def base(request, api):
    b = Base(SCENES[request.param](api))
    yield b
    b.scene.close()


@pytest.fixture(scope="module")
def base2(api):
    scene = scenes.cube_small(api)
    scene.supersample = 2
    b = Base(scene)
    assert b.z0.shape == (240, 320)
    yield b
    b.scene.close()


def meaningful(b, ops, shared=True):
    """Conditions on the INPUTS (never on the kernel) under which a case tests something; returns the keep flags.
    Both scenes leave most of the frame at the background's infinite z (all but 94 pixels of the LH one), so "a finite
    z at every centre" cannot be asked of lists that cover the frame: the depth is finite wherever the centre's z is,
    never a NaN, and overlay_lists.depths gives six in ten of the points on the background a finite depth of their own."""
    centre = b.z0.reshape(-1)[ops.target[0]]
    assert not np.isnan(ops.z).any() and np.isfinite(ops.z[np.isfinite(centre)]).all()
    keep = ol.kept(ops, b.z0, b.sign)
    assert 0.2 <= keep.mean() <= 0.8, keep.mean()
    if shared:
        assert ol.shared_pixels(ops, keep) >= 1
    return keep


def reference(b, ops):
    za, fa = b.z0.copy(), b.f0.copy()
    with np.errstate(invalid="ignore"):             # (an infinite depth on the background: NaN >= 0 is False, here as there)
        ops.replay(fa, za, b.sign)
    assert (za.view(np.uint64) != b.z0.view(np.uint64)).any() and (fa.view(np.uint32) != b.f0.view(np.uint32)).any()
    return za, fa


def draw_and_compare(b, ops, ss=1):
    """Draws *ops* on the base frame and holds z, the float frame and the uint8 frame to the replay."""
    za, fa = reference(b, ops)
    b.backend.set_overlay_lists(ops)
    out = b.backend.render(b.scene, counters=True, keep_float=True, overlay=True).copy()
    z, f = b.backend.read_z(), b.backend.read_frame_f32()
    bad = z.view(np.uint64) != za.view(np.uint64)
    assert not bad.any(), f"z: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0]}"
    bad = (f.view(np.uint32) != fa.view(np.uint32)).any(axis=-1)
    assert not bad.any(), f"float frame: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0]}"
    want = resolve(fa, ss) if ss > 1 else (fa[::-1] ** 0.8 * 255).astype(np.uint8)
    assert out.shape == want.shape
    assert np.abs(out.astype(np.int16) - want.astype(np.int16)).max() <= 1
    untouched = np.ones(b.height * b.width, bool)
    untouched[ops.touched] = False
    untouched = untouched.reshape(b.height // ss, ss, b.width // ss, ss).all(axis=(1, 3))[::-1]
    assert untouched.any() or len(ops.touched) > b.height * b.width * 0.9
    assert np.array_equal(out[untouched], b.plain[untouched]), "a pixel outside the lists' targets changed"
    # the frame-only render: taps written only for the tiles of the lists' tile mask
    only = b.backend.render(b.scene, counters=False, keep_buffers=False, overlay=True)
    assert np.array_equal(only, out)
    return out


def test_segment_lengths(base):
    """Segments of 1 ... 32768 points, LDS and global-memory segments in turn, two global ones back to back."""
    ops = ol.segment_lengths(base.height, base.width, np.random.default_rng(101))
    ol.with_depths(ops, base.z0, np.random.default_rng(102))
    assert sorted(ops.seg_count.tolist()) == sorted(ol.LENGTHS + (4097, 4097))
    path = ol.takes_global_path(ops)
    assert np.array_equal(path, ops.seg_count > ol.LDS_POINTS)         # (the short ones fit the table)
    assert (path[:-1] != path[1:]).sum() >= 6 and (path[:-1] & path[1:]).any()      # in turn; two global ones back to back
    meaningful(base, ops)
    draw_and_compare(base, ops)


def test_duplicates(base):
    """4097 and 2000 points on the same 7 pixels: the last kept writer of thousands wins, corners included."""
    ops = ol.duplicates(base.height, base.width, np.random.default_rng(111))
    ol.with_depths(ops, base.z0, np.random.default_rng(112))
    assert len(np.unique(ops.target[0])) == 7 and ops.seg_count.tolist() == [4097, 2000]
    assert (ops.target[0] == ops.target[1]).any() and (ops.target[0] == ops.target[2]).any()      # a corner: its own neighbour
    assert np.isin(ops.target[0], ops.target[2]).any()                  # a centre that is another point's neighbour
    meaningful(base, ops)
    draw_and_compare(base, ops)


@pytest.mark.parametrize("case", ["table_at_limit", "table_at_limit_all_kept", "table_one_past_limit", "table_overfull"])
def test_table_load(base, case):
    """The plus lattice, whose n points have 5 n distinct targets, as one segment: the longest prefix the LDS table takes
    (12 285 pixels), one point more (over the limit: global memory), and the whole lattice, which has more targets than
    the table has entries and must be drawn all the same."""
    ops = ol.cases(base.height, base.width, 0)[case]
    all_kept = case.endswith("all_kept")
    ol.with_depths(ops, base.z0, np.random.default_rng(122), **(ol.ALL_KEPT if all_kept else {}))
    n, distinct, path = int(ops.seg_count[1]), ol.distinct_targets(ops), ol.takes_global_path(ops)
    assert distinct[1] == 5 * n and not path[0] and not path[2]
    if case.startswith("table_at_limit"):
        assert n == 2457 and not path[1] and ol.LDS_TARGETS - 5 < distinct[1] <= ol.LDS_TARGETS
    elif case == "table_one_past_limit":
        assert n == 2458 and path[1] and n <= ol.LDS_POINTS
    else:
        assert n == {(120, 160): 3729, (136, 152): 4020}[(base.height, base.width)]
        assert path[1] and n <= ol.LDS_POINTS and distinct[1] > ol.TABLE
    if all_kept:
        # the table as full as it gets: the targets of the prefix are entries, but for some of the points around the run
        # that was drawn before them (which left its own z there)
        keep = ol.kept(ops, base.z0, base.sign)
        assert 12000 <= ol.table_entries(ops, keep, 1) <= ol.LDS_TARGETS
    else:
        meaningful(base, ops)
    draw_and_compare(base, ops)


def test_probe_wrap(base):
    """More kept targets with a key hash in the table's last 64 entries than entries there: probes wrap to entry 0."""
    ops, count = ol.probe_wrap(base.height, base.width)
    ol.with_depths(ops, base.z0, np.random.default_rng(132))
    # csrc/kernels_overlay.h, k_overlay: key = X + 1; hash = (key * 2654435761u) >> (32 - 14)
    lin = np.arange(base.height * base.width, dtype=np.uint64)
    tail = ((lin + 1) * 2654435761 % 2 ** 32) >> 18 >= 16384 - 64
    assert count == tail.sum() > 64 and np.array_equal(np.unique(ops.target[0][:count]), np.nonzero(tail)[0])
    if (base.height, base.width) == (120, 160):
        assert count == 75
    keep = meaningful(base, ops)
    assert not ol.takes_global_path(ops).any() and ol.tail_entries(ops, keep) > 64
    draw_and_compare(base, ops)


def test_supersampled(base2):
    """Lists on the 240 x 320 sample grid of a frame with supersample = 2: the kernel leaves the uint8 frame to
    k_resolve_touched, which finalises the output pixels of the explicit lists' touched samples."""
    ops = ol.segment_lengths(base2.height, base2.width, np.random.default_rng(141), lengths=(1, 64, 65, 1025, 4096, 4097, 8192))
    ol.with_depths(ops, base2.z0, np.random.default_rng(142))
    path = ol.takes_global_path(ops)
    assert np.array_equal(path, ops.seg_count > ol.LDS_POINTS) and path.any() and not path.all()
    meaningful(base2, ops)
    draw_and_compare(base2, ops, ss=2)


def _split_frame(b, ops, world=2):
    """tests/test_overlay.py, test_split_frame_with_overlay_equals_the_single_device_frame, with explicit lists: one GPU
    plays *world* equal bands in turn; returns (assembled frame after mr_overlay_apply, single-device frame, slots)."""
    import torch
    from py_numpy_renderer_amd.multigpu import row_band
    backend, scene, h, w = b.backend, b.scene, b.height, b.width
    backend.set_overlay_lists(ops)
    want = backend.render(scene, counters=False, keep_buffers=False, overlay=True).copy()
    rows_bytes = h // world * w * 3
    offset = -(-rows_bytes // 16) * 16
    n_slots = backend.overlay_state_bytes() // 24
    part_bytes = offset + -(-n_slots * 24 // 16) * 16
    gathered = torch.zeros(world * part_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for r in range(world):
        backend.render_device(scene, gathered.data_ptr() + r * part_bytes, 0, shadows=True, no_timing=True, overlay=True,
                              row_band=row_band(h, r, world))
    assert not backend.overflowed()                       # (synchronises)
    frame = gathered.view(world, part_bytes)[:, :rows_bytes].contiguous().view(h, w, 3).clone()
    torch.cuda.synchronize()
    backend.overlay_apply(gathered.data_ptr(), part_bytes, offset, world, False, int(scene.system), frame.data_ptr(), 0)
    backend.overflowed()
    return frame.cpu().numpy(), want, n_slots


def test_split_frame_lists_changing(base):
    """mr_overlay_apply carves z | colour | win | any out of one buffer at offsets that depend on the number of touched
    pixels.  Lists A touch nearly every pixel; lists B, drawn next on the same scene and stream, touch fewer, so that
    their bidding words lie where A kept float colours: unless they are cleared, no bidder of B's 4097-point segment
    (global memory: the only path that reads those words) wins, and the segment is not drawn."""
    a = ol.with_depths(ol.segment_lengths(base.height, base.width, np.random.default_rng(151)), base.z0, np.random.default_rng(152))
    b = ol.with_depths(ol.fewer_pixels(base.height, base.width, np.random.default_rng(153)), base.z0, np.random.default_rng(154))
    assert 4097 in b.seg_count.tolist()
    meaningful(base, a), meaningful(base, b)
    got_a, want_a, slots_a = _split_frame(base, a)
    assert slots_a == len(a.touched) and (want_a != base.plain).any()
    assert np.array_equal(got_a, want_a)
    got_b, want_b, slots_b = _split_frame(base, b)
    assert slots_b == len(b.touched) and 0.4 * slots_a < slots_b < slots_a
    assert (want_b != base.plain).any() and (want_b != want_a).any()
    bad = (got_b != want_b).any(axis=-1)
    assert not bad.any(), f"lists B on the assembled frame: {int(bad.sum())} pixels differ from the single-device frame"


def test_validation(base):
    """What mr_scene_set_overlay refuses (nothing is rendered), and the longest segment it accepts."""
    h, w, backend = base.height, base.width, base.backend
    rng = np.random.default_rng(161)

    def lists(*counts):
        return ol.make(h, w, [ol._pixels(rng, h, w, n) for n in counts])

    def refused(ops, reason):
        with pytest.raises(RuntimeError, match=reason):
            backend.set_overlay_lists(ops)

    refused(lists(10, 32769), "segment longer than")
    ops = lists(100, 100)
    ops.seg_first = ops.seg_first.copy()
    ops.seg_first[1] = 99
    refused(ops, "segments must follow each other")                  # overlap
    ops.seg_first[1] = 101
    refused(ops, "segments must follow each other")                  # gap
    ops = lists(100)
    ops.target[3, 17] = -1
    refused(ops, "negative overlay target")
    ops = lists(100)
    ops.target[4, 99] = h * w
    refused(ops, "targets outside")
    ops = lists(100)
    ops.width = 32768
    refused(ops, "bad frame size")
    backend.set_overlay_lists(lists(5, 32768))
