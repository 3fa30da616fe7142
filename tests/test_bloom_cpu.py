"""CPU: the bloom's host mirror ``mr_host_bloom`` against the NumPy restatement bloom_ref.py, bit for bit, frame and pyramid,
on every field of bloom_fields.py; the consequences csrc/bloom_def.h states; the mutants of the definition, each told apart
by some field; what the library and the Python layer refuse; the packer's gain and level rule.  No device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import bloom_fields as bf
import bloom_ref
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = bf.cases()


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    _native.load_library()
    return _native


# ---------------------------------------------------------------------------- 1. the mirror is the definition
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_mirror_is_the_reference_on_every_field(native, case):
    changed = 0
    for levels in sorted(set(bf.LEVELS + (case.levels, 6))):
        at = case.at(levels)
        want, got = at.reference(), at.mirror(native)
        assert [d.shape for d in got[1]] == [d.shape for d in want[1]], f"{at!r}: the level sizes"
        frame, pyramid = bf.all_bits(got, want)
        assert frame == 0 and pyramid == 0, f"{at!r}: {frame} floats of the frame and {pyramid} of the pyramid are not the reference's"
        assert got[2][-1] is got[1][-1] or bf.bits(got[2][-1], got[1][-1]) == 0
        changed += bf.bits(got[0], at.frame)
    assert changed > 0 or case.name == "below the threshold", f"{case!r}: no float changed: the mirror was shown nothing"


def test_the_pyramid_is_packed_as_the_header_states(native):
    case = bf.Case("packing", bf.seeded((11, 6)), levels=3)
    sizes = native.bloom_levels(11, 6, 3)
    assert sizes == [(6, 3), (3, 2), (2, 1)]
    n = [h * w * 3 for h, w in sizes]
    flat = np.full(2 * sum(n) - n[-1] + 2, -3.0, np.float32)
    out = np.empty_like(case.frame)
    lib = native.load_library()
    assert lib.mr_host_bloom(case.frame.ctypes.data, 11, 6, C.byref(case.desc(native)), out.ctypes.data, flat[1:].ctypes.data) == 0
    assert flat[0] == -3.0 and flat[-1] == -3.0, "the float count the header states"
    _, D, U = case.reference()
    order = [D[0], D[1], D[2], U[1], U[0]]                 # D_1 .. D_L, then U_{L-1} .. U_1
    assert bf.bits(flat[1:-1], np.concatenate([a.ravel() for a in order])) == 0


def test_the_fields_cover_what_they_are_named_for():
    shapes = {c.shape for c in CASES}
    assert set(bf.SMALL_SIZES) <= shapes and {(1, 1), (1, 2), (2, 3), (3, 5), (17, 33), (130, 9)} == set(bf.SMALL_SIZES)
    for tw, th in bf.BLOOM_TILES:
        for a in (-1, 1):
            for b in (-1, 1):
                h, w = 2 * th + a, 2 * tw + b
                assert (h, w) in shapes
                # level 0 holds more than one workgroup's source rectangle; level 1 straddles a workgroup's edge or fills it
                assert (h + 1) // 2 in (th, th + 1) and (w + 1) // 2 in (tw, tw + 1)
    out = next(c for c in CASES if c.name == "levels run out")
    sizes = bloom_ref.level_sizes(*out.shape, out.levels)
    assert sizes.count((1, 1)) >= 2, "1 x 1 halves to 1 x 1 before the levels are used up"
    for c in CASES:
        assert c.frame.min() >= 0 and c.frame.max() <= 1 and np.isfinite(c.frame).all()
        if c.name.startswith("seeded") and c.frame.size > 3:
            assert (bloom_ref.bright(c.frame, c.threshold) > 0).any(), f"{c!r}: nothing is bright"


# ---------------------------------------------------------------------------- 2. the stated consequences
@pytest.mark.parametrize("levels", [1, 4, 8])
def test_below_the_threshold_the_frame_is_untouched(native, levels):
    case = bf.below().at(levels)
    assert case.frame.max() <= case.threshold
    out, D, U = case.mirror(native)
    assert bf.bits(out, case.frame) == 0
    for level in D + U:
        assert not level.view(np.uint32).any(), "every level is +0"


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (21, 38), (130, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_uniform_field_glows_by_the_iterated_sum(native, size, levels):
    case = bf.uniform(size, levels)
    out, D, U = case.mirror(native)
    b = np.float32(0.375)
    total = b
    for l in range(levels - 1, -1, -1):                  # U_L = b; U_l = b + U_{l+1}
        assert (D[l] == b).all() and (U[l] == total).all(), f"level {l + 1}"
        if l:
            total = np.float32(b + total)
    want = np.float32(np.float32(0.75) + bloom_ref.gain(case.intensity, levels) * total)
    assert (out == want).all() and out.shape == case.frame.shape


@pytest.mark.parametrize("at", bf.MASS_AT, ids=lambda a: f"{a[0]}-{a[1]}")
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_the_interior_conserves_mass(native, levels, at):
    """One sample whose bright value is a power of two in every channel, at places of either parity.  (The sum is exact
    because every partial sum of the chain then fits float32; at three levels a bright value with more mantissa bits, or
    a place such as (49, 50) whose taps meet the finest unit and the largest value in one sample, rounds once somewhere:
    the mass is then L times the bright value to within that rounding, and the test does not claim more.)

    The glow is g * up(U_1) with g = 1 here.  Its sum is taken from up(U_1) itself, formed from the mirror's own U_1: at
    three levels the glow's unit is 2^-32, and at the bright sample the composite's one rounding of F + glow (F's unit is
    2^-24 there) would be in the sum of out - F.  That out is F + up(U_1), rounded once, is asserted beside it."""
    case = bf.mass(levels, at)
    out, D, U = case.mirror(native)
    assert float(bloom_ref.gain(case.intensity, levels)) == 1.0
    glow32 = bloom_ref.up(U[0], bf.MASS_SIZE)
    assert bf.bits(out, case.frame + glow32) == 0
    glow = glow32.astype(np.float64)
    if levels <= 2:
        assert (out.astype(np.float64) - case.frame.astype(np.float64) == glow).all(), "at two levels the composite is exact too"
    b0 = bloom_ref.bright(case.frame, case.threshold)[at].astype(np.float64)
    assert (b0 == (0.5, 0.25, 0.125)).all()
    border = np.ones(bf.MASS_SIZE, bool)
    border[8:-8, 8:-8] = False
    assert not glow[border].any(), "the glow reaches the border: the field is too small for the claim"
    assert (glow.sum(axis=(0, 1)) == levels * b0).all(), (glow.sum(axis=(0, 1)), levels * b0)
    for l, level in enumerate(D):                        # every level down holds a quarter of the samples and the same mean
        assert (level.astype(np.float64).sum(axis=(0, 1)) * 4.0 ** (l + 1) == b0).all(), f"D_{l + 1}"


def test_every_level_is_finite_at_the_extremes(native):
    frame = bf.seeded((9, 14))
    frame[3, 4] = (1.0, 1.0, 1.0)
    frame[5, 5] = (np.float32(1e-38), 0.0, 0.0)           # a bright sample next to nothing: (m - t) / m with the smallest m
    for t in (0.0, 1e-45, 0.99999994):
        out, D, U = native.host_bloom(frame, native.fill_bloom_desc(t, 1.0, 8), pyramid=True)
        assert all(np.isfinite(a).all() for a in [out] + D + U), t


# ---------------------------------------------------------------------------- 3. the mutants
@pytest.mark.parametrize("mutant", bloom_ref.MUTANTS)
def test_every_mutant_is_told_apart_by_some_field(native, mutant):
    caught = []
    for case in CASES:
        want, wrong = case.reference(), case.reference(mutant=mutant)
        sizes_differ = [d.shape for d in wrong[1]] != [d.shape for d in want[1]]
        if sizes_differ or bf.bits(wrong[0], want[0]):
            caught.append(case.name)
            if not sizes_differ:                         # ... and the mirror stands with the definition
                assert bf.bits(case.mirror(native)[0], want[0]) == 0
    print(f"{mutant}: told apart by {len(caught)} of {len(CASES)} fields: {caught[:6]}")
    assert caught, f"no field tells {mutant} from the definition"


# ---------------------------------------------------------------------------- 4. refusals and bindings, no device
def test_symbols_are_bound(native):
    lib = native.load_library()
    for name in ("mr_scene_set_bloom", "mr_host_bloom", "mr_debug_bloom", "mr_debug_bloom_times", "mr_debug_bloom_post"):
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert C.sizeof(native.BloomDesc) == 8 + 8 + 4 + 4
    header = open(os.path.join(ROOT, "include", "mi355rast.h")).read()
    body = header.split("typedef struct mr_bloom_desc")[1].split("} mr_bloom_desc;")[0]
    for line in ("double threshold;", "double gain;", "int32_t levels;"):
        assert line in body
    assert "#define MR_ABI_VERSION 4" in header and lib.mr_abi_version() == 4


def test_the_library_checks_the_description(native):
    lib = native.load_library()
    handle = lib.mr_scene_create()
    nan, inf = float("nan"), float("inf")
    desc = lambda t=0.8, g=0.125, n=4: C.byref(native.fill_bloom_desc(t, g, n))
    assert lib.mr_scene_set_bloom(None, desc()) == native.MR_E_INVALID
    assert lib.mr_scene_set_bloom(handle, None) == 0                       # off, on a scene that never had it
    assert lib.mr_scene_set_bloom(handle, desc()) == 0, lib.mr_last_error()          # (copied: no device is touched)
    for word, over in (("levels", dict(n=0)), ("levels", dict(n=9)), ("levels", dict(n=-1)), ("threshold", dict(t=nan)), ("threshold", dict(t=inf)),
                       ("threshold", dict(t=-0.5)), ("threshold", dict(t=1e39)), ("gain", dict(g=0.0)), ("gain", dict(g=nan)), ("gain", dict(g=-1.0)),
                       ("gain", dict(g=1e-46)), ("gain", dict(g=inf))):
        assert lib.mr_scene_set_bloom(handle, desc(**over)) == native.MR_E_INVALID, over
        assert word.encode() in lib.mr_last_error(), (over, lib.mr_last_error())
    for ok in (dict(t=0.0), dict(n=1), dict(n=8), dict(t=5.0)):
        assert lib.mr_scene_set_bloom(handle, desc(**ok)) == 0, ok
    out = np.zeros(4, np.int32)
    assert lib.mr_debug_bloom(handle, out.ctypes.data) == 0 and out.tolist() == [0] * 4
    assert lib.mr_debug_bloom(handle, None) == native.MR_E_INVALID
    ms = (C.c_float * 3)()
    assert lib.mr_debug_bloom_times(handle, ms) == native.MR_E_INVALID and b"no frame with bloom yet" in lib.mr_last_error()
    # a split frame is refused before any device work
    fr = native.FrameDesc()
    fr.width, fr.height, fr.system, fr.row_begin, fr.row_end = 8, 8, 1, 0, 4
    rgb = np.zeros((8, 8, 3), np.uint8)
    assert lib.mr_render(handle, C.byref(fr), rgb.ctypes.data, None) == native.MR_E_INVALID
    assert b"bloom takes whole frames" in lib.mr_last_error()
    fr.row_end, fr.stripe_count, fr.stripe_index = 8, 2, 0
    assert lib.mr_render_async(handle, C.byref(fr), rgb.ctypes.data, 0) == native.MR_E_INVALID
    assert b"bloom takes whole frames" in lib.mr_last_error()
    lib.mr_scene_destroy(handle)


def test_the_mirror_and_the_debug_entry_check_their_arguments(native):
    lib = native.load_library()
    f, out = np.ones((4, 4, 3), np.float32), np.empty((4, 4, 3), np.float32)
    good = native.fill_bloom_desc(0.5, 0.25, 2)
    args = lambda **o: [o.get("f", f.ctypes.data), o.get("h", 4), o.get("w", 4), o.get("d", C.byref(good)), o.get("out", out.ctypes.data), None]
    assert lib.mr_host_bloom(*args()) == 0                    # (no pyramid is asked for: not an error)
    bad = lambda **o: C.byref(native.fill_bloom_desc(o.get("t", 0.5), o.get("g", 0.25), o.get("n", 2)))
    for over in (dict(f=None), dict(out=None), dict(d=None), dict(h=0), dict(w=-1), dict(h=40000), dict(out=f.ctypes.data), dict(d=bad(n=0)),
                 dict(d=bad(n=9)), dict(d=bad(t=float("nan"))), dict(d=bad(t=float("inf"))), dict(d=bad(g=0.0))):
        assert lib.mr_host_bloom(*args(**over)) == native.MR_E_INVALID, over
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        native.host_bloom(f[..., :2], good)
    with pytest.raises(ValueError, match="levels"):
        native.host_bloom(f, native.fill_bloom_desc(0.5, 0.25, 9))
    # mr_debug_bloom_post refuses before it asks for a device
    handle = lib.mr_scene_create()
    for over, word in ((dict(shape=3), "shape"), (dict(shape=-1), "shape"), (dict(n=0), "levels"), (dict(n=9), "levels"), (dict(t=float("nan")), "threshold")):
        with pytest.raises(ValueError, match=word):
            native.debug_bloom_post(handle, f, native.fill_bloom_desc(over.get("t", 0.5), 0.25, over.get("n", 2)), over.get("shape", 0))
    post = lambda *a: lib.mr_debug_bloom_post(*a)
    assert post(handle, f.ctypes.data, 40000, 4, C.byref(good), 0, out.ctypes.data, None) == native.MR_E_INVALID and b"resolution" in lib.mr_last_error()
    assert post(handle, None, 4, 4, C.byref(good), 0, out.ctypes.data, None) == native.MR_E_INVALID and b"NULL" in lib.mr_last_error()
    assert post(None, f.ctypes.data, 4, 4, C.byref(good), 0, out.ctypes.data, None) == native.MR_E_INVALID
    counts = np.zeros(4, np.int32)
    assert lib.mr_debug_bloom(handle, counts.ctypes.data) == 0 and counts.tolist() == [0] * 4
    lib.mr_scene_destroy(handle)


def test_the_python_class_and_property(api):
    import py_numpy_renderer_amd as pkg
    from py_numpy_renderer_amd import Bloom, multigpu
    assert "Bloom" in pkg.__all__ and pkg.Bloom is Bloom
    assert (Bloom().threshold, Bloom().intensity, Bloom().levels) == (0.8, 0.5, 4)
    bloom = Bloom(threshold=0, intensity=2, levels=6)
    assert repr(bloom) == "Bloom(threshold=0.0, intensity=2.0, levels=6)" and Bloom.__slots__ == ("threshold", "intensity", "levels")
    with pytest.raises(AttributeError, match="read-only"):
        bloom.levels = 2
    for threshold in (-0.1, 1, 1.5, float("nan"), float("inf"), 0.99999999):          # (the last is 1 as float32)
        with pytest.raises(ValueError, match="bloom: threshold"):
            Bloom(threshold=threshold)
    for intensity in (0, -1, float("nan"), float("inf"), 1e-46, 1e39):
        with pytest.raises(ValueError, match="bloom: intensity"):
            Bloom(intensity=intensity)
    for value in ("0.5", True, [0.5], 1j, None):
        with pytest.raises(TypeError, match="real number"):
            Bloom(threshold=value)
        with pytest.raises(TypeError, match="real number"):
            Bloom(intensity=value)
    for levels in (0, 7, -1, 100):
        with pytest.raises(ValueError, match="bloom: levels"):
            Bloom(levels=levels)
    for levels in (4.0, "4", True, None):
        with pytest.raises(TypeError, match="an int"):
            Bloom(levels=levels)
    assert Bloom(levels=np.int32(1)).levels == 1 and Bloom(threshold=np.float32(0.5)).threshold == 0.5
    scene = scenes.cube_small(api)
    assert scene.bloom is None
    with pytest.raises(TypeError, match="Bloom"):
        scene.bloom = 0.8
    scene.bloom = bloom
    assert scene.bloom is bloom
    with pytest.raises(ValueError, match="bloom"):
        multigpu.BandRenderer(scene)                     # (refused before any device is asked for)
    scene.accumulate().close()                           # the pass keeps no state between frames: an accumulation takes it
    scene.bloom = None
    assert scene.bloom is None


def test_the_packer_s_gain_and_level_rule(api, native):
    from py_numpy_renderer_amd import Bloom, _pack
    scene = scenes.cube_small(api)
    for intensity, levels in ((0.5, 4), (1.0, 3), (0.3, 6), (2.0, 1)):
        scene.bloom = Bloom(threshold=0.625, intensity=intensity, levels=levels)
        for s, extra in ((1, 0), (2, 1), (4, 2)):
            scene.supersample = s
            t, g, n = _pack.bloom_constants(scene)
            assert t == 0.625 and n == levels + extra, "levels + log2(supersample): as wide in output pixels"
            assert np.float32(g) == g and g == float(np.float32(np.float64(intensity) / levels)) == float(bloom_ref.gain(intensity, levels))
            d = native.fill_bloom_desc(t, g, n)
            assert (d.threshold, d.gain, d.levels) == (t, g, n) and n <= 8
    assert native.DeviceRenderer._bloom_values(scene) == (0.625, 2.0, 1)
    scene.bloom = None
    assert native.DeviceRenderer._bloom_values(scene) is None
