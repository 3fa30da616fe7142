"""CPU: the tone mapping's host mirror ``mr_host_tone_map`` against the NumPy restatement tonemap_ref.py, bit for bit --
frame, histogram and exposure -- on every field of tonemap_fields.py; the consequences csrc/tonemap_def.h states; the
mutants of the definition, each told apart by some field; what the library and ``ToneMap`` refuse; the packer's table and
its permille.  No device is touched."""
import numpy as np
import pytest

import tonemap_fields as tf
import tonemap_ref as ref

f32 = np.float32
CASES = tf.cases()


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    _native.load_library()
    return _native


# ---------------------------------------------------------------------------- 1. the mirror is the definition
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_mirror_is_the_reference_on_every_field(native, case):
    for operator in ref.OPERATORS:
        for fixed in (None, 1.0, 0.37):
            for e_prev in {None, case.e_prev, 3.0}:
                at = case.at(e_prev=e_prev, operator=operator, exposure=case.params.exposure if fixed is None else fixed)
                got, want = at.mirror(native), at.reference()
                print(f"{at!r}: e = {want[2]!r}, {int(want[1].sum())} samples metered")
                assert tf.same(got, want) == (0, 0, 0), f"{at!r}: (frame floats, counts, exposure) that differ: {tf.same(got, want)}"


def test_the_fields_cover_what_they_are_named_for():
    shapes = {c.shape for c in CASES}
    assert set(tf.SIZES) | {tf.LARGE} <= shapes
    assert {h * w % 4 for h, w in tf.SIZES} == {0, 1, 2, 3}
    hist = ref.histogram(tf.ramp())
    assert (hist[1:] >= 1).all() and hist[0] == 0, "a sample in each of the bins 1 .. 255"
    grey = tf.ramp()[..., 0].ravel()
    y = ref.luminance(tf.ramp()).ravel()
    for k in range(-23, 9):                                  # both sides of every octave boundary, as the meter sees them
        edge = f32(np.ldexp(1.0, k))
        i = int(np.nonzero(grey == edge)[0][0])
        assert ref.bins(y[i:i + 2]).tolist() in ([8 * (k + 24), 8 * (k + 24) - 1], [8 * (k + 24) - 1] * 2, [8 * (k + 24)] * 2)
    assert ref.bins(f32([2.0 ** -24, np.nextafter(f32(2.0 ** -24), f32(0)), 1e-40, 0.0, -0.0, 256.0, 65504.0])).tolist() == [0, 0, 0, 0, 0, 255, 255]
    for c in CASES:
        assert np.isfinite(c.frame).all() and c.frame.min() >= 0
    assert any(int(c.reference()[1].sum()) == 0 and c.frame.max() > 0 for c in CASES), "a trim that keeps nothing of a lit frame"
    pair = tf.order_pair()
    assert ref.bins(ref.luminance(pair)).ravel().tolist() == [176, 176, 175]
    assert ref.bins(ref.luminance(pair, "luminance_order")).ravel().tolist() == [175, 175, 176]


def test_the_first_bin_starts_at_two_to_the_minus_24():
    assert ref.bins(f32([2.0 ** -24])).tolist() == [0] and ref.bins(f32([2.0 ** -24 * 1.125])).tolist() == [1]
    assert ref.bins(f32([2.0 ** -24 * 1.125, 1.0, 0.18, 255.9])).tolist() == [1, 192, 171, 255]


# ---------------------------------------------------------------------------- 2. the stated consequences
def _metered(native, frame, **params):
    return tf.Case("", frame, ref.Params(**params)).mirror(native)


def test_scaling_the_frame_by_a_power_of_two_scales_the_exposure_exactly(native):
    frame = tf.noise((37, 53))
    hist = ref.histogram(frame)
    assert hist[:1 + 24].sum() == 0 and hist[255 - 16:].sum() == 0, "no sample leaves bins 1 .. 254 when scaled"
    e = _metered(native, frame)[2]
    assert 2.0 ** -6 < e / 8 and e * 8 < 2.0 ** 6, "the clamp is not hit"
    for k in (-3, 2):
        scaled = _metered(native, tf.noise((37, 53), k=k))
        assert scaled[2] == f32(np.ldexp(e, -k)), (k, e, scaled[2])
        assert (scaled[1] == np.roll(hist, 8 * k)).all(), "every sample moves 8 k bins"


def test_the_meter_is_within_half_a_bin_of_the_geometric_mean(native):
    frame = tf.noise((37, 53))
    e = float(_metered(native, frame)[2])
    exact = 0.18 / np.exp2(np.log2(ref.luminance(frame).astype(np.float64)).mean())
    print(f"metered {e!r}, from the exact geometric mean {exact!r}")
    assert abs(np.log2(e / exact)) <= 1 / 16 + 2 / 256       # (half a bin a sample; the rounding of FRAC and of q)
    flat = float(_metered(native, tf.uniform((3, 5)))[2])
    assert f32(flat) == f32(f32(0.18) * ref.EXP2[122]) * f32(4) and abs(flat - 1.0018256) < 1e-7


def test_the_trims_move_the_mean(native):
    n = ref.histogram(tf.noise((37, 53)))
    q_all = ref.mean_q(*ref.sums(n, 0, 1000))
    q_trim = ref.mean_q(*ref.sums(n, 500, 950))
    q_dark = ref.mean_q(*ref.sums(n, 0, 1))
    print(f"q untrimmed {q_all}, 500 .. 950 {q_trim}, 0 .. 1 {q_dark}")
    assert q_dark < q_all < q_trim and q_trim - q_all > 256, "the upper half is more than a stop brighter"
    assert ref.sums(n, 0, 1)[1] == 1961 // 1000
    got = [float(_metered(native, tf.noise((37, 53)), low_pm=lo, high_pm=hi)[2]) for lo, hi in ((0, 1000), (500, 950))]
    assert got[1] < got[0]


@pytest.mark.parametrize("case", [c for c in CASES if c.params.exposure is None][:12], ids=lambda c: c.name)
def test_linear_at_exposure_one_is_the_identity(native, case):
    out, hist, e = case.at(operator="linear", exposure=1.0).mirror(native)
    assert tf.bits(out, case.frame) == 0 and e == 1.0 and not hist.any()


def test_the_order_of_the_samples_does_not_matter(native):
    frame = tf.noise((64, 65))
    want = _metered(native, frame)
    shuffled = np.random.default_rng(3).permutation(frame.reshape(-1, 3)).reshape(frame.shape)
    got = _metered(native, shuffled)
    assert (got[1] == want[1]).all() and got[2] == want[2]
    assert tf.bits(np.sort(got[0].reshape(-1, 3), axis=0), np.sort(want[0].reshape(-1, 3), axis=0)) == 0


def test_nothing_metered_keeps_the_previous_exposure_or_one(native):
    black = tf.Case("black", np.zeros((3, 5, 3), f32), ref.Params(operator="linear", speed=0.5))
    assert black.mirror(native)[2] == 1.0
    assert black.at(e_prev=2.5).mirror(native)[2] == 2.5
    assert not black.mirror(native)[1].any(), "black is metered out"


def test_adaptation_moves_from_the_previous_exposure_towards_the_target(native):
    case = tf.Case("adapt", tf.noise((37, 53)), ref.Params(speed=0.25))
    e_t = case.mirror(native)[2]
    e = case.at(e_prev=2.0).mirror(native)[2]
    assert e == f32(f32(2.0) + f32(f32(0.25) * f32(e_t - f32(2.0)))) and min(e_t, 2.0) < e < max(e_t, 2.0)


# ---------------------------------------------------------------------------- 3. the mutants
@pytest.mark.parametrize("mutant", sorted(ref.MUTANTS))
def test_every_mutant_is_told_apart_by_a_field(mutant):
    killers = [c.name for c in CASES if tf.same(c.reference(mutant), c.reference()) != (0, 0, 0)]
    print(f"{mutant} ({ref.MUTANTS[mutant]}): told apart by {killers}")
    assert killers, f"no field of tonemap_fields.py tells '{ref.MUTANTS[mutant]}' from the definition"


# ---------------------------------------------------------------------------- 4. the refusals
def _desc(native, **over):
    args = dict(op=2, fixed=0, exposure=1.0, key=0.18, white=4.0, speed=1.0, min_exposure=2.0 ** -6, max_exposure=2.0 ** 6, low_pm=0, high_pm=1000,
                table=ref.EXP2)
    args.update(over)
    return native.fill_tone_map_desc(**args)


BAD_TABLES = {"exp2[0] != 1": lambda t: t.__setitem__(0, np.nextafter(f32(1), f32(2))), "not increasing": lambda t: t.__setitem__(7, t[6]),
              "reaches 2": lambda t: t.__setitem__(255, 2.0), "NaN": lambda t: t.__setitem__(100, np.nan)}


@pytest.mark.parametrize("over, match", [
    (dict(op=3), "operator"), (dict(op=-1), "operator"), (dict(fixed=2), "fixed"),
    (dict(key=0.0), "key"), (dict(key=np.inf), "key"), (dict(key=1e-50), "key"), (dict(white=-1.0), "white"), (dict(white=np.nan), "white"),
    (dict(exposure=0.0, fixed=1), "exposure"), (dict(exposure=1e39, fixed=1), "exposure"),
    (dict(min_exposure=0.0), "min_exposure"), (dict(max_exposure=np.inf), "max_exposure"), (dict(min_exposure=2.0, max_exposure=1.0), "exceed"),
    (dict(speed=0.0), "speed"), (dict(speed=1.5), "speed"), (dict(speed=np.nan), "speed"),
    (dict(low_pm=-1), "trims"), (dict(low_pm=500, high_pm=500), "trims"), (dict(high_pm=1001), "trims"),
], ids=lambda v: None if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_the_library_refuses_a_bad_description(native, over, match):
    with pytest.raises(ValueError, match=match):
        native.host_tone_map(tf.uniform((2, 3)), _desc(native, **over))


@pytest.mark.parametrize("name", sorted(BAD_TABLES))
def test_the_library_checks_the_table(native, name):
    table = ref.EXP2.copy()
    BAD_TABLES[name](table)
    with pytest.raises(ValueError, match="exp2"):
        native.host_tone_map(tf.uniform((2, 3)), _desc(native, table=table))
    native.host_tone_map(tf.uniform((2, 3)), _desc(native))


def test_the_mirror_refuses_bad_arguments(native):
    lib, C = native.load_library(), native.C
    frame, out = tf.uniform((2, 3)), np.empty((2, 3, 3), f32)
    desc = _desc(native)
    call = lambda f, h, w, d, has, prev, o: lib.mr_host_tone_map(f, h, w, d, has, prev, o, None, None)
    assert call(frame.ctypes.data, 2, 3, C.byref(desc), 0, 0.0, out.ctypes.data) == 0
    assert call(None, 2, 3, C.byref(desc), 0, 0.0, out.ctypes.data) == native.MR_E_INVALID
    assert call(frame.ctypes.data, 2, 3, None, 0, 0.0, out.ctypes.data) == native.MR_E_INVALID
    assert call(frame.ctypes.data, 2, 3, C.byref(desc), 0, 0.0, None) == native.MR_E_INVALID
    assert call(frame.ctypes.data, 0, 3, C.byref(desc), 0, 0.0, out.ctypes.data) == native.MR_E_INVALID
    assert call(frame.ctypes.data, 2, 32768, C.byref(desc), 0, 0.0, out.ctypes.data) == native.MR_E_INVALID
    for prev in (0.0, -1.0, np.inf, np.nan):
        assert call(frame.ctypes.data, 2, 3, C.byref(desc), 1, prev, out.ctypes.data) == native.MR_E_INVALID
    assert call(frame.ctypes.data, 2, 3, C.byref(desc), 0, np.nan, out.ctypes.data) == 0, "without has_prev the value is not read"
    assert lib.mr_scene_set_tone_map(None, C.byref(desc)) == native.MR_E_INVALID
    assert lib.mr_scene_reset_exposure(None) == native.MR_E_INVALID


def test_the_mirror_may_write_in_place(native):
    case = next(c for c in CASES if c.name == "noise, narrow bounds")
    want = case.mirror(native)
    lib, C = native.load_library(), native.C
    frame = case.frame.copy()
    desc = case.desc(native)
    assert lib.mr_host_tone_map(frame.ctypes.data, *case.shape, C.byref(desc), 0, 0.0, frame.ctypes.data, None, None) == 0
    assert tf.bits(frame, want[0]) == 0


def test_tone_map_checks_its_arguments(api):
    import scenes
    from py_numpy_renderer_amd import ToneMap, multigpu
    tm = ToneMap()
    assert (tm.operator, tm.exposure, tm.key, tm.low, tm.high, tm.speed, tm.white) == ("aces", None, 0.18, 0.0, 1.0, 1.0, 4.0)
    assert (tm.min_exposure, tm.max_exposure) == (2.0 ** -6, 2.0 ** 6) and not tm.adaptive
    assert ToneMap(speed=0.5).adaptive and not ToneMap(speed=0.5, exposure=2.0).adaptive
    assert not ToneMap(speed=1.0 - 1e-12).adaptive, "1 as float32"
    assert "reinhard" in repr(ToneMap("reinhard")) and eval(repr(ToneMap("reinhard", exposure=2))).exposure == 2.0
    with pytest.raises(AttributeError):
        tm.key = 1.0
    for bad in (dict(operator="filmic"), dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=float("inf")), dict(key=0.0), dict(key=1e-50),
                dict(white=0.0), dict(speed=0.0), dict(speed=1.01), dict(speed=float("nan")), dict(low=-0.1), dict(high=1.1), dict(low=0.5, high=0.5),
                dict(low=0.7, high=0.2), dict(low=0.5, high=0.5004), dict(min_exposure=0.0), dict(max_exposure=float("nan")),
                dict(min_exposure=3.0, max_exposure=2.0)):
        with pytest.raises(ValueError):
            ToneMap(**bad)
    for bad in (dict(operator=2), dict(exposure="1"), dict(key=None), dict(speed=True), dict(low="0"), dict(white=[4.0])):
        with pytest.raises(TypeError):
            ToneMap(**bad)
    scene = scenes.cube_small(api)
    assert scene.tone_map is None
    with pytest.raises(TypeError, match="ToneMap"):
        scene.tone_map = "aces"
    scene.tone_map = tm
    assert scene.tone_map is tm
    with pytest.raises(ValueError, match="tone_map"):
        multigpu.BandRenderer(scene)                     # (refused before any device is asked for)
    scene.accumulate().close()                           # metered frame by frame the pass keeps no state: an accumulation takes it
    scene.tone_map = ToneMap(exposure=2.0, speed=0.5)
    scene.accumulate().close()                           # ... and with a fixed exposure
    scene.tone_map = ToneMap(speed=0.5)
    with pytest.raises(ValueError, match="adaptive tone_map"):
        scene.accumulate()                               # (an adaptive one has no previous frame there)
    scene.tone_map = None
    assert scene.tone_map is None
    scene.accumulate().close()


def test_tone_map_is_exported_and_bound():
    import py_numpy_renderer_amd as api
    from py_numpy_renderer_amd import _native
    assert "ToneMap" in api.__all__ and api.ToneMap is not None
    for name in ("mr_scene_set_tone_map", "mr_scene_reset_exposure", "mr_host_tone_map", "mr_read_exposure", "mr_read_luminance_histogram",
                 "mr_debug_tone_map", "mr_debug_tone_map_times", "mr_debug_tone_map_post"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(_native.load_library(), name)


# ---------------------------------------------------------------------------- 5. the packer
def test_the_packers_table_and_permille():
    from py_numpy_renderer_amd import ToneMap, _pack
    table = _pack.tone_map_table()
    assert table.dtype == np.float32 and table.shape == (256,)
    assert tf.bits(table, np.exp2(np.arange(256) / 256.0).astype(np.float32)) == 0 and tf.bits(table, ref.EXP2) == 0
    assert table[0] == 1.0 and (np.diff(table) > 0).all() and table[-1] < 2.0
    assert [_pack.permille(v) for v in (0.0, 1.0, 0.5, 0.95, 0.0004, 0.0005, 0.9995, 0.29, 0.57)] == [0, 1000, 500, 950, 0, 1, 1000, 290, 570]

    class Holder:
        tone_map = ToneMap("reinhard", key=0.25, low=0.5, high=0.95, speed=0.5, white=2.0, min_exposure=0.5, max_exposure=8.0)
    got = _pack.tone_map_constants(Holder)
    assert got[:10] == (1, 0, 1.0, 0.25, 2.0, 0.5, 0.5, 8.0, 500, 950) and got[10] is not None
    Holder.tone_map = ToneMap("linear", exposure=3.0)
    assert _pack.tone_map_constants(Holder)[:3] == (0, 1, 3.0)
