"""CPU: the light shafts' host mirror ``mr_host_light_shafts`` against the NumPy restatement shafts_ref.py, bit for bit -- the
frame, the march's source S and its result R -- on every field of shafts_fields.py at every d; the consequences
csrc/shafts_def.h states, as known answers; the mutants of the definition, each told apart by some field; what the library
and the Python layer refuse; the packer's light position, weights and levels.  No device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes
import shafts_fields as sf
import shafts_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sf.cases()
F32 = np.float32


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    _native.load_library()
    return _native


# ---------------------------------------------------------------------------- 1. the mirror is the definition
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_mirror_is_the_reference_on_every_field(native, case):
    changed = 0
    for levels in sf.LEVELS:
        at = case.at(levels)
        want, got = at.reference(), at.mirror(native)
        assert got[1].shape == want[1].shape == got[2].shape == shafts_ref.level_size(*at.shape, levels) + (3,), f"{at!r}: the level's size"
        out, source, march = sf.all_bits(got, want)
        assert out == 0 and source == 0 and march == 0, f"{at!r}: {out} floats of the frame, {source} of S and {march} of R are not the reference's"
        changed += sf.bits(got[0], at.frame)
    quiet = case.name in ("below the threshold", "mask none")
    assert (changed > 0) != quiet, f"{case!r}: {changed} floats changed"


def test_the_fields_cover_what_they_are_named_for():
    shapes = {c.shape for c in CASES}
    assert {(1, 1), (1, 2), (2, 3), (3, 5), (17, 33), (130, 9)} == set(sf.SMALL_SIZES) <= shapes
    for d in sf.LEVELS:
        k = 3 << d
        assert {(k - 1, k + 1), (k + 1, k - 1)} <= shapes, f"2^{d} k +- 1 on each axis"
        for a in (-1, 1):
            assert ((sf.SOURCE_BLOCK[0] << d) + a, (sf.SOURCE_BLOCK[1] << d) + a) in shapes, f"k_shaft_source's block at d = {d}, {a:+d}"
    header = open(os.path.join(ROOT, "py-numpy-renderer_amd", "csrc", "kernels_shafts.h")).read()
    assert f"SHAFT_SRC_TW = {sf.SOURCE_BLOCK[1]}, SHAFT_SRC_TH = {sf.SOURCE_BLOCK[0]};" in header and f"SHAFT_MARCH_T = {sf.MARCH_BLOCK};" in header
    assert any(w % 4 == 0 and w % 16 for _, w in shapes) and any(w % 4 for _, w in shapes), "rows on and off 16-byte boundaries"
    assert any(h > sf.MARCH_BLOCK << 1 and w > sf.MARCH_BLOCK << 1 for h, w in shapes), "more than one block of k_shaft_march at d = 1"
    names = {c.name for c in CASES}
    assert len(names) == len(CASES)
    assert {f"mask {k}" for k in ("none", "all", "bar", "comb", "corners")} <= names and {f"light {k}" for k in sf.LIGHTS} <= names
    assert {c.samples for c in CASES} >= {1, 2, 64, 128} and {c.density for c in CASES} >= {0.25, 1.0, 1.5}
    for c in CASES:
        assert c.frame.min() >= 0 and c.frame.max() <= 1 and np.isfinite(c.frame).all()
    # the lights stand where their names say, on every level
    h, w = shafts_ref.level_size(*sf.FIELD, 2)
    at = {name: rule(h, w) for name, rule in sf.LIGHTS.items()}
    inside = lambda p: -0.5 <= p[0] <= w - 0.5 and -0.5 <= p[1] <= h - 0.5
    assert inside(at["inside"]) and at["on a sample"] == (round(at["on a sample"][0]), round(at["on a sample"][1]))
    assert at["on the left border"][0] == -0.5 and at["on the right border"][0] == w - 0.5 and at["on the bottom border"][1] == -0.5 and at["on the top border"][1] == h - 0.5
    for name in sf.LIGHTS:
        assert inside(at[name]) == (not name.startswith(("just", "past", "far"))), name
    # far outside: tap 1 of every sample has left the level, at any density the fields use
    far = next(c for c in CASES if c.name == "light far outside")
    lx, ly = far.light
    assert abs(lx) * 0.25 / far.samples > w and abs(ly) * 0.25 / far.samples > h


# ---------------------------------------------------------------------------- 2. the stated consequences, as known answers
@pytest.mark.parametrize("levels", sf.LEVELS)
def test_no_sky_above_the_threshold_leaves_the_frame_untouched(native, levels):
    for case in (sf.below().at(levels), next(c for c in CASES if c.name == "mask none").at(levels)):
        sky = ~np.isfinite(case.zbuf)
        assert not sky.any() or case.frame[sky].max() <= case.threshold
        assert case.frame[~sky].max() > case.threshold, "a covered sample above the threshold: the mask is what keeps it out"
        out, S, R = case.mirror(native)
        assert sf.bits(out, case.frame) == 0
        assert not S.view(np.uint32).any() and not R.view(np.uint32).any(), "S and R are +0"


@pytest.mark.parametrize("light", ["inside", "on a sample", "on the top border"])
@pytest.mark.parametrize("samples, density, decay", [(1, 1.0, 0.97), (2, 0.25, 0.5), (64, 1.0, 0.97), (128, 0.9, 1.0)])
@pytest.mark.parametrize("levels", sf.LEVELS)
def test_a_uniform_sky_marches_to_the_iterated_sum(native, levels, samples, density, decay, light):
    case = sf.uniform(levels=levels, light=light, samples=samples, density=density, decay=decay)
    assert all(v % (1 << levels) == 0 for v in case.shape) and density <= 1
    out, S, R = case.mirror(native)
    s = F32(0.375)
    assert (S == s).all(), "S is uniform, exactly"
    acc = F32(0.0)
    for w in shafts_ref.weights(decay, samples):
        acc = F32(acc + w * s)
    assert (R == acc).all(), "R is the same iterated sum at every coarse sample"
    assert abs(float(acc) - 0.375) < 0.375 * samples * 2.0 ** -23, "the weights sum to 1"
    assert (out == F32(F32(0.75) + F32(1.0) * acc)).all() and out.shape == case.frame.shape


@pytest.mark.parametrize("levels", sf.LEVELS)
def test_a_ray_through_an_occluder_gathers_strictly_less(native, levels):
    case = sf.occluder(levels)
    out, S, R = case.mirror(native)
    lx, ly = (int(v) for v in case.light)
    h, w = R.shape[:2]
    covered = np.isfinite(case.zbuf)[::1 << levels, ::1 << levels]      # the block on the level: it covers whole coarse samples
    xs = np.flatnonzero(covered[ly])
    assert len(xs) and xs.max() < lx, "the block lies left of the light, on its row"
    reach = min(lx - 1, w - 1 - lx)
    shaded = [k for k in range(1, reach + 1) if lx - k < xs.min()]
    assert shaded, "no coarse sample beyond the block"
    for k in shaded:
        a, b = R[ly, lx - k], R[ly, lx + k]              # the same distance from the light: through the block, and through open sky
        assert (a < b).all(), (k, a, b)
        assert (b == R[ly, lx]).all(), "an open ray gathers what the light's own sample gathers"
    assert (out >= case.frame).all() and (out[0, -1] > case.frame[0, -1]).all()


def test_every_value_is_finite_at_the_extremes(native):
    frame = sf.seeded((9, 14))
    frame[3, 4] = (1.0, 1.0, 1.0)
    frame[5, 5] = (F32(1e-38), 0.0, 0.0)                   # a bright sample next to nothing: (m - t) / m with the smallest m
    z = sf.zbuffer(sf.mask((9, 14), "all"))
    z[0, 0] = np.nan                                       # not finite: sky
    for t in (0.0, 1e-45, 0.99999994):
        for light in ((3.0, 2.0), (3.0e38, -3.0e38), (-1e30, 1e-30)):
            for step in (1.0 / 64, 3.0e38, 1e-45):
                desc = native.fill_light_shafts_desc(*light, t, 1.0, step, 64, 2, shafts_ref.weights(0.97, 64))
                out, S, R = native.host_light_shafts(frame, z, desc, fields=True)
                assert all(np.isfinite(a).all() for a in (out, S, R)), (t, light, step)
    desc = native.fill_light_shafts_desc(3.0, 2.0, 0.0, 1.0, 1.0 / 64, 64, 1, shafts_ref.weights(0.97, 64))
    assert native.host_light_shafts(frame, z, desc, fields=True)[1][0, 0].any(), "a NaN in the z-buffer is sky"


# ---------------------------------------------------------------------------- 3. the mutants
@pytest.mark.parametrize("mutant", shafts_ref.MUTANTS)
def test_every_mutant_is_told_apart_by_some_field(native, mutant):
    caught = []
    for case in CASES:
        want, wrong = case.reference(), case.reference(mutant=mutant)
        sizes_differ = wrong[1].shape != want[1].shape
        if sizes_differ or sf.bits(wrong[0], want[0]):
            caught.append(case.name)
            if not sizes_differ:                         # ... and the mirror stands with the definition
                assert sf.bits(case.mirror(native)[0], want[0]) == 0
    print(f"{mutant}: told apart by {len(caught)} of {len(CASES)} fields: {caught[:6]}")
    assert caught, f"no field tells {mutant} from the definition"


# ---------------------------------------------------------------------------- 4. refusals and bindings, no device
def _desc(native, **o):
    n = o.get("n", 4)
    weights = o.get("weights", shafts_ref.weights(0.9, max(min(n, 128), 1)))
    return native.fill_light_shafts_desc(o.get("lx", 1.0), o.get("ly", 2.0), o.get("t", 0.25), o.get("g", 0.5), o.get("step", 0.25), n, o.get("d", 2), weights)


BAD = (("position", dict(lx=float("nan"))), ("position", dict(ly=float("inf"))), ("threshold", dict(t=float("nan"))), ("threshold", dict(t=float("inf"))),
       ("threshold", dict(t=-0.5)), ("gain", dict(g=0.0)), ("gain", dict(g=float("nan"))), ("gain", dict(g=-1.0)), ("gain", dict(g=float("inf"))),
       ("step", dict(step=0.0)), ("step", dict(step=float("nan"))), ("step", dict(step=-0.25)), ("step", dict(step=float("inf"))),
       ("samples", dict(n=0)), ("samples", dict(n=129)), ("samples", dict(n=-1)), ("halvings", dict(d=0)), ("halvings", dict(d=5)), ("halvings", dict(d=-1)),
       ("weights", dict(weights=[0.5, float("nan"), 0.25, 0.25])), ("weights", dict(weights=[0.5, 0.5, -0.25, 0.25])),
       ("weights", dict(weights=[0.5, 0.5, 0.25, float("inf")])))


def test_symbols_are_bound(native):
    lib = native.load_library()
    for name in ("mr_scene_set_light_shafts", "mr_host_light_shafts", "mr_debug_light_shafts", "mr_debug_light_shafts_times", "mr_debug_light_shafts_post"):
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert C.sizeof(native.LightShaftsDesc) == 5 * 4 + 2 * 4 + 128 * 4
    header = open(os.path.join(ROOT, "include", "mi355rast.h")).read()
    body = header.split("typedef struct mr_light_shafts_desc")[1].split("} mr_light_shafts_desc;")[0]
    order = [body.index(word) for word in ("float light_x, light_y;", "float threshold;", "float gain;", "float step;", "int32_t samples;", "int32_t halvings;",
                                           "float weights[128];")]
    assert order == sorted(order)
    assert "#define MR_ABI_VERSION 4" in header and lib.mr_abi_version() == 4


def test_the_library_checks_the_description(native):
    lib = native.load_library()
    handle = lib.mr_scene_create()
    assert lib.mr_scene_set_light_shafts(None, C.byref(_desc(native))) == native.MR_E_INVALID
    assert lib.mr_scene_set_light_shafts(handle, None) == 0                       # off, on a scene that never had it
    assert lib.mr_scene_set_light_shafts(handle, C.byref(_desc(native))) == 0, lib.mr_last_error()      # (copied: no device is touched)
    for word, over in BAD:
        assert lib.mr_scene_set_light_shafts(handle, C.byref(_desc(native, **over))) == native.MR_E_INVALID, over
        assert word.encode() in lib.mr_last_error(), (over, lib.mr_last_error())
    # (a weight behind the first `samples` is not read; a light far outside, a threshold of 0 and every d and n at their ends are taken)
    for ok in (dict(weights=[0.25, 0.25, 0.25, 0.25, float("nan")]), dict(lx=-3e38, ly=3e38), dict(t=0.0), dict(t=5.0), dict(d=1), dict(d=4), dict(n=1), dict(n=128)):
        assert lib.mr_scene_set_light_shafts(handle, C.byref(_desc(native, **ok))) == 0, ok
    out = np.zeros(4, np.int32)
    assert lib.mr_debug_light_shafts(handle, out.ctypes.data) == 0 and out.tolist() == [0] * 4
    assert lib.mr_debug_light_shafts(handle, None) == native.MR_E_INVALID
    ms = (C.c_float * 3)()
    assert lib.mr_debug_light_shafts_times(handle, ms) == native.MR_E_INVALID and b"no frame with light shafts yet" in lib.mr_last_error()
    # a split frame is refused before any device work
    fr = native.FrameDesc()
    fr.width, fr.height, fr.system, fr.row_begin, fr.row_end = 8, 8, 1, 0, 4
    rgb = np.zeros((8, 8, 3), np.uint8)
    assert lib.mr_render(handle, C.byref(fr), rgb.ctypes.data, None) == native.MR_E_INVALID
    assert b"light shafts takes whole frames" in lib.mr_last_error()
    fr.row_end, fr.stripe_count, fr.stripe_index = 8, 2, 0
    assert lib.mr_render_async(handle, C.byref(fr), rgb.ctypes.data, 0) == native.MR_E_INVALID
    assert b"light shafts takes whole frames" in lib.mr_last_error()
    lib.mr_scene_destroy(handle)


def test_the_mirror_and_the_debug_entry_check_their_arguments(native):
    lib = native.load_library()
    f, z, out = np.ones((4, 4, 3), np.float32), np.full((4, 4), np.inf), np.empty((4, 4, 3), np.float32)
    good = _desc(native)
    args = lambda **o: [o.get("f", f.ctypes.data), o.get("z", z.ctypes.data), o.get("h", 4), o.get("w", 4), o.get("d", C.byref(good)), o.get("out", out.ctypes.data),
                        None, None]
    assert lib.mr_host_light_shafts(*args()) == 0                    # (neither S nor R is asked for: not an error)
    assert (out > f).all()
    refused = [dict(f=None), dict(z=None), dict(out=None), dict(d=None), dict(h=0), dict(w=-1), dict(h=40000), dict(out=f.ctypes.data)]
    refused += [dict(d=C.byref(_desc(native, **over))) for _, over in BAD]
    for over in refused:
        assert lib.mr_host_light_shafts(*args(**over)) == native.MR_E_INVALID, over
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        native.host_light_shafts(f[..., :2], z, good)
    with pytest.raises(ValueError, match=r"zbuf must be \(H, W\)"):
        native.host_light_shafts(f, z[:2], good)
    with pytest.raises(ValueError, match="halvings"):
        native.host_light_shafts(f, z, _desc(native, d=5))
    # mr_debug_light_shafts_post refuses before it asks for a device
    handle = lib.mr_scene_create()
    for word, over in BAD:
        with pytest.raises(ValueError, match=word):
            native.debug_light_shafts_post(handle, f, z, _desc(native, **over))
    post = lib.mr_debug_light_shafts_post
    assert post(handle, f.ctypes.data, z.ctypes.data, 40000, 4, C.byref(good), out.ctypes.data, None, None) == native.MR_E_INVALID and b"resolution" in lib.mr_last_error()
    assert post(handle, None, z.ctypes.data, 4, 4, C.byref(good), out.ctypes.data, None, None) == native.MR_E_INVALID and b"NULL" in lib.mr_last_error()
    assert post(handle, f.ctypes.data, None, 4, 4, C.byref(good), out.ctypes.data, None, None) == native.MR_E_INVALID and b"NULL" in lib.mr_last_error()
    assert post(None, f.ctypes.data, z.ctypes.data, 4, 4, C.byref(good), out.ctypes.data, None, None) == native.MR_E_INVALID
    counts = np.zeros(4, np.int32)
    assert lib.mr_debug_light_shafts(handle, counts.ctypes.data) == 0 and counts.tolist() == [0] * 4
    lib.mr_scene_destroy(handle)


def test_the_python_class_and_property(api):
    import py_numpy_renderer_amd as pkg
    from py_numpy_renderer_amd import LightShafts, multigpu
    assert "LightShafts" in pkg.__all__ and pkg.LightShafts is LightShafts
    default = LightShafts()
    assert tuple(getattr(default, n) for n in LightShafts.__slots__) == (0, 0.5, 0.9, 0.97, 64, 0.0, 2)
    assert LightShafts.__slots__ == ("light", "intensity", "density", "decay", "samples", "threshold", "halvings")
    shafts = LightShafts(light=1, intensity=2, density=1, decay=1, samples=128, threshold=0, halvings=1)
    assert repr(shafts) == "LightShafts(light=1, intensity=2.0, density=1.0, decay=1.0, samples=128, threshold=0.0, halvings=1)"
    with pytest.raises(AttributeError, match="read-only"):
        shafts.samples = 2
    for name, values in (("intensity", (0, -1, float("nan"), float("inf"), 1e-46, 1e39)), ("density", (0, -0.5, float("nan"), float("inf"), 1e-46, 1e39)),
                         ("decay", (0, -0.5, 1.0000001, 2, float("nan"), float("inf"), 1e-46)), ("threshold", (-0.1, 1, 1.5, float("nan"), float("inf"), 0.99999999))):
        for value in values:
            with pytest.raises(ValueError, match=f"light shafts: {name}"):
                LightShafts(**{name: value})
        for value in ("0.5", True, [0.5], 1j, None):
            with pytest.raises(TypeError, match="real number"):
                LightShafts(**{name: value})
    for name, values in (("light", (-1, 2 ** 31)), ("samples", (0, 129, -1)), ("halvings", (0, 3, -1))):
        for value in values:
            with pytest.raises(ValueError, match=f"light shafts: {name}"):
                LightShafts(**{name: value})
        for value in (1.0, "1", True, None):
            with pytest.raises(TypeError, match="an int"):
                LightShafts(**{name: value})
    assert LightShafts(samples=np.int32(1)).samples == 1 and LightShafts(threshold=np.float32(0.5)).threshold == 0.5
    scene = scenes.cube_small(api)
    assert scene.light_shafts is None
    with pytest.raises(TypeError, match="LightShafts"):
        scene.light_shafts = 0.5
    scene.light_shafts = shafts
    assert scene.light_shafts is shafts
    with pytest.raises(ValueError, match="light_shafts"):
        multigpu.BandRenderer(scene)                     # (refused before any device is asked for)
    scene.accumulate().close()                           # the pass keeps no state between frames: an accumulation takes it
    scene.light_shafts = None
    assert scene.light_shafts is None


# ---------------------------------------------------------------------------- 5. the packer
def _hand_projection(scene, point, s):
    """Row vector through the camera's MVP, the divide and the viewport of the s-times finer grid, written out."""
    cam = scene.camera
    clip = np.asarray(point, dtype=np.float64) @ np.asarray(cam.MVP, dtype=np.float64)
    height, width = (s * int(v) for v in scene.resolution)
    x = clip[0] / clip[3] * (width / 2) + width / 2 + cam.x_offset * s
    y = clip[1] / clip[3] * (height / 2) + height / 2 + cam.y_offset * s
    return x, y, clip[3]


FRONT = (-0.5, 0.5, -3.0)             # in front of the standard camera at (0.5, 1, 2) looking at the origin, and in view


def test_the_packer_places_the_light_on_the_level(api, native):
    from py_numpy_renderer_amd import LightShafts, _pack
    scene = scenes.cube_small(api)
    scene.add_light(api.Light(FRONT, ambient_strength=0.1, specular_strength=0.1))
    scene.camera.x_offset, scene.camera.y_offset = 3, -2
    for halvings in (1, 2):
        scene.light_shafts = LightShafts(light=1, density=0.9, samples=48, decay=0.9, intensity=0.3, threshold=0.125, halvings=halvings)
        for s, extra in ((1, 0), (2, 1), (4, 2)):
            scene.supersample = s
            lx, ly, t, g, step, n, d, w = _pack.light_shafts_constants(scene)
            x, y, clip_w = _hand_projection(scene, FRONT + (1.0,), s)
            assert clip_w > 0 and d == halvings + extra, "halvings + log2(supersample): the same share of the output resolution"
            assert lx == float(F32((x + 0.5) / 2 ** d - 0.5)) and ly == float(F32((y + 0.5) / 2 ** d - 0.5)), (s, lx, ly, x, y)
            hd, wd = native.shafts_level(s * scene.resolution[0], s * scene.resolution[1], d)
            assert -0.5 <= lx <= wd - 0.5 and -0.5 <= ly <= hd - 0.5, "the light is in view"
            assert (t, g, n) == (0.125, float(F32(0.3)), 48) and step == float(F32(np.float64(0.9) / 48))
            assert sf.bits(w, shafts_ref.weights(0.9, 48)) == 0 and w.dtype == np.float32 and len(w) == 48
            desc = native.fill_light_shafts_desc(lx, ly, t, g, step, n, d, w)
            assert (desc.light_x, desc.light_y, desc.samples, desc.halvings) == (lx, ly, 48, d) and list(desc.weights)[:48] == w.tolist() and not any(list(desc.weights)[48:])
    scene.supersample = 1
    # the grid is the un-jittered one: the private jitter of temporal_aa moves the frame's viewport and not the light
    still = _pack.light_shafts_constants(scene)[:2]
    scene.__dict__["_sample_jitter"] = (0.375, -0.25)
    assert _pack.sample_grid(scene, jittered=True)[3][3, 0] != _pack.sample_grid(scene)[3][3, 0]
    assert _pack.light_shafts_constants(scene)[:2] == still
    scene.__dict__.pop("_sample_jitter")
    # a directional light: the point at infinity it shines from
    sun = api.Light((0, 0, 0), light_type=api.Lightning.DIRECTIONAL_LIGHTNING, center=tuple(-np.asarray(FRONT)))
    scene.add_light(sun)
    scene.light_shafts = LightShafts(light=2)
    lx, ly = _pack.light_shafts_constants(scene)[:2]
    x, y, clip_w = _hand_projection(scene, FRONT + (0.0,), 1)
    assert clip_w > 0 and lx == float(F32((x + 0.5) / 4 - 0.5)) and ly == float(F32((y + 0.5) / 4 - 0.5))


def test_a_light_behind_the_camera_plane_has_no_position(api, native):
    from py_numpy_renderer_amd import LightShafts, _pack
    scene = scenes.cube_small(api)                       # its light, at (2, 3, 4), stands behind the camera at (0.5, 1, 2)
    scene.light_shafts = LightShafts()
    assert _hand_projection(scene, (2.0, 3.0, 4.0, 1.0), 1)[2] < 0
    assert _pack.light_shafts_constants(scene) is None
    scene.light = api.Light(tuple(np.asarray(scene.camera.position, dtype=np.float64).ravel()[:3]))      # in the camera's plane: w = 0
    assert _pack.light_shafts_constants(scene) is None
    scene.light = api.Light((float("nan"), 0.0, 0.0))
    assert _pack.light_shafts_constants(scene) is None
    values = native.DeviceRenderer._light_shafts_values(scene)
    assert values[0] == (0, 0.5, 0.9, 0.97, 64, 0.0, 2)
    scene.light_shafts = LightShafts(light=1)
    with pytest.raises(ValueError, match="light 1 does not exist"):
        _pack.light_shafts_constants(scene)
    with pytest.raises(ValueError, match="light 1 does not exist"):
        native.DeviceRenderer._light_shafts_values(scene)
    scene.light_shafts = None
    assert native.DeviceRenderer._light_shafts_values(scene) is None


@pytest.mark.parametrize("decay, samples", [(0.97, 64), (1.0, 128), (0.5, 128), (0.9, 1), (1e-3, 7)])
def test_the_weights_sum_to_one(decay, samples):
    from py_numpy_renderer_amd import _pack
    w = _pack.light_shafts_weights(decay, samples)
    assert w.dtype == np.float32 and w.shape == (samples,) and (w >= 0).all() and np.isfinite(w).all()
    assert sf.bits(w, shafts_ref.weights(decay, samples)) == 0
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= samples * 2.0 ** -25, "each weight is rounded once, by at most half a unit of 2^-24"
    assert (np.diff(w) <= 0).all() and w[0] == w.max()
