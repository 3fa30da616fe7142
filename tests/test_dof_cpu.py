"""CPU: ``Scene.depth_of_field`` without a device -- the host mirror ``mr_host_dof`` against the NumPy restatement
dof_ref.py (bit for bit), known answers on synthetic depth fields, and every refusal that needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import dof_ref
import post_fields
import scenes
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libmi355rast.so is not built: run __graft_entry__.build()")
    return _native


def _bits(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def _both(native, z, frame, m, kf, perspective, focus):
    """The mirror's frame, held to the reference's."""
    got = native.host_dof(z, frame, native.fill_dof_desc(m, kf, perspective, focus))
    assert _bits(got, dof_ref.apply(z, frame, m, kf, perspective, focus)) == 0
    return got


# ---------------------------------------------------------------------------- 1. the mirror against the reference
@pytest.fixture(scope="module")
def capture_cases(api):
    """(name, Z, F, map, kf, perspective, focus) of the committed captures test_ao_cpu.py takes, computed once."""
    from py_numpy_renderer_amd import DepthOfField, _pack
    cases = []
    for name, kw in (("diablo_small", {}), ("cube_small", dict(lens_radius=0.05)), ("torus_spot", dict(focus=3.0, lens_radius=0.1)),
                     ("tetra_ortho", dict(lens_radius=0.05))):
        data, _ = load_golden(name)
        scene = getattr(scenes, name)(api)
        scene.depth_of_field = DepthOfField(**kw)
        m, kf, perspective, focus = _pack.dof_constants(scene)
        cases.append((name, data["z"], np.ascontiguousarray(data["frame"], dtype=np.float32), m, kf, perspective, focus))
    return cases


def test_mirror_is_the_reference_on_the_captures(native, capture_cases):
    for name, z, frame, m, kf, perspective, focus in capture_cases:
        want = dof_ref.apply(z, frame, m, kf, perspective, focus)
        got = native.host_dof(z, frame, native.fill_dof_desc(m, kf, perspective, focus))
        s = dof_ref.circle(z, m, kf, perspective, focus)
        covered = np.isfinite(z)
        print(f"{name}: {_bits(got, want)} floats differ, {_bits(got, frame)} floats changed, kf {kf:.3f}, focus {focus:.3f}, "
              f"|s| of the covered samples in [{np.abs(s[covered]).min():.3f}, {np.abs(s[covered]).max():.3f}]")
        assert _bits(got, want) == 0, name
        assert _bits(got, frame) > 0, name
        assert perspective == (0 if name == "tetra_ortho" else 1)


@pytest.mark.parametrize("shape, seed", [((16, 16), 1), ((37, 41), 2), ((24, 40), 3)])
def test_mirror_is_the_reference_on_synthetic_depth_fields(native, shape, seed):
    """Hills with steps across the plane in focus, a patch that lies in it, holes of +inf, -inf and NaN; the map is a real
    Moebius map, so the float64 part of the definition is exercised too; kf small, middling and far beyond the clamp."""
    m, focus = post_fields.MOEBIUS, post_fields.HILLS_FOCUS
    z, frame = post_fields.dof_hills(shape, seed, m, focus)          # (the field lives in post_fields.py, for the kernel's tests too)
    low, high = [], []
    for kf, perspective in ((0.1, 1), (4.0, 1), (60.0, 1), (1.5, 0), (30.0, 0)):
        s = np.abs(dof_ref.circle(z, m, kf, perspective, focus))
        covered = np.isfinite(z)
        low.append(float(s[covered].min())), high.append(float(s[covered].max()))
        got = _both(native, z, frame, m, kf, perspective, focus)
        assert (_bits(got, frame) > 0) == (kf != 0.1), (shape, kf, perspective)      # kf 0.1: c < 0.5 everywhere, the sky too
        assert np.isfinite(got).all()
    print(f"{shape}: |s| of the covered samples from {min(low):.4f} to {max(high):.2f}")
    assert min(low) < 0.01 and max(high) > 2 * dof_ref.MAX_RADIUS, "the circles do not span 0 to beyond the clamp"


# ---------------------------------------------------------------------------- 2. known answers
IDENTITY = (1.0, 0.0, 0.0, 1.0)                  # e = float32(Z): the depth field is given directly
FOCUS = 16.0                                     # with kf = 1 and an orthographic camera s = Z - 16 exactly


@pytest.fixture(scope="module")
def colours():
    return np.random.default_rng(5).random((40, 48, 3), dtype=np.float32)


def test_a_plane_in_focus_is_returned_bit_for_bit(native, colours):
    z = np.full(colours.shape[:2], FOCUS)
    for kf, perspective in ((1.0, 0), (500.0, 0), (3.0, 1), (1e6, 1)):
        assert _bits(_both(native, z, colours, IDENTITY, kf, perspective, FOCUS), colours) == 0, (kf, perspective)


def test_one_bright_sample_on_a_black_plane_with_c_2(native):
    """c == 2: rr = 4, w = 0.25, thirteen samples to a disc.  W = 13 * 0.25 = 3.25 exactly wherever the disc lies inside
    the frame, so the bright sample, four samples from the nearest edges, becomes (0.25f * v) / 3.25f on its disc."""
    h, w, v = 20, 24, F32(0.7)
    z = np.full((h, w), FOCUS + 2.0)
    frame = np.zeros((h, w, 3), dtype=F32)
    frame[4, 5] = v
    got = _both(native, z, frame, IDENTITY, 1.0, 0, FOCUS)
    ys, xs = np.mgrid[0:h, 0:w]
    disc = (ys - 4) ** 2 + (xs - 5) ** 2 <= 4
    assert int(disc.sum()) == 13
    want = (F32(0.25) * v) / F32(3.25)
    assert _bits(got[disc], np.full((13, 3), want, dtype=F32)) == 0
    assert not got[~disc].any()


def test_a_sharp_foreground_keeps_every_sample_and_the_background_round_it_changes(native, colours):
    h, w = colours.shape[:2]
    z = np.full((h, w), FOCUS + 8.0)                                 # the background: c == 8
    fg = np.zeros((h, w), dtype=bool)
    fg[14:26, 18:32] = True
    z[fg] = FOCUS                                                    # in focus, 8 units in front of it
    got = _both(native, z, colours, IDENTITY, 1.0, 0, FOCUS)
    assert _bits(got[fg], colours[fg]) == 0, "a background's blur bled over the sharp foreground"
    ys, xs = np.mgrid[0:h, 0:w]
    dist2 = np.maximum(np.maximum(14 - ys, ys - 25), 0) ** 2 + np.maximum(np.maximum(18 - xs, xs - 31), 0) ** 2
    near = ~fg & (dist2 <= 64)
    changed = (got.view(np.uint32) != colours.view(np.uint32)).any(axis=-1)
    assert near.sum() > 100 and changed[near].all()
    # and the foreground's colours are not in it: a background sample is the mean of the BACKGROUND samples of its disc
    y, x = 20, 16                                                    # two samples left of the rectangle
    disc = ((ys - y) ** 2 + (xs - x) ** 2 <= 64) & ~fg
    assert np.allclose(got[y, x], colours[disc].mean(axis=0, dtype=np.float64), rtol=1e-5)


def test_a_blurred_foreground_spreads_over_the_sharp_background(native, colours):
    h, w = colours.shape[:2]
    z = np.full((h, w), FOCUS)                                       # the background, in focus
    fg = np.zeros((h, w), dtype=bool)
    fg[14:26, 18:32] = True
    z[fg] = FOCUS - 8.0                                              # in front of it: c == 8
    got = _both(native, z, colours, IDENTITY, 1.0, 0, FOCUS)
    changed = (got.view(np.uint32) != colours.view(np.uint32)).any(axis=-1)
    ys, xs = np.mgrid[0:h, 0:w]
    dist2 = np.maximum(np.maximum(14 - ys, ys - 25), 0) ** 2 + np.maximum(np.maximum(18 - xs, xs - 31), 0) ** 2
    assert changed[~fg & (dist2 <= 64)].all(), "a sharp background sample beside the blurred foreground kept its colour"
    assert not changed[~fg & (dist2 > 64)].any(), "the foreground reached further than its circle"
    # a background sample under a whole disc of the foreground keeps 4 / (4 + n / 64) of its own colour, n its disc's samples
    black = np.zeros_like(colours)
    black[20, 16] = 1.0
    alone = _both(native, z, black, IDENTITY, 1.0, 0, FOCUS)[20, 16, 0]
    n = int((fg & ((ys - 20) ** 2 + (xs - 16) ** 2 <= 64)).sum())
    assert n > 0 and np.isclose(alone, 4.0 / (4.0 + n / 64.0), rtol=1e-6)


def test_an_all_background_frame_under_perspective_is_a_uniform_blur(native):
    frame = np.random.default_rng(7).random((24, 28, 3), dtype=np.float32)
    ys, xs = np.mgrid[0:24, 0:28]
    for value in (np.inf, -np.inf, np.nan):
        for kf, radius in ((3.0, 3.0), (40.0, 16.0)):
            z = np.full((24, 28), value)
            got = _both(native, z, frame, IDENTITY, kf, 1, FOCUS)
            for y, x in ((0, 0), (12, 14), (23, 5)):
                disc = (ys - y) ** 2 + (xs - x) ** 2 <= radius * radius
                assert np.allclose(got[y, x], frame[disc].mean(axis=0, dtype=np.float64), rtol=2e-5), (value, kf, y, x)
    # under an orthographic camera the background's circle is +inf: the clamp
    got = _both(native, np.full((24, 28), np.inf), frame, IDENTITY, 0.001, 0, FOCUS)
    assert np.allclose(got[12, 14], frame[(ys - 12) ** 2 + (xs - 14) ** 2 <= 256].mean(axis=0, dtype=np.float64), rtol=2e-5)


# ---------------------------------------------------------------------------- 3. refusals and bindings, no device
def test_symbols_are_bound_and_the_abi_stays(native):
    lib = native.load_library()
    for name in ("mr_scene_set_depth_of_field", "mr_host_dof", "mr_debug_dof", "mr_debug_dof_times"):
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert lib.mr_abi_version() == native.ABI_VERSION == 4
    assert C.sizeof(native.DofDesc) == 6 * 8 + 8
    assert lib.mr_abi_struct_size(0) == C.sizeof(native.FrameDesc), "mr_frame_desc changed"
    assert lib.mr_abi_struct_size(6) == C.sizeof(native.AoDesc), "mr_ao_desc changed"
    header = open(os.path.join(ROOT, "include", "mi355rast.h")).read()
    assert "typedef struct mr_dof_desc" in header and "#define MR_ABI_VERSION 4" in header
    for line in ("double depth_map[4];", "double kf;", "double focus;", "int32_t perspective;"):
        assert line in header.split("typedef struct mr_dof_desc")[1].split("} mr_dof_desc;")[0]


def test_the_library_and_the_mirror_check_the_description(native):
    lib = native.load_library()
    handle = lib.mr_scene_create()

    def desc(m=IDENTITY, kf=2.0, perspective=1, focus=3.0):
        return native.fill_dof_desc(m, kf, perspective, focus)

    assert lib.mr_scene_set_depth_of_field(None, C.byref(desc())) == native.MR_E_INVALID
    assert lib.mr_scene_set_depth_of_field(handle, None) == 0                   # off, on a scene that never had it
    assert lib.mr_scene_set_depth_of_field(handle, C.byref(desc())) == 0        # (copied: no device is touched)
    bad = [("focus", dict(focus=0.0)), ("focus", dict(focus=-1.0)), ("focus", dict(focus=float("nan"))),
           ("focus", dict(focus=float("inf"))), ("focus", dict(focus=1e-46)), ("focus", dict(focus=1e39)),
           ("kf must", dict(kf=0.0)), ("kf must", dict(kf=-2.0)), ("kf must", dict(kf=float("nan"))),
           ("kf must", dict(kf=float("inf"))), ("kf must", dict(kf=1e-46)), ("kf must", dict(kf=1e39)),
           ("depth map", dict(m=(1.0, float("nan"), 0.0, 1.0))), ("depth map", dict(m=(float("inf"), 0.0, 0.0, 1.0))),
           ("perspective", dict(perspective=2)), ("perspective", dict(perspective=-1))]
    z, frame = np.full((4, 4), 2.0), np.ones((4, 4, 3), np.float32)
    for word, over in bad:
        d = desc(**over)
        assert lib.mr_scene_set_depth_of_field(handle, C.byref(d)) == native.MR_E_INVALID, over
        assert word.encode() in lib.mr_last_error(), (over, lib.mr_last_error())
        with pytest.raises(ValueError, match=word):
            native.host_dof(z, frame, d)
    assert lib.mr_scene_set_depth_of_field(handle, C.byref(desc(perspective=0))) == 0
    out = np.zeros(3, np.int32)
    assert lib.mr_debug_dof(handle, out.ctypes.data) == 0 and out.tolist() == [0, 0, 0]
    assert lib.mr_debug_dof(handle, None) == native.MR_E_INVALID
    ms = (C.c_float * 1)()
    assert lib.mr_debug_dof_times(handle, ms) == native.MR_E_INVALID            # no frame yet
    lib.mr_scene_destroy(handle)


def test_the_mirror_checks_its_arguments(native):
    lib = native.load_library()
    d = native.fill_dof_desc(IDENTITY, 2.0, 0, 3.0)
    z, frame = np.full((4, 4), 2.0), np.ones((4, 4, 3), np.float32)
    out = np.empty_like(frame)
    args = lambda **o: [o.get("z", z.ctypes.data), o.get("f", frame.ctypes.data), o.get("h", 4), o.get("w", 4), o.get("d", C.byref(d)),
                        o.get("out", out.ctypes.data)]
    assert lib.mr_host_dof(*args()) == 0
    for over in (dict(z=None), dict(f=None), dict(d=None), dict(out=None), dict(h=0), dict(w=-1), dict(h=40000),
                 dict(out=frame.ctypes.data)):                   # (not in place: neighbours' colours are read)
        assert lib.mr_host_dof(*args(**over)) == native.MR_E_INVALID, over
    with pytest.raises(ValueError, match="z must be"):
        native.host_dof(z, frame[:2], d)


def test_the_python_class_and_property(api):
    import py_numpy_renderer_amd as pkg
    from py_numpy_renderer_amd import DepthOfField, multigpu
    assert "DepthOfField" in pkg.__all__ and pkg.DepthOfField is DepthOfField
    dof = DepthOfField()
    assert (dof.focus, dof.lens_radius) == (None, 0.02)
    dof = DepthOfField(focus=3, lens_radius=0.5)
    assert (dof.focus, dof.lens_radius) == (3.0, 0.5) and "lens_radius=0.5" in repr(dof)
    with pytest.raises(AttributeError, match="read-only"):
        dof.focus = 1.0
    with pytest.raises(AttributeError, match="read-only"):
        dof.lens_radius = 1.0
    for kw in (dict(focus=0), dict(focus=-1), dict(focus=float("nan")), dict(focus=1e-46), dict(focus=1e39), dict(lens_radius=0),
               dict(lens_radius=-0.1), dict(lens_radius=float("inf")), dict(lens_radius=1e-46)):
        with pytest.raises(ValueError, match="depth of field"):
            DepthOfField(**kw)
    for kw in (dict(focus="2"), dict(lens_radius=True), dict(focus=[2.0]), dict(lens_radius=1j), dict(lens_radius=None)):
        with pytest.raises(TypeError, match="real number"):
            DepthOfField(**kw)
    scene = scenes.cube_small(api)
    assert scene.depth_of_field is None
    with pytest.raises(TypeError, match="DepthOfField"):
        scene.depth_of_field = 0.1
    scene.depth_of_field = dof
    assert scene.depth_of_field is dof
    with pytest.raises(ValueError, match="depth_of_field"):
        multigpu.BandRenderer(scene)                     # (refused before any device is asked for)
    scene.depth_of_field = None
    assert scene.depth_of_field is None


def test_the_description_of_a_view(api, native):
    """kf = float32(lens_radius * 0.5 * Hs * |P[1][1]| / focus) with Hs the sample grid's height; focus=None is the eye
    depth of the camera's center, per camera; the frame key carries the parameters."""
    from py_numpy_renderer_amd import DepthOfField, _pack
    scene = scenes.diablo_small(api, resolution=(30, 40))
    key_off = native.DeviceRenderer._frame_key(scene, True)
    scene.depth_of_field = DepthOfField(focus=2.5, lens_radius=0.03)
    key_on = native.DeviceRenderer._frame_key(scene, True)
    scene.depth_of_field = DepthOfField(focus=2.5, lens_radius=0.04)
    key_wider = native.DeviceRenderer._frame_key(scene, True)
    scene.depth_of_field = DepthOfField(lens_radius=0.04)
    assert len({key_off, key_on, key_wider, native.DeviceRenderer._frame_key(scene, True)}) == 4
    scene.depth_of_field = DepthOfField(focus=2.5, lens_radius=0.04)
    p11 = float(np.asarray(scene.camera.projection)[1, 1])
    for s in (1, 2, 4):
        scene.supersample = s
        m, kf, perspective, focus = _pack.dof_constants(scene)
        assert kf == float(np.float32(0.04 * 0.5 * (30 * s) * abs(p11) / 2.5)) and perspective == 1 and focus == 2.5
        assert m == _pack.depth_map(scene, scene.camera)
        d = native.fill_dof_desc(m, kf, perspective, focus)
        assert (tuple(d.depth_map), d.kf, d.focus, d.perspective) == (m, kf, focus, perspective)
    # focus=None follows the camera
    scene.supersample = 1
    scene.depth_of_field = DepthOfField(lens_radius=0.04)
    cam = scene.camera
    want = float(np.linalg.norm(np.asarray(cam.center, dtype=np.float64) - np.asarray(cam.position, dtype=np.float64)))
    m, kf, perspective, focus = _pack.dof_constants(scene)
    assert focus == want and kf == float(np.float32(0.04 * 0.5 * 30 * abs(p11) / want))
    other = api.Camera((0.5, 1, 2), (0.2, 0.5, -1.0), fovy=60, near=0.1, far=20, backface_culling=True)
    scene.camera = other
    far_focus = _pack.dof_constants(scene, other)[3]
    assert far_focus == float(np.linalg.norm(np.array([0.2, 0.5, -1.0]) - np.array([0.5, 1.0, 2.0]))) and far_focus != want
    ortho = scenes.tetra_ortho(api)
    ortho.depth_of_field = DepthOfField(lens_radius=0.05)
    m, kf, perspective, focus = _pack.dof_constants(ortho)
    p11 = float(np.asarray(ortho.camera.projection)[1, 1])
    assert perspective == 0 and kf == float(np.float32(0.05 * 0.5 * int(ortho.resolution[0]) * abs(p11) / focus))
