"""CPU: ``Scene.ambient_occlusion`` without a device -- the depth map, the host mirror ``mr_host_ao`` against the NumPy
restatement ao_ref.py (bit for bit), known answers on synthetic depth fields, and every refusal that needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import ao_ref
import post_fields
import scenes
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libmi355rast.so is not built: run __graft_entry__.build()")
    return _native


def _desc(native, m, k, perspective, **kw):
    from types import SimpleNamespace
    return native.fill_ao_desc(SimpleNamespace(**ao_ref.params(**kw)), m, k, perspective)


def _bits(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


# ---------------------------------------------------------------------------- 1. the depth map
def _forward(camera, z_e):
    """The chain of DESIGN.md section 6i from a point z_e on the view axis to the z-buffer's value, in float64."""
    P = np.asarray(camera.projection, dtype=np.float64)
    V = np.asarray(camera.viewport, dtype=np.float64)
    n, f = float(camera.near), float(camera.far)
    z_c = z_e * P[2, 2] + P[3, 2]
    w_c = z_e * P[2, 3] + P[3, 3]
    scr = (z_c / w_c) * V[2, 2] + V[3, 2]
    return 2 * n * f / ((f + n) - scr * (f - n))


def _back(m, z):
    return (m[0] * z + m[1]) / (m[2] * z + m[3])


def _entries(api):
    from py_numpy_renderer_amd.transformation import perspectives
    return [(sub, proj, system) for sub, by_proj in perspectives.items() for proj, by_sys in by_proj.items() for system in by_sys]


def _camera_for(api, sub, proj, system):
    """The cameras of tests/scenes.py: ``_std_cameras`` for a perspective entry, ``tetra_ortho``'s for the orthographic one."""
    if proj == api.PROJECTION_TYPE.ORTHOGRAPHIC:
        cam = api.Camera((0.5, 1, 2), (0, 0, 0), projection_type=proj, fovy=35, far=20, backface_culling=True)
    else:
        cam = scenes._std_cameras(api)[0]
    scene = api.Scene(cam, scenes._std_light(api), resolution=(120, 160), system=system, subsystem=sub)
    return scene, cam


def test_depth_map_round_trip_for_every_projection(api):
    from py_numpy_renderer_amd import _pack
    entries = _entries(api)
    assert len(entries) == 5
    rng = np.random.default_rng(11)
    for sub, proj, system in entries:
        scene, cam = _camera_for(api, sub, proj, system)
        depth = rng.uniform(float(cam.near), float(cam.far), 4096)
        z_e = depth if system == api.SYSTEM.LH else -depth           # in front of the camera: z_e < 0 right-handed, > 0 left-handed
        m = _pack.depth_map(scene, cam)
        got = _back(m, _forward(cam, z_e))
        worst = float(np.abs(got / depth - 1).max())
        print(f"{sub!r} {proj!r} {system!r}: m = {m}, worst relative error {worst:.3g}")
        assert (got > 0).all() and worst <= 1e-9


def test_depth_map_of_an_ill_conditioned_camera_is_finite_positive_and_monotone(api):
    """diablo_floor_lh_gl's camera, near 1e-4 and far 400: Z spans a narrow range for almost every depth.  No bound is set
    in advance; the worst error is printed (DESIGN.md section 6i quotes it)."""
    from py_numpy_renderer_amd import _pack
    scene = scenes.diablo_floor_lh_gl(api)
    cam = scene.camera
    depth = np.geomspace(float(cam.near) * 1.001, float(cam.far) * 0.999, 20001)
    m = _pack.depth_map(scene, cam)
    z = _forward(cam, depth)                                         # (left-handed: z_e > 0 in front)
    got = _back(m, z)
    print(f"diablo_floor_lh_gl: m = {m}, worst relative error {float(np.abs(got / depth - 1).max()):.3g} "
          f"(at depth {float(depth[np.abs(got / depth - 1).argmax()]):.4g}); between depth 0.5 and 50: "
          f"{float(np.abs(got / depth - 1)[(depth > 0.5) & (depth < 50)].max()):.3g}")
    assert np.isfinite(got).all() and (got > 0).all()
    assert (np.diff(got) > 0).all(), "not monotone"


def test_eye_depth_of_the_committed_capture(api):
    """diablo_small's z-buffer holds values near -0.0109 for geometry 1.62 to 3.16 units in front of the camera."""
    from py_numpy_renderer_amd import _pack
    data, _ = load_golden("diablo_small")
    scene = scenes.diablo_small(api)
    m = _pack.depth_map(scene, scene.camera)
    z = data["z"]
    covered = np.isfinite(z)
    e = ao_ref.eye_depth(z, m)
    assert covered.sum() > 1000 and np.array_equal(np.isfinite(e), covered)
    print(f"diablo_small: Z in [{z[covered].min():.6f}, {z[covered].max():.6f}] -> eye depth in [{e[covered].min():.4f}, {e[covered].max():.4f}]")
    assert 1.6 <= e[covered].min() and e[covered].max() <= 3.2
    # the capture's own matrices give the same map as the scene's camera
    assert np.allclose(data["host_viewport"][2:, 2], np.asarray(scene.camera.viewport)[2:, 2], rtol=0, atol=0)


# ---------------------------------------------------------------------------- 2. the mirror against the reference
@pytest.fixture(scope="module")
def capture_cases(api):
    """(name, Z, F, map, k, perspective, parameters) of the committed captures, computed once."""
    from py_numpy_renderer_amd import AmbientOcclusion, _pack
    cases = []
    for name, kw in (("diablo_small", {}), ("cube_small", dict(radius=0.2)), ("torus_spot", dict(radius=0.3, strength=2.0)),
                     ("tetra_ortho", dict(radius=0.25, depth_range=0.5, bias=0.0))):
        data, _ = load_golden(name)
        scene = getattr(scenes, name)(api)
        scene.ambient_occlusion = AmbientOcclusion(**kw)
        m, k, perspective = _pack.ao_constants(scene)
        cases.append((name, data["z"], np.ascontiguousarray(data["frame"], dtype=np.float32), m, k, perspective, kw))
    return cases


def test_mirror_is_the_reference_on_the_captures(native, capture_cases):
    for name, z, frame, m, k, perspective, kw in capture_cases:
        want = ao_ref.apply(z, frame, m, k, perspective, **ao_ref.params(**kw))
        got = native.host_ao(z, frame, _desc(native, m, k, perspective, **kw))
        changed = _bits(got, frame)
        print(f"{name}: {_bits(got, want)} floats differ, {changed} floats darkened")
        assert _bits(got, want) == 0, name
        assert perspective == (0 if name == "tetra_ortho" else 1)
        if name != "cube_small":                     # (a cube seen from outside has no crease)
            assert changed > 0, name


@pytest.mark.parametrize("shape, seed", [((16, 16), 1), ((37, 41), 2), ((24, 40), 3)])
def test_mirror_is_the_reference_on_synthetic_depth_fields(native, shape, seed):
    """Smooth hills with steps and holes, under a perspective and an orthographic footprint; the map is a real Moebius
    map, so the float64 part of the definition is exercised too."""
    m = post_fields.MOEBIUS
    z, frame = post_fields.ao_hills(shape, seed, m)                  # (the field lives in post_fields.py, for the kernel's tests too)
    for k, perspective, kw in ((9.0, 1, {}), (70.0, 1, dict(radius=0.5, strength=3.0)), (5.5, 0, dict(radius=0.2, bias=0.0)),
                               (0.25, 1, dict(strength=8.0, depth_range=10.0))):
        want = ao_ref.apply(z, frame, m, k, perspective, **ao_ref.params(**kw))
        got = native.host_ao(z, frame, _desc(native, m, k, perspective, **kw))
        assert _bits(got, want) == 0, (shape, k, perspective, kw)
        # (k = 70 clamps the footprint to 32 samples: in a frame 16 wide and high every pair then leaves the frame)
        assert (_bits(got, frame) > 0) == (not (shape == (16, 16) and k == 70.0)), (shape, k)
        hole = ~np.isfinite(z)
        assert _bits(got[hole], frame[hole]) == 0


# ---------------------------------------------------------------------------- 3. known answers
IDENTITY = (1.0, 0.0, 0.0, 1.0)                  # e = float32(Z): the depth field is given directly
STEP = dict(radius=0.25, strength=1.0)           # inv_fall 4, depth_range 0.75, bias 0.0234375: all exact in float32
K = 8.0                                          # orthographic footprint: dx = 8, 4, 6, 2, 0, -2, -6, -4 for the eight pairs


def _both(native, z, frame, m, k, perspective, **kw):
    got = native.host_ao(z, frame, _desc(native, m, k, perspective, **kw))
    assert _bits(got, ao_ref.apply(z, frame, m, k, perspective, **ao_ref.params(**kw))) == 0
    return got


@pytest.fixture(scope="module")
def colours():
    return np.random.default_rng(5).random((48, 64, 3), dtype=np.float32)


def test_planes_are_not_darkened(native, colours):
    ys, xs = np.mgrid[0:48, 0:64]
    flat = np.full((48, 64), 2.5)
    tilted_screen = 2.0 + xs / 64.0 + ys / 32.0                      # linear on the screen: c == 0 exactly
    tilted_world = (1.0 / (0.5 - xs / 512.0 - ys / 1024.0)).astype(np.float32).astype(np.float64)     # a plane under perspective: e convex
    for name, z in (("constant", flat), ("linear on the screen", tilted_screen), ("a plane under perspective", tilted_world)):
        for k, perspective in ((K, 0), (40.0, 1)):
            got = _both(native, z, colours, IDENTITY, k, perspective, **STEP)
            assert _bits(got, colours) == 0, (name, k, perspective)


def _step_field(height):
    z = np.full((48, 64), 2.0)
    z[:, 32:] = 2.0 + height
    return z


def test_a_step_darkens_its_far_side_to_the_formula(native, colours):
    got = _both(native, _step_field(0.125), colours, IDENTITY, K, 0, **STEP)
    dx = np.abs(np.rint(ao_ref.TAPS[:, 0] * np.float32(K))).astype(int)
    assert sorted(dx.tolist()) == [0, 2, 2, 4, 4, 6, 6, 8]
    occ = np.float32((0.125 - 0.0234375) * 4.0)                      # t of a pair one of whose taps crosses the step
    assert occ == np.float32(0.40625)
    inner = slice(8, 40)                                             # rows whose taps stay inside the frame
    assert _bits(got[inner, 8:32], colours[inner, 8:32]) == 0, "the near side was darkened"
    for d in range(0, 24):                                           # column 32 + d: d samples behind the step
        n = int((dx > d).sum())
        total = np.float32(0)
        for _ in range(n):
            total = np.float32(total + occ)
        ao = np.float32(1) - np.float32(1.0) * np.float32(total * np.float32(0.125))
        want = (colours[inner, 32 + d] * ao).astype(np.float32)
        assert _bits(got[inner, 32 + d], want) == 0, f"{d} samples behind the step: {n} pairs"
        assert (n > 0) == (d < 8)
    assert _bits(got[inner, 40:56], colours[inner, 40:56]) == 0, "darkened further than the footprint from the step"


def test_a_step_beyond_the_range_is_untouched(native, colours):
    got = _both(native, _step_field(1.0), colours, IDENTITY, K, 0, **STEP)
    assert _bits(got, colours) == 0


def test_background_only_is_untouched(native, colours):
    for value in (np.inf, -np.inf, np.nan):
        got = _both(native, np.full((48, 64), value), colours, IDENTITY, K, 0, **STEP)
        assert _bits(got, colours) == 0


def test_a_bias_no_pair_passes_leaves_the_frame_bit_for_bit(native, colours, capture_cases):
    got = _both(native, _step_field(0.125), colours, IDENTITY, K, 0, radius=0.25, bias=1e30)
    assert _bits(got, colours) == 0
    name, z, frame, m, k, perspective, _ = capture_cases[0]
    assert _bits(_both(native, z, frame, m, k, perspective, bias=1e30), frame) == 0


# ---------------------------------------------------------------------------- 4. teeth
def test_the_defaults_darken_a_fifth_of_diablo_small(capture_cases):
    name, z, frame, m, k, perspective, kw = capture_cases[0]
    assert name == "diablo_small" and kw == {}
    ao = ao_ref.factor(z, m, k, perspective, **ao_ref.params())
    covered = np.isfinite(z)
    share = float((ao[covered] < 1).mean())
    print(f"diablo_small, defaults: {share:.1%} of {int(covered.sum())} covered samples darkened, mean factor {float(ao[covered].mean()):.3f}")
    assert share >= 0.20
    assert (ao[~covered] == 1).all() and ao.min() >= 0


# ---------------------------------------------------------------------------- 5. refusals and bindings, no device
def test_symbols_are_bound_and_the_abi_stays(native):
    lib = native.load_library()
    for name in ("mr_scene_set_ambient_occlusion", "mr_host_ao", "mr_debug_ao", "mr_debug_ao_times"):
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert lib.mr_abi_version() == native.ABI_VERSION == 4
    assert lib.mr_abi_struct_size(6) == C.sizeof(native.AoDesc) == 9 * 8 + 8
    assert lib.mr_abi_struct_size(7) == -1
    assert lib.mr_abi_struct_size(0) == C.sizeof(native.FrameDesc), "mr_frame_desc changed"
    header = open(os.path.join(ROOT, "include", "mi355rast.h")).read()
    assert "typedef struct mr_ao_desc" in header and "#define MR_ABI_VERSION 4" in header


def test_the_library_checks_the_description(native):
    lib = native.load_library()
    handle = lib.mr_scene_create()
    good = dict(m=IDENTITY, k=8.0, perspective=1)

    def desc(**over):
        kw = dict(radius=0.1, strength=1.0, depth_range=0.3, bias=0.01)
        args = dict(good)
        for name in list(over):
            if name in args:
                args[name] = over.pop(name)
        kw.update(over)
        from types import SimpleNamespace
        return native.fill_ao_desc(SimpleNamespace(**kw), args["m"], args["k"], args["perspective"])

    assert lib.mr_scene_set_ambient_occlusion(None, C.byref(desc())) == native.MR_E_INVALID
    assert lib.mr_scene_set_ambient_occlusion(handle, None) == 0                # off, on a scene that never had it
    assert lib.mr_scene_set_ambient_occlusion(handle, C.byref(desc())) == 0     # (copied: no device is touched)
    bad = [("radius", dict(radius=0.0)), ("radius", dict(radius=-1.0)), ("radius", dict(radius=float("nan"))),
           ("radius", dict(radius=1e-46)), ("radius", dict(radius=1e39)),
           ("strength", dict(strength=0.0)), ("strength", dict(strength=8.5)), ("strength", dict(strength=float("inf"))),
           ("depth_range", dict(depth_range=0.0)), ("depth_range", dict(depth_range=float("inf"))),
           ("bias", dict(bias=-0.001)), ("bias", dict(bias=float("nan"))),
           ("k must", dict(k=0.0)), ("k must", dict(k=float("inf"))),
           ("depth map", dict(m=(1.0, float("nan"), 0.0, 1.0))), ("perspective", dict(perspective=2))]
    z, frame = np.full((4, 4), 2.0), np.ones((4, 4, 3), np.float32)
    for word, over in bad:
        d = desc(**over)
        assert lib.mr_scene_set_ambient_occlusion(handle, C.byref(d)) == native.MR_E_INVALID, over
        assert word.encode() in lib.mr_last_error(), (over, lib.mr_last_error())
        with pytest.raises(ValueError, match=word):
            native.host_ao(z, frame, d)
    assert lib.mr_scene_set_ambient_occlusion(handle, C.byref(desc(bias=0.0, strength=8.0))) == 0
    out = np.zeros(3, np.int32)
    assert lib.mr_debug_ao(handle, out.ctypes.data) == 0 and out.tolist() == [0, 0, 0]
    assert lib.mr_debug_ao(handle, None) == native.MR_E_INVALID
    ms = (C.c_float * 1)()
    assert lib.mr_debug_ao_times(handle, ms) == native.MR_E_INVALID             # no frame yet
    lib.mr_scene_destroy(handle)


def test_the_mirror_checks_its_arguments(native):
    lib = native.load_library()
    d = _desc(native, IDENTITY, 8.0, 0)
    z, frame = np.full((4, 4), 2.0), np.ones((4, 4, 3), np.float32)
    out = np.empty_like(frame)
    args = lambda **o: [o.get("z", z.ctypes.data), o.get("f", frame.ctypes.data), o.get("h", 4), o.get("w", 4), o.get("d", C.byref(d)),
                        o.get("out", out.ctypes.data)]
    assert lib.mr_host_ao(*args()) == 0
    for over in (dict(z=None), dict(f=None), dict(d=None), dict(out=None), dict(h=0), dict(w=-1), dict(h=40000)):
        assert lib.mr_host_ao(*args(**over)) == native.MR_E_INVALID, over
    with pytest.raises(ValueError, match="z must be"):
        native.host_ao(z, frame[:2], d)
    same = frame.copy()                                  # in place: out_frame may be the frame
    assert lib.mr_host_ao(z.ctypes.data, same.ctypes.data, 4, 4, C.byref(d), same.ctypes.data) == 0


def test_the_python_class_and_property(api):
    import py_numpy_renderer_amd as pkg
    from py_numpy_renderer_amd import AmbientOcclusion, multigpu
    assert "AmbientOcclusion" in pkg.__all__ and pkg.AmbientOcclusion is AmbientOcclusion
    ao = AmbientOcclusion()
    assert (ao.radius, ao.strength, ao.depth_range, ao.bias) == (0.1, 1.0, 3.0 * 0.1, 3.0 * 0.1 / 32.0)
    ao = AmbientOcclusion(radius=0.5, strength=2, depth_range=1.0, bias=0)
    assert (ao.radius, ao.strength, ao.depth_range, ao.bias) == (0.5, 2.0, 1.0, 0.0) and "radius=0.5" in repr(ao)
    with pytest.raises(AttributeError, match="read-only"):
        ao.radius = 1.0
    for kw in (dict(radius=0), dict(radius=-1), dict(radius=float("nan")), dict(radius=1e-46), dict(radius=1e39), dict(strength=0),
               dict(strength=8.5), dict(depth_range=0), dict(depth_range=float("inf")), dict(bias=-1e-3), dict(bias=float("nan"))):
        with pytest.raises(ValueError, match="ambient occlusion"):
            AmbientOcclusion(**kw)
    for kw in (dict(radius="0.1"), dict(strength=True), dict(bias=[0.1]), dict(depth_range=1j)):
        with pytest.raises(TypeError, match="real number"):
            AmbientOcclusion(**kw)
    scene = scenes.cube_small(api)
    assert scene.ambient_occlusion is None
    with pytest.raises(TypeError, match="AmbientOcclusion"):
        scene.ambient_occlusion = 0.1
    scene.ambient_occlusion = ao
    assert scene.ambient_occlusion is ao
    with pytest.raises(ValueError, match="ambient_occlusion"):
        multigpu.BandRenderer(scene)                     # (refused before any device is asked for)
    scene.ambient_occlusion = None
    assert scene.ambient_occlusion is None


def test_the_description_of_a_view(api, native):
    """k = float32(radius * 0.5 * Hs * |P[1][1]|) with Hs the sample grid's height; the frame key carries the parameters."""
    from py_numpy_renderer_amd import AmbientOcclusion, _pack
    scene = scenes.diablo_small(api, resolution=(30, 40))
    key_off = native.DeviceRenderer._frame_key(scene, True)
    scene.ambient_occlusion = AmbientOcclusion(radius=0.2)
    key_on = native.DeviceRenderer._frame_key(scene, True)
    scene.ambient_occlusion = AmbientOcclusion(radius=0.2, strength=2.0)
    assert len({key_off, key_on, native.DeviceRenderer._frame_key(scene, True)}) == 3
    p11 = float(np.asarray(scene.camera.projection)[1, 1])
    for s in (1, 2, 4):
        scene.supersample = s
        m, k, perspective = _pack.ao_constants(scene)
        assert k == float(np.float32(0.2 * 0.5 * (30 * s) * abs(p11))) and perspective == 1
        assert m == _pack.depth_map(scene, scene.camera)
    ortho = scenes.tetra_ortho(api)
    ortho.ambient_occlusion = AmbientOcclusion()
    assert _pack.ao_constants(ortho)[2] == 0
