"""CPU: ``Scene.motion_blur`` without a device -- the host mirrors ``mr_host_velocity`` and ``mr_host_motion_blur`` against
the NumPy restatement motion_ref.py (bit for bit), known answers on synthetic fields, the reprojection that anchors
``_pack.motion_matrices``, the previous state's bookkeeping, and every refusal that needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_fields as mf
import motion_ref
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libmi355rast.so is not built: run __graft_entry__.build()")
    return _native


def _both(native, field):
    """The mirrors' (U, F'), held to the reference's."""
    u, f = field.mirror(native)
    want_u, want_f = field.reference()
    assert mf.bits(u, want_u) == 0, f"{field!r}: {mf.bits(u, want_u)} velocity floats differ"
    assert mf.bits(f, want_f) == 0, f"{field!r}: {mf.bits(f, want_f)} floats differ"
    return u, f


# ---------------------------------------------------------------------------- 1. the mirrors against the reference
@pytest.mark.parametrize("size", mf.CPU_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mirrors_are_the_reference_on_every_field(native, size):
    moved = 0
    for field in mf.gpu_cases(size):
        u, f = _both(native, field)
        assert np.isfinite(u).all() and np.isfinite(f).all()
        moved += mf.bits(f, field.frame)
    assert moved > 0 or size == (1, 1)


# ---------------------------------------------------------------------------- 2. known answers
def test_a_shift_by_three_is_exact_on_finite_and_background_samples(native):
    """T and B under which every sample was 3 columns further right: U == (-3, 0), exactly.  Z is a power of two here, so
    that x * Z, y * Z and the quotients are exact; at any other Z the moving component is still exactly -3 (the float64
    error of (x Z + 3 Z) / Z is far below float32's step at 3) and the other one is y - (y Z) / Z, zero or an ulp of y."""
    rng = np.random.default_rng(8)
    z = np.where(rng.random((33, 65)) < 0.2, np.inf, np.where(rng.random((33, 65)) < 0.5, -0.5, 4.0))
    winner = np.where(np.isfinite(z), 0, -1)
    field = mf.Field("shift3", z, winner, rng.random((33, 65, 3), dtype=np.float32), face_off=(0,), class_of_model=(0,),
                     matrices=(mf.shift_t(-3.0, 0.0),), background=mf.shift_b(-3.0, 0.0), m=mf.IDENTITY)
    assert not np.isfinite(field.z).all() and np.isfinite(field.z).any()
    u, _ = _both(native, field)
    assert (u[..., 0] == F32(-3)).all() and (u[..., 1] == 0).all()
    u, _ = _both(native, mf.uniform((33, 65), (-3.0, 0.0)))            # the hills' Z, holes and all
    assert (u[..., 0] == F32(-3)).all() and np.abs(u[..., 1]).max() < 1e-13


def test_identity_motion_is_at_rest_and_returns_the_frame(native):
    field = mf.at_rest((33, 65))
    u, f = _both(native, field)
    h = motion_ref.segment(u, field.shutter)[0]
    assert not h.any() and mf.bits(f, field.frame) == 0


def test_less_than_half_a_sample_is_at_rest_and_more_is_not(native):
    for length, at_rest in ((0.49, True), (0.51, False)):
        for direction in mf.COMPASS[:3]:
            field = mf.uniform((20, 24), (length * direction[0], length * direction[1]))
            u, f = _both(native, field)
            h = motion_ref.segment(u, 1.0)[0]
            assert (not h.any()) == at_rest, (length, direction)
            assert (mf.bits(f, field.frame) == 0) == at_rest, (length, direction)
    # the shutter scales it: 0.9 sample at shutter 0.5 is 0.45
    field = mf.uniform((20, 24), (0.9, 0.0), shutter=0.5)
    assert mf.bits(_both(native, field)[1], field.frame) == 0


def test_one_bright_sample_spreads_over_nine_samples_of_its_row(native):
    """U = (8, 0), shutter 1: h = 4, the segment covers along = -4 .. 4, w = 1 / 9 everywhere and W is nine adds of it.
    Every one of the nine outputs is (w v) / W: nine roundings in W, one in the product, one in the quotient, so each is v
    / 9 to within 11 half-steps and the frame's sum (taken in float64) is v to within 11 * 2^-24 * v."""
    h, w, v = 9, 40, F32(0.7)
    z, winner, frame = mf.plane((h, w), 1)
    frame[:] = 0
    frame[4, 20] = v
    field = mf.Field("bright", z, winner, frame, face_off=(0,), class_of_model=(0,), matrices=(mf.shift_t(8.0, 0.0),))
    u, f = _both(native, field)
    assert (u[..., 0] == F32(8)).all() and np.abs(u[..., 1]).max() < 1e-13
    lit = f[..., 0] != 0
    assert lit.sum() == 9 and lit[4, 16:25].all()
    for ch in range(3):
        assert abs(float(f[..., ch].sum(dtype=np.float64)) - float(v)) <= 11 * 2.0 ** -24 * float(v)


def _two_layers(fg_u, bg_u, seed=3):
    """A foreground rectangle (model 1, nearer) over a background plane (model 0), each with its own motion."""
    shape = (40, 56)
    rng = np.random.default_rng(seed)
    fg = np.zeros(shape, dtype=bool)
    fg[12:28, 20:36] = True
    depth = np.where(fg, 1.5, 3.0)
    import post_fields
    z = post_fields.z_of(depth, mf.MOEBIUS)
    winner = np.where(fg, 2, 0).astype(np.int32)
    frame = rng.random(shape + (3,), dtype=np.float32)
    field = mf.Field("layers", z, winner, frame, face_off=(0, 2), class_of_model=(1, 2),
                     matrices=(mf.IDENTITY_T, mf.shift_t(*bg_u), mf.shift_t(*fg_u)))
    return field, fg


def test_a_still_foreground_in_front_of_a_moving_background_keeps_its_bits(native):
    field, fg = _two_layers(fg_u=(0.0, 0.0), bg_u=(12.0, 5.0))
    _, f = _both(native, field)
    changed = (f.view(np.uint32) != field.frame.view(np.uint32)).any(axis=-1)
    assert not changed[fg].any(), "a moving background smeared over the still foreground"
    assert changed[~fg].all()


def test_a_background_sample_beside_a_moving_foreground_changes(native):
    field, fg = _two_layers(fg_u=(10.0, 0.0), bg_u=(0.0, 0.0))
    _, f = _both(native, field)
    changed = (f.view(np.uint32) != field.frame.view(np.uint32)).any(axis=-1)
    # the foreground's segments reach h = 5 samples along x: the background left and right of it, on its rows
    assert changed[12:28, 15:20].all() and changed[12:28, 36:41].all()
    assert not changed[:11].any() and not changed[29:].any() and not changed[:, :14].any() and not changed[:, 42:].any()


def test_the_interior_of_a_uniformly_moving_object_is_the_box_mean_along_d(native):
    field = mf.Field("box", *mf.plane((24, 60), 5), face_off=(0,), class_of_model=(0,), matrices=(mf.shift_t(8.0, 0.0),))
    _, f = _both(native, field)
    for y, x in ((3, 10), (12, 30), (20, 50)):
        assert np.allclose(f[y, x], field.frame[y, x - 4:x + 5].mean(axis=0, dtype=np.float64), rtol=2e-6), (y, x)
    field = mf.Field("box_y", *mf.plane((60, 24), 6), face_off=(0,), class_of_model=(0,), matrices=(mf.shift_t(0.0, -12.0),))
    _, f = _both(native, field)
    assert np.allclose(f[30, 7], field.frame[24:37, 7].mean(axis=0, dtype=np.float64), rtol=2e-6)


# ---------------------------------------------------------------------------- 3. the reprojection: _pack.motion_matrices
def _screen(scene, world, pose=None):
    """(x, y, Z, w) of world points (N, 4) through the package's own camera and viewport and upstream's linearize_z."""
    from py_numpy_renderer_amd import _pack
    cam = scene.camera
    pts = world if pose is None else world @ pose
    clip = pts @ np.asarray(cam.MVP, dtype=np.float64)
    w = clip[:, 3]
    scr = (clip / w[:, None]) @ np.asarray(_pack.sample_grid(scene)[3], dtype=np.float64)
    n, f = float(cam.near), float(cam.far)
    return scr[:, 0], scr[:, 1], 2 * n * f / ((f + n) - scr[:, 2] * (f - n)), w


def _reprojection_error(scene, world, model, state_a, state_b):
    """Largest distance, in samples, between where T says the points of state B were and where state A puts them."""
    from py_numpy_renderer_amd import _pack
    (cam_a, pose_a), (cam_b, pose_b) = state_a, state_b
    scene.camera, scene.models[model].pose = cam_a, pose_a
    xa, ya, _, wa = _screen(scene, world, scene.models[model].pose)
    previous = _pack.MotionState(scene)
    scene.camera, scene.models[model].pose = cam_b, pose_b
    xb, yb, zb, wb = _screen(scene, world, scene.models[model].pose)
    _, T, _, class_of, _ = _pack.motion_matrices(scene, previous)
    moved = not (pose_a is pose_b or (pose_a is not None and pose_b is not None and np.array_equal(pose_a, pose_b)))
    assert (class_of[model] != 0) == moved and len(T) == 1 + int(moved)
    t = T[class_of[model]]
    u = np.stack([xb * zb, yb * zb, zb, np.ones_like(zb)], axis=1) @ t
    seen = (wa > 0) & (wb > 0)
    assert seen.sum() >= 8 and (u[seen, 2] * zb[seen] > 0).all(), "a point in front of both cameras fails the kernel's test"
    return float(np.hypot(u[seen, 0] / u[seen, 2] - xa[seen], u[seen, 1] / u[seen, 2] - ya[seen]).max())


REPROJECTION_MEASURED = 4.7e-12        # samples: the largest error the cases below give (4.674e-12, printed by the test)


def test_the_matrices_land_on_the_previous_screen_position(api):
    """Mesh vertices (cube.obj) and a plane parallel to the image, pushed through camera, viewport and linearize_z under
    state A and under state B; T applied to B's (x Z, y Z, Z, 1) must land on A's screen position.  Perspective and
    orthographic cameras, right- and left-handed, a viewport offset, supersampling, a model with two poses.  The bound is
    16 times the largest error measured here on the CPU -- 4.674e-12 sample (REPROJECTION_MEASURED; deterministic float64
    arithmetic), so 7.5e-11 -- far below the 1e-3 sample that would show in a 16-sample blur."""
    from py_numpy_renderer_amd import rotate_xyz, translation
    bound = 16 * REPROJECTION_MEASURED
    assert bound < 1e-3
    worst = 0.0
    cube = np.asarray(api.Model.load_model(os.path.join(scenes.ASSETS, "cube", "cube.obj")).vertices, dtype=np.float64) * 0.45
    pose_1 = np.asarray(rotate_xyz((20.0, -10.0, 35.0)), dtype=np.float64) @ np.asarray(translation((0.1, 0.05, -0.2)), dtype=np.float64)
    pose_2 = np.asarray(rotate_xyz((-15.0, 25.0, 5.0)), dtype=np.float64) @ np.asarray(translation((-0.2, 0.1, 0.15)), dtype=np.float64)
    recipes = [("rh_dx", scenes.cube_outward, dict(), 1, (0, 0)), ("lh_gl", scenes.diablo_floor_lh_gl, dict(), 1, (0, 0)),
               ("ortho", scenes.tetra_ortho, dict(projection_type=api.PROJECTION_TYPE.ORTHOGRAPHIC), 1, (0, 0)),
               ("offset_ss2", scenes.cube_outward, dict(), 2, (13, -7))]
    for name, recipe, extra, ss, offsets in recipes:
        scene = recipe(api, resolution=(136, 152))
        scene.supersample = ss
        base = scene.camera
        kw = dict(fovy=base.fovy, near=0.1 if "projection_type" not in extra else None, far=base.far, backface_culling=True, **extra)
        if kw["near"] is None:
            del kw["near"]

        def camera(position, center):
            cam = api.Camera(position, center, **kw)
            cam.scene = scene
            cam.x_offset, cam.y_offset = offsets
            return cam

        cam_a = camera((0.5, 1.0, 2.0), (0, 0, 0))
        cam_b = camera((0.7, 0.9, 1.8), (0.1, 0.0, -0.1))
        # a plane parallel to B's image: constant eye depth, spread over the view
        g = np.linspace(-0.6, 0.6, 7)
        depth = -1.5 if int(scene.system) == int(api.SYSTEM.RH) else 1.5
        eye = np.array([[x, y, depth, 1.0] for x in g for y in g])
        plane = eye @ np.linalg.inv(np.asarray(cam_b.lookat, dtype=np.float64))
        for what, world in (("cube", cube), ("plane", plane)):
            for states in (((cam_a, None), (cam_b, None)), ((cam_a, pose_1), (cam_a, pose_2)), ((cam_a, None), (cam_b, pose_1)),
                           ((cam_a, pose_2), (cam_b, pose_2))):
                err = _reprojection_error(scene, world, 0, *states)
                worst = max(worst, err)
                assert err <= bound, (name, what, err)
        scene.models[0].pose = None
    print(f"largest reprojection error: {worst:.3e} sample (bound {bound:.3e})")


def test_a_sky_moves_under_a_rotating_camera_and_not_under_a_translating_one(api):
    """The background's matrix B: samples no face covers lie at infinity under a perspective camera."""
    from py_numpy_renderer_amd import _pack
    scene = scenes.cube_outward(api, resolution=(136, 152))
    kw = dict(fovy=60, near=0.1, far=20, backface_culling=True)

    def camera(position, center):
        cam = api.Camera(position, center, **kw)
        cam.scene = scene
        return cam

    ys, xs = np.mgrid[0:136:9, 0:152:9]
    rows = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)], axis=1).astype(np.float64)
    scene.camera = camera((0.5, 1.0, 2.0), (0.0, 0.0, 0.0))
    previous = _pack.MotionState(scene)
    scene.camera = camera((1.0, 1.3, 2.4), (0.5, 0.3, 0.4))            # the same direction of view, another place
    u = rows @ _pack.motion_matrices(scene, previous)[2]
    assert (u[:, 2] > 0).all() and np.abs(u[:, :2] / u[:, 2:] - rows[:, :2]).max() < 1e-9
    scene.camera = camera((0.5, 1.0, 2.0), (0.3, 0.0, 0.0))            # the same place, turned
    b = _pack.motion_matrices(scene, previous)[2]
    u = rows @ b
    moved = u[:, :2] / u[:, 2:] - rows[:, :2]
    assert (u[:, 2] > 0).all() and np.abs(moved).max() > 3
    # a direction of the world, seen by both: B takes its sample of this frame to its sample of the previous one
    d = np.array([[0.1, -0.2, -1.0, 0.0], [-0.3, -0.4, -1.0, 0.0]])
    now, before = d @ _pack.MotionState(scene).S, d @ previous.S
    assert (now[:, 3] > 0).all() and (before[:, 3] > 0).all()
    got = np.stack([now[:, 0] / now[:, 3], now[:, 1] / now[:, 3], np.ones(2)], axis=1) @ b
    assert np.abs(got[:, :2] / got[:, 2:] - before[:, :2] / before[:, 3:]).max() < 1e-8


# ---------------------------------------------------------------------------- 4. the previous state (no device)
def test_the_previous_state_follows_the_frames_issued(api, native):
    from py_numpy_renderer_amd import MotionBlur, translation
    scene = scenes.cube_outward(api, resolution=(30, 40))
    issue = lambda: native.DeviceRenderer.issue_motion(None, scene)
    frame = lambda: scene.__dict__.get("_motion_frame")
    issue()
    assert frame() is None and native.DeviceRenderer._motion_values(scene) is None
    key_off = native.DeviceRenderer._frame_key(scene, True)
    scene.motion_blur = MotionBlur(shutter=0.75)
    issue()
    first = frame()
    assert first[0] == 0.75 and native.DeviceRenderer._frame_key(scene, True) != key_off
    identity = np.frombuffer(first[2], dtype=np.float64).reshape(-1, 4, 3)
    assert len(identity) == 1 and np.array_equal(identity[0], mf.IDENTITY_T)
    assert np.array_equal(np.frombuffer(first[3], dtype=np.float64).reshape(3, 3), np.eye(3))
    issue()
    assert frame() == first, "nothing moved: the second frame's motion is the identity too"
    scene.models[0].pose = np.asarray(translation((0.1, 0.0, 0.0)), dtype=np.float64)
    issue()
    moved = frame()
    assert moved != first and np.frombuffer(moved[4], dtype=np.int32).tolist() == [1, 0]
    assert native.DeviceRenderer._frame_key(scene, True) != key_off
    issue()
    assert frame() == first, "the pose stayed: class 0 again"
    cam = api.Camera((0.6, 1, 2), (0, 0, 0), fovy=60, near=0.1, far=20, backface_culling=True)
    scene.camera = cam
    issue()
    panned = frame()
    assert panned != first and np.frombuffer(panned[4], dtype=np.int32).tolist() == [0, 0]
    # a frame rendered again after an overflow takes its first attempt's matrices and leaves the previous state alone
    state = scene.__dict__["_motion_prev"]
    scene.__dict__["_motion_replay"] = moved
    issue()
    assert frame() == moved and scene.__dict__["_motion_prev"] is state
    del scene.__dict__["_motion_replay"]
    # reset_motion, a new MotionBlur and another model list all forget the previous state
    scene.camera = api.Camera((0.7, 1, 2), (0, 0, 0), fovy=60, near=0.1, far=20, backface_culling=True)
    scene.reset_motion()
    issue()
    assert frame() == first
    scene.camera = cam
    scene.motion_blur = MotionBlur(shutter=0.75)
    issue()
    assert frame() == first
    scene.camera = api.Camera((0.7, 1, 2), (0, 0, 0), fovy=60, near=0.1, far=20, backface_culling=True)
    scene.models.append(scene.models.pop(0))                         # the same models in another order: another list
    issue()
    assert frame() == first
    # a singular pose falls back to class 0
    scene.models[0].pose = np.diag([1.0, 1.0, 0.0, 1.0])
    issue()
    assert np.frombuffer(frame()[4], dtype=np.int32).tolist() == [0, 0]
    scene.motion_blur = None
    issue()
    assert frame() is None and native.DeviceRenderer._motion_values(scene) is None


# ---------------------------------------------------------------------------- 5. refusals and bindings, no device
def test_symbols_are_bound(native):
    lib = native.load_library()
    for name in ("mr_scene_set_motion_blur", "mr_host_velocity", "mr_host_motion_blur", "mr_read_velocity", "mr_debug_motion",
                 "mr_debug_motion_times", "mr_debug_motion_post"):
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert C.sizeof(native.MotionDesc) == 4 * 8 + 8 + 8 + 9 * 8 + 8 + 8
    header = open(os.path.join(ROOT, "include", "mi355rast.h")).read()
    body = header.split("typedef struct mr_motion_desc")[1].split("} mr_motion_desc;")[0]
    for line in ("double depth_map[4];", "double shutter;", "const double *matrices;", "double background[9];",
                 "const int32_t *class_of_model;", "int32_t n_classes, n_models;"):
        assert line in body
    # mr_debug_post keeps its signature
    assert "const mr_ao_desc *ao, int32_t ao_shape, const mr_dof_desc *dof, int32_t dof_shape, const double *weights" in header


def _scene_with_models(native, n):
    """A library scene of *n* one-triangle models (host arrays only: no device is touched)."""
    lib = native.load_library()
    handle = lib.mr_scene_create()
    verts = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1]], dtype=np.float32)
    faces = np.zeros((1, 3, 4), dtype=np.int32)
    faces[0, :, 0] = (0, 1, 2)
    mat = native.MaterialDesc()
    mat.tex_kd = mat.tex_norm = mat.tex_ks = -1
    for _ in range(n):
        d = native.ModelDesc()
        d.vertices, d.faces, d.materials = verts.ctypes.data, faces.ctypes.data, C.pointer(mat)
        d.n_vertices, d.n_faces, d.n_materials, d.vertices_are_f32, d.clip, d.depth_test = 3, 1, 1, 1, 1, 1
        assert lib.mr_scene_add_model(handle, C.byref(d)) >= 0, lib.mr_last_error()
    return lib, handle


def test_the_library_and_the_mirrors_check_the_description(native):
    lib, handle = _scene_with_models(native, 2)
    nan, inf = float("nan"), float("inf")

    def desc(shutter=0.5, matrices=(mf.IDENTITY_T, mf.shift_t(1, 2)), background=mf.IDENTITY_B, classes=(0, 1), m=mf.MOEBIUS):
        return native.fill_motion_desc(m, shutter, matrices, background, classes)

    assert lib.mr_scene_set_motion_blur(None, C.byref(desc())) == native.MR_E_INVALID
    assert lib.mr_scene_set_motion_blur(handle, None) == 0                      # off, on a scene that never had it
    assert lib.mr_scene_set_motion_blur(handle, C.byref(desc())) == 0, lib.mr_last_error()          # (copied: no device is touched)
    bad_t = mf.shift_t(1, 2)
    bad_t[3, 1] = nan
    bad_b = mf.IDENTITY_B.copy()
    bad_b[0, 2] = inf
    bad = [("shutter", dict(shutter=0.0)), ("shutter", dict(shutter=-0.5)), ("shutter", dict(shutter=1.0000001)), ("shutter", dict(shutter=nan)),
           ("shutter", dict(shutter=inf)), ("shutter", dict(shutter=1e-46)), ("shutter", dict(shutter=2.0)),
           ("matrix entry", dict(matrices=(mf.IDENTITY_T, bad_t))), ("matrix entry", dict(background=bad_b)),
           ("depth map", dict(m=(1.0, nan, 0.0, 1.0))), ("class is out of range", dict(classes=(0, 2))),
           ("class is out of range", dict(classes=(-1, 0)))]
    z, winner, frame = np.full((4, 4), 2.0), np.zeros((4, 4), np.int32), np.ones((4, 4, 3), np.float32)
    for word, over in bad:
        d = desc(**over)
        assert lib.mr_scene_set_motion_blur(handle, C.byref(d)) == native.MR_E_INVALID, over
        assert word.encode() in lib.mr_last_error(), (over, lib.mr_last_error())
        with pytest.raises(ValueError, match=word):
            native.host_velocity(z, winner, (0, 1), d)
    assert lib.mr_scene_set_motion_blur(handle, C.byref(desc(shutter=1.0))) == 0    # the closed end of (0, 1]
    for classes in ((0,), (0, 1, 0)):                                 # n_models other than the scene's
        assert lib.mr_scene_set_motion_blur(handle, C.byref(desc(classes=classes))) == native.MR_E_INVALID
        assert b"n_models" in lib.mr_last_error()
    out = np.zeros(3, np.int32)
    assert lib.mr_debug_motion(handle, out.ctypes.data) == 0 and out.tolist() == [0, 0, 0]
    assert lib.mr_debug_motion(handle, None) == native.MR_E_INVALID
    ms = (C.c_float * 2)()
    assert lib.mr_debug_motion_times(handle, ms) == native.MR_E_INVALID         # no frame yet
    vel = np.zeros((4, 4, 2), np.float32)
    assert lib.mr_read_velocity(handle, vel.ctypes.data) == native.MR_E_INVALID and b"nothing rendered" in lib.mr_last_error()
    # partial frames and sub-frames of an accumulation are refused by the rendering entry points, before any device work
    fr = native.FrameDesc()
    fr.width, fr.height, fr.system, fr.row_begin, fr.row_end = 8, 8, 1, 0, 4
    rgb = np.zeros((8, 8, 3), np.uint8)
    assert lib.mr_render(handle, C.byref(fr), rgb.ctypes.data, None) == native.MR_E_INVALID and b"motion blur takes whole frames" in lib.mr_last_error()
    fr.row_end, fr.stripe_count, fr.stripe_index = 8, 2, 0
    assert lib.mr_render_device(handle, C.byref(fr), C.c_void_p(rgb.ctypes.data), None) == native.MR_E_INVALID
    assert b"motion blur takes whole frames" in lib.mr_last_error()
    fr.stripe_count = 0
    assert lib.mr_accum_add(handle, C.byref(fr), 1.0) == native.MR_E_INVALID and b"motion blur is not available" in lib.mr_last_error()
    lib.mr_scene_destroy(handle)


def test_the_mirrors_check_their_arguments(native):
    lib = native.load_library()
    d = native.fill_motion_desc(mf.IDENTITY, 0.5, (mf.IDENTITY_T,), mf.IDENTITY_B, (0,))
    z, winner, frame = np.full((4, 4), 2.0), np.zeros((4, 4), np.int32), np.ones((4, 4, 3), np.float32)
    off = np.zeros(1, np.int32)
    vel, out = np.zeros((4, 4, 2), np.float32), np.empty_like(frame)
    v_args = lambda **o: [o.get("z", z.ctypes.data), o.get("win", winner.ctypes.data), o.get("off", off.ctypes.data), o.get("h", 4), o.get("w", 4),
                          o.get("d", C.byref(d)), o.get("out", vel.ctypes.data)]
    assert lib.mr_host_velocity(*v_args()) == 0
    for over in (dict(z=None), dict(win=None), dict(off=None), dict(d=None), dict(out=None), dict(h=0), dict(w=-1), dict(h=40000)):
        assert lib.mr_host_velocity(*v_args(**over)) == native.MR_E_INVALID, over
    descending = np.array([3], np.int32)
    assert lib.mr_host_velocity(*v_args(off=descending.ctypes.data)) == native.MR_E_INVALID and b"ascend from 0" in lib.mr_last_error()
    b_args = lambda **o: [o.get("z", z.ctypes.data), o.get("vel", vel.ctypes.data), o.get("f", frame.ctypes.data), o.get("h", 4), o.get("w", 4),
                          o.get("d", C.byref(d)), o.get("out", out.ctypes.data)]
    assert lib.mr_host_motion_blur(*b_args()) == 0
    for over in (dict(z=None), dict(vel=None), dict(f=None), dict(d=None), dict(out=None), dict(h=0), dict(w=-1), dict(w=40000),
                 dict(out=frame.ctypes.data)):                   # (not in place: neighbours' colours are read)
        assert lib.mr_host_motion_blur(*b_args(**over)) == native.MR_E_INVALID, over
    with pytest.raises(ValueError, match="z and winner must be"):
        native.host_velocity(z, winner[:2], (0,), d)
    with pytest.raises(ValueError, match="first faces"):
        native.host_velocity(z, winner, (0, 1), d)
    # mr_debug_motion_post refuses before it asks for a device
    handle = lib.mr_scene_create()
    with pytest.raises(ValueError, match="shape"):
        native.debug_motion_post(handle, z, winner, frame, (0,), d, shape=7)
    lib.mr_scene_destroy(handle)


def test_the_python_class_and_property(api):
    import py_numpy_renderer_amd as pkg
    from py_numpy_renderer_amd import MotionBlur, multigpu
    assert "MotionBlur" in pkg.__all__ and pkg.MotionBlur is MotionBlur
    assert MotionBlur().shutter == 0.5
    mb = MotionBlur(shutter=1)
    assert mb.shutter == 1.0 and "shutter=1.0" in repr(mb)
    with pytest.raises(AttributeError, match="read-only"):
        mb.shutter = 0.25
    for shutter in (0, -0.5, 1.0000001, 2, float("nan"), float("inf"), 1e-46):
        with pytest.raises(ValueError, match="motion blur"):
            MotionBlur(shutter=shutter)
    for shutter in ("0.5", True, [0.5], 1j, None):
        with pytest.raises(TypeError, match="real number"):
            MotionBlur(shutter=shutter)
    scene = scenes.cube_small(api)
    assert scene.motion_blur is None
    with pytest.raises(TypeError, match="MotionBlur"):
        scene.motion_blur = 0.5
    scene.motion_blur = mb
    assert scene.motion_blur is mb
    with pytest.raises(ValueError, match="motion_blur"):
        multigpu.BandRenderer(scene)                     # (refused before any device is asked for)
    with pytest.raises(ValueError, match="accumulate"):
        scene.accumulate()
    with pytest.raises(ValueError, match="accumulate"):
        scene.render_mean(4, lambda k: None)
    scene.motion_blur = None
    assert scene.motion_blur is None
    scene.accumulate().close()


def test_partial_frames_and_open_accumulations_are_refused_before_the_device(api, native):
    from py_numpy_renderer_amd import MotionBlur
    scene = scenes.cube_small(api)
    acc = scene.accumulate()                              # opened before the blur was switched on
    scene.motion_blur = MotionBlur()
    issue = native.DeviceRenderer.issue_motion
    with pytest.raises(ValueError, match="whole frames"):
        issue(None, scene, partial=True)
    with pytest.raises(ValueError, match="accumulate"):
        issue(None, scene, accumulating=True)
    assert scene.__dict__.get("_motion_prev") is None, "a refused frame became the previous one"
    assert native.DeviceRenderer._is_partial(scene, (0, 60), None) and native.DeviceRenderer._is_partial(scene, None, (0, 2))
    assert not native.DeviceRenderer._is_partial(scene, (0, 120), None) and not native.DeviceRenderer._is_partial(scene, None, None)
    acc.close()
