"""CPU: the per-face velocity of models that bend, without a device -- the host mirrors ``mr_host_face_homographies`` and
``mr_host_velocity_faces`` against the NumPy restatement motion_faces_ref.py (bit for bit), known answers against exact
rational arithmetic, a bone against the pose it equals, the samples the pass must not touch, the Python layer's flags and
every refusal that needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_faces_fields as ff
import motion_faces_ref as ref
import motion_fields as mf
import scenes
import skin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# The largest distance, in samples, between the float64 restatement's previous position (x - u_0/u_2 before its rounding to
# float32) and the exact rational one, over the faces of the known answers below: 2.320e-14 printed by
# test_the_accuracy_of_the_definition (deterministic float64 arithmetic).  The tests allow 16 times that, the margin section
# 6k uses for the reprojection, plus float32's own rounding of U where a float32 is compared.
ACCURACY_MEASURED = 2.4e-14
BOUND = 16 * ACCURACY_MEASURED


def f32_step(u):
    """Half a float32 step at |u|: what the one rounding to float32 adds."""
    return float(np.spacing(F32(abs(u)))) / 2


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libmi355rast.so is not built: run __graft_entry__.build()")
    return _native


def _both(native, field):
    """The mirrors' (H, U), held to the reference's bit for bit."""
    h, u = field.mirror(native)
    want_h, want_u = field.reference()
    assert h.shape == want_h.shape and ff.bits64(h, want_h) == 0, f"{field!r}: {ff.bits64(h, want_h)} of {want_h.size} doubles of H differ"
    assert ff.bits32(u, want_u) == 0, f"{field!r}: {ff.bits32(u, want_u)} of {want_u.size} velocity floats differ"
    return h, u


# ---------------------------------------------------------------------------- 1. the mirrors against the reference
@pytest.mark.parametrize("size", ff.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mirrors_are_the_reference_on_every_winner_map(native, size):
    for flags in ff.CPU_FLAGS:
        field = ff.three_models(size, flags, seed=size[0])
        h, u = _both(native, field)
        touched = field.touched()
        # the samples of models that are not flagged, and uncovered samples, keep their sentinel bits
        assert ff.bits32(u[~touched], field.velocity[~touched]) == 0, f"{field!r}: a sample outside the flagged models was written"
        assert not np.isnan(u[touched]).any(), f"{field!r}: a flagged sample kept its sentinel"
        assert len(h) == sum(n for n, f in zip((7, 1, 4), flags) if f)


def test_mirrors_are_the_reference_on_the_awkward_faces(native):
    field = ff.counted(len(ff.KINDS) + 3)
    h, u = _both(native, field)
    kind = {name: h[i] for i, name in enumerate(ff.KINDS)}
    for name in ("zero_area", "collinear", "nan_previous"):
        assert not kind[name].any(), f"{name}: H is not zero"
    for name in ("front", "back", "behind_previous", "behind_current", "sub_sample", "still"):
        assert np.abs(kind[name]).max() == 1.0, f"{name}: H is not scaled by its largest entry"
    # det of both signs: the two windings of one triangle have the same H up to the order of the sums, and so the same U
    assert np.allclose(kind["front"], kind["back"], rtol=1e-13, atol=1e-15)
    c = ref.project(field.verts_now, field.s_now)[field.corners]
    det = np.linalg.det(c)
    assert det[0] * det[1] < 0, "the list holds no pair of opposite windings"
    # a zero record moves nothing: U == (0, 0) at every sample that shows such a face
    for name in ("zero_area", "collinear", "nan_previous"):
        at = field.winner == ff.KINDS.index(name)
        assert at.any() and not u[at].any()
    # a corner behind the previous camera: the face's plane still maps, samples whose point lay behind it have U == 0
    assert np.isfinite(u[field.touched()]).all()


@pytest.mark.parametrize("n_faces", (1, 63, 64, 65, 257))
def test_mirrors_are_the_reference_at_every_face_count(native, n_faces):
    _both(native, ff.counted(n_faces, shape=(9, 31), seed=n_faces))


# ---------------------------------------------------------------------------- 2. known answers, exactly
def _plane_triangle(z=-3.0):
    """A triangle in the plane z = *z*, parallel to camera_s()'s image: it covers samples round (35, 22)."""
    return np.array([[-0.9, -0.7, z, 1.0], [1.1, -0.6, z, 1.0], [0.1, 0.9, z, 1.0]])


def _slanted_triangle():
    """A large triangle slanted 60 degrees against camera_s()'s image plane: depth 2 .. 5.46 across 41 samples."""
    far = -2.0 - 2.0 * np.tan(np.radians(60.0))
    return np.array([[-1.0, -0.6, -2.0, 1.0], [1.0, -0.6, far, 1.0], [0.0, 0.7, (far - 2.0) / 2, 1.0]])


def _rigid(degrees=(4.0, -7.0, 3.0), shift=(0.12, -0.05, 0.2)):
    """A rigid move of the world, 4 x 4, row vectors."""
    a, b, c = np.radians(degrees)
    rx = np.array([[1, 0, 0], [0, np.cos(a), np.sin(a)], [0, -np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, -np.sin(b)], [0, 1, 0], [np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), np.sin(c), 0], [-np.sin(c), np.cos(c), 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = rx @ ry @ rz
    m[3, :3] = shift
    return m


def _interior(v, s, shape=(45, 70)):
    """The samples strictly inside the triangle's screen footprint, as (x, y) integer pairs."""
    c = ref.project(v, s)
    px, py = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]
    out = []
    for y in range(shape[0]):
        for x in range(shape[1]):
            e = [(px[(k + 1) % 3] - px[k]) * (y - py[k]) - (py[(k + 1) % 3] - py[k]) * (x - px[k]) for k in range(3)]
            if all(t > 1e-6 for t in e) or all(t < -1e-6 for t in e):
                out.append((x, y))
    return out


def _known_answer_cases():
    """(name, V, P, Sn, Sp) of the faces the accuracy is measured on."""
    s0, s1 = ff.camera_s(), ff.camera_s(eye=(0.07, -0.03, 0.15), yaw=0.02)
    plane, slanted = _plane_triangle(), _slanted_triangle()
    shifted = plane.copy()
    shifted[:, 0] += 3 * 3.0 / 60.0                                 # three samples at depth 3 under focal length 60
    return [("rest", plane, plane, s0, s0), ("rest_slanted", slanted, slanted, s1, s1), ("shift3", plane, shifted, s0, s0),
            ("slanted_rigid", slanted, slanted @ _rigid(), s0, s0), ("slanted_camera", slanted, slanted, s0, s1),
            ("slanted_both", slanted, slanted @ _rigid((-3.0, 5.0, -8.0), (-0.1, 0.08, -0.15)), s1, s0)]


def _restated(v, p, sn, sp, x, y):
    """The float64 restatement's U at sample (x, y) BEFORE its rounding to float32, and the rounded one."""
    h = ref.homographies(v, p, [[0, 1, 2]], sn, sp)[0]
    u = [(x * h[0, c] + y * h[1, c]) + h[2, c] for c in range(3)]
    assert u[2] > 0
    u64 = (x - u[0] / u[2], y - u[1] / u[2])
    u32 = ref.velocity_faces(np.zeros((y + 1, x + 1), np.int32), (0,), (0,), h[None], np.zeros((y + 1, x + 1, 2), F32))[y, x]
    assert u32[0] == F32(u64[0]) and u32[1] == F32(u64[1])
    return u64, u32


def test_the_accuracy_of_the_definition():
    """The bound every other test uses comes from here, not from the kernel or the mirror: the NumPy float64 restatement
    against exact rational arithmetic on the known answers' faces, at every seventh interior sample."""
    worst = 0.0
    for name, v, p, sn, sp in _known_answer_cases():
        samples = _interior(v, sn)[::7]
        assert len(samples) >= 20, name
        for x, y in samples:
            exact = ref.exact_velocity(v, p, sn, sp, x, y)
            assert exact is not None, (name, x, y)
            u64, _ = _restated(v, p, sn, sp, x, y)
            worst = max(worst, float(np.hypot(u64[0] - exact[0], u64[1] - exact[1])))
    print(f"largest error of the float64 restatement against exact arithmetic: {worst:.3e} sample (ACCURACY_MEASURED {ACCURACY_MEASURED:.1e})")
    assert worst <= ACCURACY_MEASURED, "the measured accuracy moved: measure again and write it into section 6l"
    assert BOUND < 1e-12


def test_nothing_moves_when_vertices_and_camera_stay(native):
    """P == V and Sp == Sn on every face of the seeded list that has a footprint, at the samples of that footprint: |U| is
    far below half a sample.  (H is det times the identity up to rounding; a face without area has a det of rounding noise
    and no footprint: no frame shows it.)"""
    now, _, corners = ff.seeded_faces(40, seed=3)
    s = ff.camera_s(eye=(0.02, 0.01, 0.3), yaw=-0.03)
    winner = np.full((45, 70), -1, np.int32)
    shown = 0
    for f in range(len(corners)):
        if (ref.project(now[corners[f]], s)[:, 2] <= 0).any():
            continue                                                 # (a corner behind the camera: no plain footprint)
        samples = _interior(now[corners[f]], s)
        shown += bool(samples)
        for x, y in samples:
            winner[y, x] = f
    field = ff.FaceField("at_rest", now, now, corners, (0,), (1,), s, s, winner)
    _, u = _both(native, field)
    t = field.touched()
    assert shown >= 30 and t.sum() > 500 and np.abs(u[t]).max() < 1e-9


def test_a_face_without_area_is_zero_or_finite_noise(native):
    """What the definition yields where the test above does not look: three collinear corners, at rest, seen through turned
    and moved cameras.  In exact arithmetic det = 0 and H = 0; in float64 det is zero or rounding noise, so H is either all
    zero (U == (0, 0)) or noise scaled to a largest entry of 1, whose U is finite -- motion_velocity lets nothing else out --
    but of any size, thousands of samples among these cases.  No frame shows a sample of such a face (it covers none), and
    k_mblur clamps a segment at 16 samples; the test pins that both outcomes occur, that U is never NaN or infinite, and
    that mirror and restatement agree bit for bit on the noise too.  Two equal corners give det = 0 exactly, always."""
    lines = [[(-0.5, -0.5, -4.0), (0.0, 0.0, -4.0), (0.25, 0.25, -4.0)], [(-0.3, 0.2, -2.5), (0.1, 0.0, -3.5), (0.5, -0.2, -4.5)]]
    doubled = [(0.1, 0.1, -3.0), (0.1, 0.1, -3.0), (0.4, 0.2, -3.0)]
    zero = noise = 0
    largest = 0.0
    for yaw in (-0.03, 0.01, 0.2, -0.4):
        for eye in ((0.02, 0.01, 0.3), (0.0, 0.0, 0.0)):
            s = ff.camera_s(eye=eye, yaw=yaw)
            for pts in lines + [doubled]:
                v = np.ones((3, 4))
                v[:, :3] = pts
                field = ff.FaceField("no_area", v, v, [[0, 1, 2]], (0,), (1,), s, s, np.zeros((45, 70), np.int32))
                h, u = _both(native, field)
                assert np.isfinite(u).all(), (yaw, eye, pts)
                if not h.any():
                    zero += 1
                    assert not u.any()
                else:
                    noise += 1
                    assert pts is not doubled and np.abs(h).max() == 1.0
                    largest = max(largest, float(np.abs(u).max()))
    print(f"faces without area: H == 0 in {zero} cases, noise in {noise}, |U| of the noise up to {largest:.3g} samples")
    assert zero >= 8 and noise >= 4 and largest > 0.5


def test_a_face_shifted_by_three_samples(native):
    name, v, p, sn, sp = _known_answer_cases()[2]
    samples = _interior(v, sn)
    winner = np.full((45, 70), -1, np.int32)
    for x, y in samples:
        winner[y, x] = 0
    field = ff.FaceField(name, v, p, [[0, 1, 2]], (0,), (1,), sn, sp, winner)
    _, u = _both(native, field)
    got = u[winner == 0].astype(np.float64)
    assert len(got) > 500
    assert np.abs(got[:, 0] + 3.0).max() <= BOUND + f32_step(3.0) and np.abs(got[:, 1]).max() <= BOUND


def _matrix_path(native, v, sn, sp, move, samples, shape=(45, 70)):
    """U of the matrix path (k_velocity's: one 4 x 3 matrix for the class, the z-buffer) on the triangle's samples, with
    the z-buffer upstream's rasteriser leaves: the eye depths of the three vertices interpolated linearly over the screen."""
    c = ref.project(v, sn)
    px, py, w = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2], c[:, 2]
    coeff = np.linalg.solve(np.stack([px, py, np.ones(3)], axis=1), w)           # Z = a x + b y + c through the vertices
    z = np.full(shape, np.inf)
    winner = np.full(shape, -1, np.int32)
    for x, y in samples:
        z[y, x], winner[y, x] = coeff @ (x, y, 1.0), 0
    # (x Z, y Z, Z) = (X, Y, W) = v . top + bottom of Sn; the previous position is ((v . R + t), 1) . Sp
    top_n, bottom_n, top_p, bottom_p = sn[:3], sn[3], sp[:3], sp[3]
    a = np.linalg.inv(top_n) @ move[:3, :3] @ top_p
    t = np.vstack([a, (-bottom_n @ a + move[3, :3] @ top_p + bottom_p)[None, :]])
    d = native.fill_motion_desc(mf.IDENTITY, 1.0, (mf.IDENTITY_T, t / np.abs(t).max()), mf.IDENTITY_B, (1,))
    return native.host_velocity(z, winner, (0,), d), winner


def test_a_large_slanted_triangle_is_exact_where_the_matrix_path_is_not(native):
    """60 degrees of slant under a perspective camera, a rigid move: the per-face U meets the exact answer at every interior
    sample; the matrix path, which reprojects through a z-buffer that is linear in the screen, misses it by whole samples
    in the middle of the face (and meets it near the vertices, where that z-buffer is right)."""
    name, v, p, sn, sp = _known_answer_cases()[3]
    move = _rigid()
    samples = _interior(v, sn)
    assert len(samples) > 400
    matrix_u, winner = _matrix_path(native, v, sn, sp, move, samples)
    field = ff.FaceField(name, v, p, [[0, 1, 2]], (0,), (1,), sn, sp, winner, velocity=matrix_u)
    _, u = _both(native, field)
    worst_face = worst_matrix = 0.0
    for x, y in samples[::5]:
        exact = ref.exact_velocity(v, p, sn, sp, x, y)
        err = float(np.hypot(float(u[y, x, 0]) - exact[0], float(u[y, x, 1]) - exact[1]))
        assert err <= BOUND + 2 * f32_step(max(abs(exact[0]), abs(exact[1]))), (x, y, err)
        worst_face = max(worst_face, err)
        worst_matrix = max(worst_matrix, float(np.hypot(float(matrix_u[y, x, 0]) - exact[0], float(matrix_u[y, x, 1]) - exact[1])))
    print(f"slanted triangle: per-face error {worst_face:.2e} sample, matrix path through a screen-linear z {worst_matrix:.2e}")
    assert worst_matrix > 0.5, "the matrix path was expected to miss by more than half a sample inside this face"


# ---------------------------------------------------------------------------- 3. one bone equals a pose
def test_one_bone_of_weight_one_is_the_pose(api, native):
    """A skin whose every vertex follows one bone M with weight 1, on a plane parallel to the image, M a move inside that
    plane: the per-face U of the skinned vertices is the U that pose = M gives through _pack.motion_matrices and the
    z-buffer (exact on such a plane), within the two paths' bounds together."""
    from py_numpy_renderer_amd import MotionBlur, _pack
    from test_motion_cpu import REPROJECTION_MEASURED
    scene = scenes.cube_outward(api, resolution=(136, 152))
    scene.motion_blur = MotionBlur(deformation=True)
    cam = scene.camera
    look = np.asarray(cam.lookat, dtype=np.float64)
    depth = -1.5 if int(scene.system) == int(api.SYSTEM.RH) else 1.5
    eye = np.array([[-0.5, -0.4, depth, 1.0], [0.6, -0.3, depth, 1.0], [0.0, 0.5, depth, 1.0]])
    rest = eye @ np.linalg.inv(look)
    in_plane = np.eye(4)
    a = np.radians(6.0)
    in_plane[:2, :2] = [[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]]
    in_plane[3, :2] = (0.11, -0.07)
    m = look @ in_plane @ np.linalg.inv(look)
    joints, weights = np.zeros((3, 4), np.int64), np.zeros((3, 4))
    weights[:, 0] = 1.0
    skinned = skin_ref.skinned_vertices(rest, joints, weights, m[None])
    previous = _pack.MotionState(scene)
    s = previous.S[:, (0, 1, 3)]
    # the pose's path: class matrix, constant z-buffer
    scene.models[0].pose = m
    depth_map, T, B, class_of, _ = _pack.motion_matrices(scene, previous)
    scene.models[0].pose = None
    assert class_of[0] == 1
    c = ref.project(skinned, s)
    n, f = float(cam.near), float(cam.far)
    clip = skinned @ np.asarray(cam.MVP, dtype=np.float64)
    scr = (clip / clip[:, 3:]) @ np.asarray(_pack.sample_grid(scene)[3], dtype=np.float64)
    zs = 2 * n * f / ((f + n) - scr[:, 2] * (f - n))
    assert np.ptp(zs) < 1e-12 * abs(zs[0]), "the moved plane is not parallel to the image"
    samples = _interior(skinned, s, shape=(136, 152))
    assert len(samples) > 300 and np.allclose(c[:, 0] / c[:, 2], scr[:, 0])
    winner = np.full((136, 152), -1, np.int32)
    for x, y in samples:
        winner[y, x] = 0
    z = np.where(winner == 0, zs.mean(), np.inf)
    n_models = len(scene.models)
    face_off = np.arange(n_models) * 1000                             # (model 0 owns the one face)
    d = native.fill_motion_desc(depth_map, 0.5, T, B, class_of)
    pose_u = native.host_velocity(z, winner, face_off, d)
    field = ff.FaceField("one_bone", skinned, rest, [[0, 1, 2]], (0,), (1,), s, s, winner)
    _, bone_u = _both(native, field)
    at = winner == 0
    diff = np.abs(bone_u[at].astype(np.float64) - pose_u[at].astype(np.float64)).max()
    size = float(np.abs(pose_u[at]).max())
    assert size > 3, "the bone moves the face by a few samples"
    assert diff <= 16 * (ACCURACY_MEASURED + REPROJECTION_MEASURED) + 2 * f32_step(size), diff


# ---------------------------------------------------------------------------- 4. the Python layer (no device)
def _bendable_scene(api):
    """cube_outward with a skin on model 0 and a morph on model 1 (no bones, no weights yet)."""
    from py_numpy_renderer_amd import Morph, Skin
    scene = scenes.cube_outward(api, resolution=(30, 40))
    a, b = scene.models[0], scene.models[1]
    joints = np.zeros((len(a.vertices), 4), np.int64)
    weights = np.zeros((len(a.vertices), 4))
    weights[:, 0] = 1.0
    a.skin = Skin(joints, weights)
    target = np.zeros((len(b.vertices), 3))
    target[0] = (0.1, 0.0, 0.0)
    b.morph = Morph([target])
    return scene


def test_motion_vertices_flags_exactly_what_bent(api, native):
    from py_numpy_renderer_amd import Morph, MotionBlur, Skin, translation
    scene = _bendable_scene(api)
    a, b = scene.models[0], scene.models[1]
    scene.motion_blur = MotionBlur(shutter=0.75, deformation=True)
    issue = lambda: native.DeviceRenderer.issue_motion(None, scene)

    def flags():
        frame = scene.__dict__["_motion_faces_frame"]
        return np.frombuffer(frame[2], dtype=np.int32).tolist(), frame[3]

    issue()
    assert flags() == ([0, 0], -1), "the first frame has no previous one"
    scene.__dict__["_motion_prev"].serial = 7                        # (what note_motion_serial leaves behind the enqueue)
    issue()
    assert flags() == ([0, 0], 7), "nothing changed"
    a.bones = np.asarray(translation((0.1, 0.0, 0.0)), dtype=np.float64)[None]
    issue()
    assert flags() == ([1, 0], -1), "new bones flag their model; the state that frame left has no serial yet"
    issue()
    assert flags()[0] == [0, 0], "the bones stayed"
    a.bones = np.array(a.bones)                                      # an equal array: no change by value
    b.morph_weights = np.array([0.5])
    issue()
    assert flags()[0] == [0, 1]
    b.morph_weights = np.array([0.25])
    a.pose = np.asarray(translation((0.0, 0.1, 0.0)), dtype=np.float64)
    issue()
    assert flags()[0] == [0, 1], "a pose alone flags nothing: its class in motion_matrices carries it"
    assert np.frombuffer(scene.__dict__["_motion_frame"][4], dtype=np.int32).tolist() == [1, 0], "motion_matrices keeps the classes"
    a.skin = Skin(a.skin.joints, a.skin.weights)                     # another object of the same value: flagged by identity
    issue()
    assert flags()[0] == [1, 0]
    b.morph = Morph(b.morph.targets)
    issue()
    assert flags()[0] == [0, 1]
    a.bones = None
    b.morph_weights = None
    issue()
    assert flags()[0] == [1, 1], "bones and weights that go flag their models"
    # the views of render_frames differ in their cameras only: after the first view nothing is flagged
    a.bones = np.asarray(translation((0.0, 0.0, 0.1)), dtype=np.float64)[None]
    views = [api.Camera((0.5 + 0.1 * k, 1, 2), (0, 0, 0), fovy=60, near=0.1, far=20, backface_culling=True) for k in range(3)]
    seen = []
    for cam in views:
        scene.camera = cam
        issue()
        seen.append(flags()[0])
    assert seen == [[1, 0], [0, 0], [0, 0]]
    s_now, s_prev = (np.frombuffer(scene.__dict__["_motion_faces_frame"][k], dtype=np.float64).reshape(4, 3) for k in (0, 1))
    assert not np.array_equal(s_now, s_prev), "the views' cameras differ: Sp is the previous view's"
    # a frame rendered again after an overflow takes its first attempt's description
    first = scene.__dict__["_motion_faces_frame"]
    state = scene.__dict__["_motion_prev"]
    scene.__dict__["_motion_replay"], scene.__dict__["_motion_faces_replay"] = scene.__dict__["_motion_frame"], ("kept",)
    issue()
    assert scene.__dict__["_motion_faces_frame"] == ("kept",) and scene.__dict__["_motion_prev"] is state
    del scene.__dict__["_motion_replay"], scene.__dict__["_motion_faces_replay"]
    # reset_motion and another model list forget the previous state
    a.bones = None
    scene.reset_motion()
    issue()
    assert flags() == ([0, 0], -1) and first != scene.__dict__["_motion_faces_frame"]
    scene.motion_blur = None
    issue()
    assert scene.__dict__.get("_motion_faces_frame") is None or scene.__dict__.get("_motion_frame") is None


def test_without_the_flag_the_frame_is_the_parents(api, native):
    """deformation=False, the default: motion_matrices' outputs are what they were, no per-face description exists, the
    state copies no bones, and the renderer's sync makes no call."""
    from py_numpy_renderer_amd import MotionBlur, _pack, translation
    scene = _bendable_scene(api)
    scene.motion_blur = MotionBlur(shutter=0.75)
    assert scene.motion_blur.deformation is False
    issue = lambda: native.DeviceRenderer.issue_motion(None, scene)
    issue()
    scene.models[0].bones = np.asarray(translation((0.1, 0.0, 0.0)), dtype=np.float64)[None]
    scene.models[1].pose = np.asarray(translation((0.0, 0.1, 0.0)), dtype=np.float64)
    previous = scene.__dict__["_motion_prev"]
    want = _pack.motion_matrices(scene, previous)
    issue()
    frame = scene.__dict__["_motion_frame"]
    assert frame == (0.75, tuple(want[0]), want[1].tobytes(), want[2].tobytes(), want[3].tobytes())
    assert np.frombuffer(frame[4], dtype=np.int32).tolist() == [0, 1], "bones move nothing without the flag"
    assert scene.__dict__["_motion_faces_frame"] is None
    state = scene.__dict__["_motion_prev"]
    assert state.bones is None and state.weights is None and state.serial is None
    s_now, s_prev, flags, serial = _pack.motion_vertices(scene, state)
    assert not flags.any() and serial == -1

    class Lib:                                                      # (a library that counts its calls)
        calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append(name) or 0

    renderer = native.DeviceRenderer.__new__(native.DeviceRenderer)
    renderer.lib, renderer.handle = Lib(), None
    renderer.sync_motion_faces(scene)
    renderer.note_motion_serial(scene)
    assert Lib.calls == [], "a scene without the flag calls none of the new entry points"
    scene.motion_blur = MotionBlur(shutter=0.75, deformation=True)
    issue()
    renderer.sync_motion_faces(scene)
    renderer.note_motion_serial(scene)
    assert Lib.calls == ["mr_scene_track_vertices", "mr_scene_set_motion_faces", "mr_scene_vertices_serial"]
    renderer.sync_motion_faces(scene)
    assert len(Lib.calls) == 3, "the same description is handed over once"
    scene.motion_blur = None
    issue()
    renderer.sync_motion_faces(scene)
    assert Lib.calls[3:] == ["mr_scene_set_motion_faces", "mr_scene_track_vertices"], "off again, tracking too"


@pytest.mark.parametrize("attr, sync, entry, make, changed", [
    ("ambient_occlusion", "sync_ambient_occlusion", "mr_scene_set_ambient_occlusion", lambda pkg: pkg.AmbientOcclusion(radius=0.5),
     lambda pkg: pkg.AmbientOcclusion(radius=0.25)),
    ("depth_of_field", "sync_depth_of_field", "mr_scene_set_depth_of_field", lambda pkg: pkg.DepthOfField(lens_radius=0.1),
     lambda pkg: pkg.DepthOfField(lens_radius=0.2))], ids=["ambient_occlusion", "depth_of_field"])
def test_a_description_goes_over_when_it_changes_and_only_then(api, native, attr, sync, entry, make, changed):
    """``DeviceRenderer._sync_desc`` behind its two callers, on a renderer whose ``__init__`` never ran and a library
    that counts its calls: none without the pass, one with it, none for the same description again, one for a changed
    one, one -- with a NULL description -- when the pass has gone, and none after that."""
    import py_numpy_renderer_amd as pkg

    class Lib:                                                      # (counts its calls and keeps whether a description came)
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda handle, desc=None: self.calls.append((name, desc is not None)) or 0

    scene = scenes.cube_small(api)
    renderer = native.DeviceRenderer.__new__(native.DeviceRenderer)
    renderer.lib, renderer.handle = Lib(), None
    go = lambda: getattr(renderer, sync)(scene)
    go()
    assert renderer.lib.calls == [], "a scene without the pass makes no call"
    setattr(scene, attr, make(pkg))
    go()
    assert renderer.lib.calls == [(entry, True)]
    go()
    setattr(scene, attr, make(pkg))                                 # (an equal object: the description is compared by value)
    go()
    assert len(renderer.lib.calls) == 1, "the same description is handed over once"
    setattr(scene, attr, changed(pkg))
    go()
    assert renderer.lib.calls[1:] == [(entry, True)], "a changed description goes over"
    setattr(scene, attr, None)
    go()
    assert renderer.lib.calls[2:] == [(entry, False)], "the pass has gone: one call with a NULL description"
    go()
    assert len(renderer.lib.calls) == 3


def test_the_python_class(api):
    from py_numpy_renderer_amd import MotionBlur
    mb = MotionBlur()
    assert mb.shutter == 0.5 and mb.deformation is False and repr(mb) == "MotionBlur(shutter=0.5, deformation=False)"
    mb = MotionBlur(0.25, deformation=True)
    assert mb.deformation is True and "deformation=True" in repr(mb)
    with pytest.raises(AttributeError, match="read-only"):
        mb.deformation = False
    for bad in (1, 0, None, "yes", 1.0, [True]):
        with pytest.raises(TypeError, match="deformation must be a bool"):
            MotionBlur(deformation=bad)
    scene = scenes.cube_small(api)
    scene.motion_blur = mb
    for call in (scene.accumulate, lambda: scene.render_mean(2, lambda k: None)):
        with pytest.raises(ValueError, match="accumulate"):
            call()


# ---------------------------------------------------------------------------- 5. refusals and bindings, no device
def test_symbols_are_bound(native):
    lib = native.load_library()
    for name in ("mr_scene_set_motion_faces", "mr_scene_track_vertices", "mr_scene_vertices_serial", "mr_host_face_homographies",
                 "mr_host_velocity_faces", "mr_debug_motion_faces_post", "mr_debug_read_prev_vertices", "mr_debug_motion_faces",
                 "mr_debug_motion_faces_times"):
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert C.sizeof(native.MotionFacesDesc) == 24 * 8 + 8 + 8 + 8
    header = open(os.path.join(ROOT, "include", "mi355rast.h")).read()
    body = header.split("typedef struct mr_motion_faces_desc")[1].split("} mr_motion_faces_desc;")[0]
    for line in ("double s_now[12], s_prev[12];", "const int32_t *deforming;", "int32_t n_models;", "int64_t prev_serial;"):
        assert line in body
    assert "#define MR_ABI_VERSION 4" in header and lib.mr_abi_version() == 4
    # mr_motion_desc is what it was
    assert C.sizeof(native.MotionDesc) == 4 * 8 + 8 + 8 + 9 * 8 + 8 + 8


def test_the_library_checks_the_description(native):
    from test_motion_cpu import _scene_with_models
    lib, handle = _scene_with_models(native, 2)
    s = ff.camera_s()
    desc = lambda s_now=s, s_prev=s, flags=(0, 1), serial=3: native.fill_motion_faces_desc(s_now, s_prev, flags, serial)
    assert lib.mr_scene_set_motion_faces(None, C.byref(desc())) == native.MR_E_INVALID
    assert lib.mr_scene_set_motion_faces(handle, None) == 0                       # off, on a scene that never had it
    assert lib.mr_scene_set_motion_faces(handle, C.byref(desc())) == native.MR_E_INVALID and b"mr_scene_set_motion_blur comes first" in lib.mr_last_error()
    blur = native.fill_motion_desc(mf.MOEBIUS, 0.5, (mf.IDENTITY_T,), mf.IDENTITY_B, (0, 0))
    assert lib.mr_scene_set_motion_blur(handle, C.byref(blur)) == 0
    assert lib.mr_scene_set_motion_faces(handle, C.byref(desc())) == 0, lib.mr_last_error()       # (copied: no device is touched)
    for bad in (float("nan"), float("inf")):
        for which in ("s_now", "s_prev"):
            m = s.copy()
            m[3, 1] = bad
            assert lib.mr_scene_set_motion_faces(handle, C.byref(desc(**{which: m}))) == native.MR_E_INVALID
            assert b"not finite" in lib.mr_last_error()
    for flags in ((1,), (0, 1, 0)):
        assert lib.mr_scene_set_motion_faces(handle, C.byref(desc(flags=flags))) == native.MR_E_INVALID and b"n_models" in lib.mr_last_error()
    d = desc()
    d.deforming = None
    assert lib.mr_scene_set_motion_faces(handle, C.byref(d)) == native.MR_E_INVALID and b"NULL" in lib.mr_last_error()
    # tracking and the serial need no device either; a scene that never committed has held no vertices
    assert lib.mr_scene_vertices_serial(handle) == 0
    assert lib.mr_scene_track_vertices(handle, 1) == 0 and lib.mr_scene_track_vertices(handle, 0) == 0
    assert lib.mr_scene_track_vertices(None, 1) == native.MR_E_INVALID
    out = np.zeros(4, np.int32)
    assert lib.mr_debug_motion_faces(handle, out.ctypes.data) == 0 and out.tolist() == [0, 0, 0, 0]
    assert lib.mr_debug_motion_faces(handle, None) == native.MR_E_INVALID
    ms = (C.c_float * 2)()
    assert lib.mr_debug_motion_faces_times(handle, ms) == native.MR_E_INVALID      # no frame yet
    verts = np.zeros((6, 4))
    assert lib.mr_debug_read_prev_vertices(handle, verts.ctypes.data) == native.MR_E_INVALID and b"no snapshot" in lib.mr_last_error()
    lib.mr_scene_destroy(handle)


def test_the_mirrors_and_the_debug_entry_check_their_arguments(native):
    lib = native.load_library()
    field = ff.three_models((4, 5), (1, 0, 1))
    faces = native.face_records(field.corners)
    nan_s = field.s_now.copy()
    nan_s[0, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        native.host_face_homographies(field.verts_now, field.verts_prev, faces, nan_s, field.s_prev)
    inf_s = field.s_prev.copy()
    inf_s[3, 2] = -np.inf
    with pytest.raises(ValueError, match="not finite"):
        native.host_face_homographies(field.verts_now, field.verts_prev, faces, field.s_now, inf_s)
    for bad in (len(field.verts_now), -1):
        outside = faces.copy()
        outside[5, 4] = bad
        with pytest.raises(ValueError, match="outside the vertex array"):
            native.host_face_homographies(field.verts_now, field.verts_prev, outside, field.s_now, field.s_prev)
    out = np.zeros((len(faces), 9))
    args = lambda **o: [o.get("now", field.verts_now.ctypes.data), o.get("prev", field.verts_prev.ctypes.data), o.get("nv", len(field.verts_now)),
                        o.get("faces", faces.ctypes.data), o.get("nf", len(faces)), o.get("sn", field.s_now.ctypes.data),
                        o.get("sp", field.s_prev.ctypes.data), o.get("out", out.ctypes.data)]
    assert lib.mr_host_face_homographies(*args()) == 0
    for over in (dict(now=None), dict(prev=None), dict(faces=None), dict(sn=None), dict(sp=None), dict(out=None), dict(nv=-1), dict(nf=-1),
                 dict(nv=3)):
        assert lib.mr_host_face_homographies(*args(**over)) == native.MR_E_INVALID, over
    hom_off, picked = field.layout()
    h = native.host_face_homographies(field.verts_now, field.verts_prev, native.face_records(field.corners[picked]), field.s_now, field.s_prev)
    native.host_velocity_faces(field.winner, field.face_off, hom_off, h, field.velocity)
    with pytest.raises(ValueError, match="has no record"):
        native.host_velocity_faces(field.winner, field.face_off, hom_off, h[:-1], field.velocity)
    with pytest.raises(ValueError, match="ascend from 0"):
        native.host_velocity_faces(field.winner, (0, 8, 7), hom_off, h, field.velocity)
    with pytest.raises(ValueError, match="ascend from 0"):
        native.host_velocity_faces(field.winner, (1, 7, 8), hom_off, h, field.velocity)
    with pytest.raises(ValueError, match="winner must be"):
        native.host_velocity_faces(field.winner[:2], field.face_off, hom_off, h, field.velocity)
    vel = field.velocity.copy()
    v_args = lambda **o: [o.get("win", field.winner.ctypes.data), o.get("off", field.face_off.ctypes.data), o.get("hom", hom_off.ctypes.data),
                          o.get("nm", 3), o.get("h", h.ctypes.data), o.get("nr", len(h)), o.get("rows", 4), o.get("cols", 5),
                          o.get("vel", vel.ctypes.data)]
    assert lib.mr_host_velocity_faces(*v_args()) == 0
    for over in (dict(win=None), dict(off=None), dict(hom=None), dict(h=None), dict(vel=None), dict(rows=0), dict(cols=40000), dict(nm=0),
                 dict(nr=-1)):
        assert lib.mr_host_velocity_faces(*v_args(**over)) == native.MR_E_INVALID, over
    # mr_debug_motion_faces_post refuses before it asks for a device
    handle = lib.mr_scene_create()
    outside = field.corners.copy()
    outside[0, 0] = 9999
    bad = ff.FaceField("outside", field.verts_now, field.verts_prev, outside, field.face_off, field.deforming, field.s_now, field.s_prev, field.winner)
    with pytest.raises(ValueError, match="outside the vertex array"):
        bad.device(native, handle)
    bad = ff.FaceField("nan", field.verts_now, field.verts_prev, field.corners, field.face_off, field.deforming, nan_s, field.s_prev, field.winner)
    with pytest.raises(ValueError, match="not finite"):
        bad.device(native, handle)
    beyond = field.winner.copy()
    beyond[0, 0] = 12                                                # a face the flagged last model does not have
    bad = ff.FaceField("beyond", field.verts_now, field.verts_prev, field.corners, field.face_off, field.deforming, field.s_now, field.s_prev, beyond)
    with pytest.raises(ValueError, match="has no record"):
        bad.device(native, handle)
    bad = ff.FaceField("descending", field.verts_now, field.verts_prev, field.corners, (0, 8, 7), field.deforming, field.s_now, field.s_prev, field.winner)
    with pytest.raises(ValueError, match="ascend"):
        bad.device(native, handle)
    lib.mr_scene_destroy(handle)
