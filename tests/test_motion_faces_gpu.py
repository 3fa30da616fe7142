"""GPU: ``MotionBlur(deformation=True)`` -- the velocity of models that bend, per winner face, from the library's snapshot of
the previous frame's vertices (k_face_homography and k_velocity_faces in kernels_motion_faces.h, host_motion_faces.h).

The yardstick: the host mirrors applied to what a TWIN of the scene -- the same recipe, camera, poses, bones and weights,
without ``motion_blur`` -- hands out through its taps: ``mr_host_velocity`` gives k_velocity's U, ``mr_host_face_homographies``
the records of the flagged models' faces from the previous vertices (``mr_debug_read_prev_vertices`` of the scene) and the
current ones (the twin's own snapshot, taken by a pass behind its frame), ``mr_host_velocity_faces`` overwrites,
``mr_host_motion_blur`` blurs.  ``read_velocity()`` and the float frame must match bit for bit."""
import numpy as np
import pytest

import scenes
import skin_ref
from test_motion_gpu import KW, SMALL, SQUEEZED, _bits, _desc, _face_off, _look, _twin_taps

pytestmark = pytest.mark.gpu


def _blur(deformation=True, shutter=1.0):
    from py_numpy_renderer_amd import MotionBlur
    return MotionBlur(shutter=shutter, deformation=deformation)


def _pair(api, resolution=SMALL, deformation=True, **settings):
    """cube_outward with the blur, and its twin without; the cube (model 0) carries the `bend` rig's skin and a morph of
    two targets in both."""
    from py_numpy_renderer_amd import Morph, Skin
    scene, twin = scenes.cube_outward(api, resolution=resolution), scenes.cube_outward(api, resolution=resolution)
    for s in (scene, twin):
        for name, value in settings.items():
            setattr(s, name, value)
        cube = s.models[0]
        joints, weights, _ = skin_ref.rig(api, cube, "bend")
        cube.skin = Skin(joints, weights)
        xyz = np.asarray(cube.vertices, dtype=np.float64)[:, :3]
        cube.morph = Morph([0.3 * xyz * (xyz[:, :1] > 0), np.tile((0.0, 0.15, 0.0), (len(xyz), 1)) * (xyz[:, 1:2] > 0)])
    scene.motion_blur = _blur(deformation)
    return scene, twin


def _bones(api, scene, frame):
    return skin_ref.rig(api, scene.models[0], "bend", frame=frame)[2]


def _n_verts(scene):
    return sum(len(m.vertices) for m in scene.models)


def _corners(scene):
    """The global vertex indices of every face's corners, (n_faces, 3)."""
    out, first = [], 0
    for m in scene.models:
        out.append(np.asarray(m._faces)[:, :, 0].astype(np.int64) + first)
        first += len(m.vertices)
    return np.concatenate(out)


def _current_vertices(api, twin):
    """The vertices the twin's last frame was rendered from: its library's snapshot, taken by one more pass -- another pose
    on the cube, taken back at once.  (The cube bends already, so the pose starts no model moving: a float32 model that
    starts to move is committed again first, and the snapshot would hold the pristine vertices.)"""
    from py_numpy_renderer_amd import translation
    backend = twin._backend()
    assert backend.lib.mr_scene_track_vertices(backend.handle, 1) == 0
    cube = twin.models[0]
    assert cube.bones is not None or cube.morph_weights is not None
    keep, commits = cube.pose, backend.pose_counters()[0]
    nudge = np.asarray(translation((0.0, 0.01, 0.0)), dtype=np.float64)
    cube.pose = nudge if keep is None else keep @ nudge
    backend.render(twin, counters=False, keep_buffers=False, overlay=False)
    assert backend.pose_counters()[0] == commits, "the twin was committed again: its snapshot is not the last frame's"
    verts = backend.read_prev_vertices(_n_verts(twin))
    cube.pose = keep
    return verts


def _hold(api, scene, twin, label, ran=True):
    """Renders the scene's next frame and holds it to the mirrors; returns (winner, k_velocity's U, U, F, F')."""
    from py_numpy_renderer_amd import _native
    assert not scene.draw_debug_frustum
    backend = scene._backend()
    before = backend.motion_faces_debug()
    scene.render()
    got, u = backend.read_frame_f32().copy(), backend.read_velocity().copy()
    after = backend.motion_faces_debug()
    z, winner, f = _twin_taps(twin)
    desc = _desc(scene)
    face_off = _face_off(scene)
    matrix_u = _native.host_velocity(z, winner, face_off, desc)
    want_u = matrix_u
    # (without the flag the frame has no per-face description: nothing is flagged)
    s_now, s_prev, deforming, prev_serial = scene.__dict__["_motion_faces_frame"] or (None, None, np.zeros(len(face_off), np.int32).tobytes(), -1)
    deforming = np.frombuffer(deforming, dtype=np.int32)
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if ran else (0, int(deforming.any()))), (label, before, after)
    if ran:
        assert deforming.any() and prev_serial >= 0
        corners = _corners(scene)
        hom_off, records = _native.hom_offsets(face_off, deforming, len(corners))
        assert after[2] == records
        flagged = np.concatenate([np.arange(face_off[m], (list(face_off) + [len(corners)])[m + 1]) for m in range(len(face_off)) if hom_off[m] >= 0])
        previous = backend.read_prev_vertices(_n_verts(scene))
        current = _current_vertices(api, twin)
        h = _native.host_face_homographies(current, previous, _native.face_records(corners[flagged]),
                                           np.frombuffer(s_now, dtype=np.float64).reshape(4, 3), np.frombuffer(s_prev, dtype=np.float64).reshape(4, 3))
        want_u = _native.host_velocity_faces(winner, face_off, hom_off, h, matrix_u)
    want = _native.host_motion_blur(z, want_u, f, desc)
    bits_u, bits = _bits(u, want_u), _bits(got, want)
    print(f"{label}: {bits_u} velocity floats and {bits} colour floats differ from the mirrors; the per-face pass changed "
          f"{int((want_u != matrix_u).any(axis=-1).sum())} of {winner.size} samples' U, |U| up to {np.hypot(u[..., 0], u[..., 1]).max():.2f}")
    assert bits_u == 0, f"{label}: read_velocity() is not the mirrors'"
    assert bits == 0, f"{label}: the float frame is not the mirrors'"
    return winner, matrix_u, u, f, got


def _set(scenes_, **state):
    for s in scenes_:
        for name, value in state.items():
            setattr(s.models[0], name, None if value is None else np.array(value, dtype=np.float64))


# ---------------------------------------------------------------------------- 1. the frames against the mirrors
def test_a_skinned_cube_over_a_still_floor(api):
    """Bones alone under a still camera.  Without the flag U is k_velocity's, zero on the cube: the frame renders sharp.  With
    it the cube's samples move by more than half a sample and the floor's U is what it was."""
    plain, plain_twin = _pair(api, deformation=False)
    scene, twin = _pair(api)
    for s in (plain, scene):
        s.render()
    _set((plain, plain_twin, scene, twin), bones=_bones(api, scene, 0))
    plain.render()
    u_plain = plain._backend().read_velocity().copy()
    assert np.abs(u_plain).max() < 1e-6, "without the flag the bones move nothing"
    assert plain._backend().motion_faces_debug() == (0, 0, 0, 0), "without the flag nothing is tracked, run or skipped"
    assert np.array_equal(plain.render(), plain_twin.render()), "at rest: sharp"
    winner, matrix_u, u, f, got = _hold(api, scene, twin, "bones from rest")
    cube = (winner >= 0) & (winner < len(scene.models[0]._faces))
    floor = winner >= len(scene.models[0]._faces)
    assert cube.sum() > 500 and floor.sum() > 500
    assert np.abs(matrix_u).max() < 1e-6, "k_velocity alone sees no motion here"
    moved = np.hypot(u[cube, 0], u[cube, 1])
    assert (moved > 0.5).mean() > 0.3 and moved.max() > 2, "the bent cube's samples do not move"
    assert _bits(u[~cube], matrix_u[~cube]) == 0, "the floor's or the sky's U changed"
    assert _bits(got, f) > 0, "the frame is not blurred"
    _set((scene, twin), bones=_bones(api, scene, 2))
    _hold(api, scene, twin, "bones, frame 0 to frame 2")
    assert np.array_equal(scene.render(), twin.render()), "nothing bends any more: the plain frame"
    for s in (plain, plain_twin, scene, twin):
        s.close()


def test_morph_weights_bones_pose_and_a_moving_camera(api):
    from py_numpy_renderer_amd import translation
    scene, twin = _pair(api)
    scene.render()
    for k, weights in enumerate(((0.8, 0.0), (0.8, 0.9), (0.1, 0.9))):
        _set((scene, twin), morph_weights=weights)
        winner, matrix_u, u, _, _ = _hold(api, scene, twin, f"morph weights {weights}")
        assert _bits(u, matrix_u) > 0
    _set((scene, twin), morph_weights=(0.5, 0.4), bones=_bones(api, scene, 1), pose=translation((0.1, 0.0, -0.04)))
    winner, matrix_u, u, _, _ = _hold(api, scene, twin, "weights, bones and pose together")
    cube = (winner >= 0) & (winner < len(scene.models[0]._faces))
    assert np.hypot(matrix_u[cube, 0], matrix_u[cube, 1]).min() > 0.5, "the pose has its class in k_velocity"
    assert _bits(u[cube], matrix_u[cube]) > 0 and _bits(u[~cube], matrix_u[~cube]) == 0
    for s in (scene, twin):
        _look(api, s, (0.6, 1.0, 1.95))
    _set((scene, twin), bones=_bones(api, scene, 3))
    winner, matrix_u, u, _, _ = _hold(api, scene, twin, "bones under a moving camera")
    floor = winner >= len(scene.models[0]._faces)
    assert np.hypot(u[floor, 0], u[floor, 1]).max() > 1, "the camera moved: the floor moves"
    # a camera move alone flags nothing: neither kernel is launched
    for s in (scene, twin):
        _look(api, s, (0.5, 1.0, 2.0))
    _hold(api, scene, twin, "the camera alone", ran=False)
    times = scene._backend().motion_faces_times()
    assert times["face_homography"] > 0 and times["velocity_faces"] > 0 and scene._backend().motion_times()["mblur"] > 0
    scene.close(), twin.close()


def test_supersampled(api):
    scene, twin = _pair(api, resolution=(68, 76), supersample=2)
    scene.render()
    _set((scene, twin), bones=_bones(api, scene, 1))
    winner, matrix_u, u, f, got = _hold(api, scene, twin, "(68, 76), supersample 2")
    assert got.shape == (136, 152, 3) and _bits(u, matrix_u) > 0
    scene.close(), twin.close()


def test_without_the_flag_the_frames_are_k_velocity_s(api):
    """deformation=False over bones, weights, a pose and a camera move: every frame is held to the mirrors of the parent's
    path alone -- mr_host_velocity's U on the twin's taps, blurred by mr_host_motion_blur -- bit for bit, and none of the
    new entry points' counters moves."""
    from py_numpy_renderer_amd import translation
    scene, twin = _pair(api, deformation=False)
    scene.render()
    steps = [dict(bones=_bones(api, scene, 1)), dict(morph_weights=(0.4, 0.2)), dict(pose=translation((0.1, 0.0, 0.0))), dict(bones=_bones(api, scene, 3))]
    for k, state in enumerate(steps):
        _set((scene, twin), **state)
        if k == 3:
            for s in (scene, twin):
                _look(api, s, (0.6, 1.0, 1.95))
        winner, matrix_u, u, f, got = _hold(api, scene, twin, f"without the flag, step {k}", ran=False)
        cube = (winner >= 0) & (winner < len(scene.models[0]._faces))
        if k < 2:
            assert np.abs(u).max() < 1e-6, "bones and weights move nothing without the flag"
        elif k == 2:
            assert np.hypot(u[cube, 0], u[cube, 1]).min() > 0.5 and _bits(got, f) > 0, "the pose moves the cube"
        else:
            assert np.hypot(u[..., 0], u[..., 1]).max() > 1 and _bits(got, f) > 0, "the camera moves the frame"
    assert scene.__dict__["_motion_faces_frame"] is None
    assert scene._backend().motion_faces_debug() == (0, 0, 0, 0)
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 2. the serial
def test_a_commit_in_between_skips_the_pass(api):
    """The snapshot must hold exactly the state the previous frame was rendered from.  A commit between two frames uploads
    the vertices again: the pass is skipped and counted, and U is k_velocity's.  The frame after that runs it again."""
    scene, twin = _pair(api)
    backend = scene._backend()
    scene.render()
    _set((scene, twin), bones=_bones(api, scene, 0))
    _hold(api, scene, twin, "before the commit")
    serial = backend.vertices_serial()
    _set((scene, twin), bones=_bones(api, scene, 1))
    scene.models[0].invalidate()                                      # (the scene goes to the library again: a commit)
    winner, matrix_u, u, _, _ = _hold(api, scene, twin, "behind a commit", ran=False)
    assert backend.vertices_serial() >= serial + 2, "a commit and a pass: two more states"
    assert _bits(u, matrix_u) == 0
    _set((scene, twin), bones=_bones(api, scene, 2))
    _, matrix_u, u, _, _ = _hold(api, scene, twin, "the frame after")
    assert _bits(u, matrix_u) > 0
    ran, skipped, _, snapshots = backend.motion_faces_debug()
    assert (ran, skipped) == (2, 1) and snapshots >= 3
    scene.close(), twin.close()


@pytest.mark.parametrize("tracked", (False, True), ids=("tracking_off", "tracking_on"))
def test_a_render_mean_in_between_skips_the_pass(api, tracked):
    """Sub-frames of an accumulation between two frames: their pose passes rewrite the vertices without any commit, so the
    snapshot the next frame's pass takes is of the last sub-frame's state, not of the previous frame's.  accumulate() refuses
    a scene with motion_blur, and assigning motion_blur forgets the previous frame, so the test takes the blur off behind the
    setter's back and puts it and the previous state back: what a caller of the C ABI can do freely.  The first sub-frame
    switches tracking off with the blur; with *tracked* the later ones run with it on again, so the snapshot itself moves
    past prev_serial.  Either way the frame after the mean skips the pass, counts it, and its U is k_velocity's."""
    scene, twin = _pair(api)
    backend = scene._backend()
    scene.render()
    _set((scene, twin), bones=_bones(api, scene, 0))
    _hold(api, scene, twin, "before the mean")
    blur, previous, serial = scene.motion_blur, scene.__dict__["_motion_prev"], backend.vertices_serial()
    assert previous.serial == serial
    commits, snapshots = backend.pose_counters()[0], backend.motion_faces_debug()[3]
    scene.motion_blur = None

    def step(k):
        if tracked and k >= 1:
            assert backend.lib.mr_scene_track_vertices(backend.handle, 1) == 0
        scene.models[0].bones = _bones(api, scene, 1 + k)

    scene.render_mean(3, step)
    scene.__dict__["_motion_blur"], scene.__dict__["_motion_prev"] = blur, previous
    assert backend.pose_counters()[0] == commits, "the sub-frames were committed: this is the other test's case"
    assert backend.vertices_serial() == serial + 3, "three passes, three more states"
    assert backend.motion_faces_debug()[3] == snapshots + (2 if tracked else 0)
    _set((scene, twin), bones=_bones(api, scene, 5))
    before = backend.motion_faces_debug()
    winner, matrix_u, u, _, _ = _hold(api, scene, twin, "behind a render_mean", ran=False)
    after = backend.motion_faces_debug()
    assert (after[0], after[1]) == (before[0], before[1] + 1), "the pass was not skipped and counted"
    assert np.frombuffer(scene.__dict__["_motion_faces_frame"][2], dtype=np.int32).tolist() == [1, 0]
    assert scene.__dict__["_motion_faces_frame"][3] == serial and after[3] == before[3] + 1, "the frame's own pass took a snapshot, of another state"
    assert _bits(u, matrix_u) == 0 and np.abs(u).max() < 1e-6, "U is not k_velocity's"
    _set((scene, twin), bones=_bones(api, scene, 6))
    _, matrix_u, u, _, _ = _hold(api, scene, twin, "the frame after")
    assert _bits(u, matrix_u) > 0
    scene.close(), twin.close()


def test_reset_motion_forgets_the_bones_too(api):
    scene, twin = _pair(api)
    scene.render()
    _set((scene, twin), bones=_bones(api, scene, 0))
    _hold(api, scene, twin, "bones")
    _set((scene, twin), bones=_bones(api, scene, 2))
    scene.reset_motion()
    before = scene._backend().motion_faces_debug()
    assert np.array_equal(scene.render(), twin.render()), "no previous frame: render()'s bytes"
    assert scene._backend().motion_faces_debug()[:2] == before[:2], "nothing flagged: neither run nor skipped"
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 3. the issue order
def _sequence(api, scene):
    """Three steps of bones and weights, each seen from two views: (state, views) pairs."""
    views = [[((0.5, 1, 2), (0, 0, 0)), ((0.56, 1, 1.97), (0, 0, 0))], [((0.56, 1, 1.97), (0, 0, 0)), ((0.5, 1.05, 2.0), (0.03, 0, 0))]]
    cams = [[(api.Camera(p, c, **KW), api.Camera(p, c, **KW)) for p, c in pair] for pair in views]
    return [(dict(bones=_bones(api, scene, 0)), cams[0]), (dict(bones=_bones(api, scene, 2), morph_weights=(0.6, 0.3)), cams[1])]


@pytest.fixture(scope="module")
def one_by_one(api):
    scene, _ = _pair(api)
    frames, flagged = [], []
    for state, views in _sequence(api, scene):
        _set((scene,), **state)
        for view in views:
            scene.camera, scene.debug_camera = view
            frames.append(scene.render().copy())
            flagged.append(np.frombuffer(scene.__dict__["_motion_faces_frame"][2], dtype=np.int32).tolist())
    assert flagged == [[0, 0], [0, 0], [1, 0], [0, 0]], "only the first view after a change has deforming models"
    assert scene._backend().motion_faces_debug()[:2] == (1, 0)
    scene.close()
    return frames


def test_render_frames_is_the_views_one_by_one(api, one_by_one):
    scene, _ = _pair(api)
    got = []
    for state, views in _sequence(api, scene):
        _set((scene,), **state)
        got += [frame.copy() for frame in scene.render_frames(views, depth=2)]
    for k, (a, b) in enumerate(zip(got, one_by_one)):
        assert np.array_equal(a, b), f"view {k}: {int((a != b).sum())} bytes differ"
    assert scene._backend().motion_faces_debug()[:2] == (1, 0)
    scene.close()


def test_render_async_is_the_views_one_by_one(api, one_by_one):
    scene, _ = _pair(api)
    got = []
    for state, views in _sequence(api, scene):
        _set((scene,), **state)
        pending = []
        for view in views:
            scene.camera, scene.debug_camera = view
            pending.append(scene.render_async())
        got += [frame.result().copy() for frame in pending]
    for k, (a, b) in enumerate(zip(got, one_by_one)):
        assert np.array_equal(a, b), f"view {k}"
    scene.close()


def test_a_frame_that_overflows_ends_with_the_unstarved_frame(api):
    def sequence(squeeze, through_frames):
        scene, _ = _pair(api)
        scene.render()
        backend = scene._backend()
        _set((scene,), bones=_bones(api, scene, 1))
        if squeeze:
            backend.set_list_capacities(**SQUEEZED)
        _look(api, scene, (0.56, 1.0, 1.97))
        view = (scene.camera, scene.debug_camera)
        before = backend.motion_debug()[0]
        out = next(iter(scene.render_frames([view]))).copy() if through_frames else scene.render().copy()
        got = out, backend.read_frame_f32().copy(), backend.read_velocity().copy(), backend.motion_debug()[0] - before, backend.motion_faces_debug()
        scene.close()
        return got

    want_rgb, want, want_u, unstarved, counts = sequence(False, False)
    assert counts[:2] == (1, 0)
    for through_frames in (False, True):
        got_rgb, got, got_u, enqueued, counts = sequence(True, through_frames)
        print(f"the pass enqueued {enqueued} times with the lists squeezed, {unstarved} without; per-face pass (ran, skipped) {counts[:2]}")
        assert enqueued >= 2 and enqueued > unstarved, "the frame did not overflow"
        assert counts[0] == enqueued and counts[1] == 0, "every attempt ran the per-face pass from the same snapshot"
        assert _bits(got_u, want_u) == 0 and _bits(got, want) == 0 and np.array_equal(got_rgb, want_rgb)
