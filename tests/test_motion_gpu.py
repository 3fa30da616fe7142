"""GPU: ``Scene.motion_blur`` -- the velocity buffer and the blur gathered along it on the device (k_velocity and k_mblur in
kernels_motion.h, host_motion.h, launch_after_tile in host_frame.h), and the previous state the Python layer keeps.

The yardstick: the host mirrors ``mr_host_velocity`` and ``mr_host_motion_blur`` (held to the NumPy restatement
motion_ref.py in test_motion_cpu.py) applied to the z-buffer Z, the winner map and the float frame F that a TWIN of the
scene -- the same recipe, camera and poses, without ``motion_blur`` -- hands out through its taps, with the matrices the
scene handed to the library.  ``read_velocity()`` and the float frame F' must match bit for bit, the frame's bytes must be
``mr_host_accum([F'], [1], scale=1)`` byte for byte, and Z must be unchanged."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import motion_ref
import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the capacities of test_accumulate_gpu.py's overflow test
SMALL = (136, 152)                                                  # the cube-and-floor captures' size
KW = dict(fovy=60, near=0.1, far=20, backface_culling=True)


def _blur(shutter=1.0):
    from py_numpy_renderer_amd import MotionBlur
    return MotionBlur(shutter=shutter)


def _bits(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def _changed(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1)


def _look(api, scene, position, center=(0, 0, 0)):
    """Both cameras of *scene* at a new place (the debug camera clips like the camera)."""
    scene.camera, scene.debug_camera = api.Camera(position, center, **KW), api.Camera(position, center, **KW)


def _desc(scene):
    """The description the scene handed to the library with its last frame."""
    from py_numpy_renderer_amd import _native
    shutter, depth_map, matrices, background, class_of = scene.__dict__["_motion_frame"]
    return _native.fill_motion_desc(depth_map, shutter, np.frombuffer(matrices, dtype=np.float64), np.frombuffer(background, dtype=np.float64),
                                    np.frombuffer(class_of, dtype=np.int32))


def _face_off(scene):
    return np.cumsum([0] + [len(m._faces) for m in scene.models])[:-1].astype(np.int32)


def _twin_taps(twin):
    """(Z, winner, F) of the twin as it is now: the frame in front of the motion blur."""
    backend = twin._backend()
    backend.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=False)
    return backend.read_z().copy(), backend.read_winner().copy(), backend.read_frame_f32().copy()


def _hold(scene, twin, label, moving=True):
    """Renders the scene's next frame and holds it to the mirrors on the twin's taps; returns (Z, winner, F, U, F')."""
    from py_numpy_renderer_amd import _native
    assert not scene.draw_debug_frustum
    out = scene.render().copy()
    backend = scene._backend()
    got, u, z_after = backend.read_frame_f32().copy(), backend.read_velocity().copy(), backend.read_z().copy()
    z, winner, f = _twin_taps(twin)
    desc = _desc(scene)
    want_u = _native.host_velocity(z, winner, _face_off(scene), desc)
    want = _native.host_motion_blur(z, want_u, f, desc)
    s = scene.supersample
    _, want_rgb = _native.host_accum(got[None], [1.0], shift={1: 0, 2: 1, 4: 2}[s], scale=1.0, want_acc=False)
    h = motion_ref.segment(want_u, desc.shutter)[0]
    bits_u, bits = _bits(u, want_u), _bits(got, want)
    steps = int(np.abs(out.astype(np.int16) - want_rgb.astype(np.int16)).max())
    print(f"{label}: {bits_u} velocity floats and {bits} colour floats differ from the mirrors, bytes differ by at most {steps}, "
          f"|U| up to {np.hypot(u[..., 0], u[..., 1]).max():.2f}, h up to {h.max():.2f}, {_changed(got, f).mean():.1%} of {z.size} samples changed")
    assert u.shape == z.shape + (2,) and got.shape == f.shape and out.shape == want_rgb.shape
    assert bits_u == 0, f"{label}: read_velocity() is not mr_host_velocity's"
    assert bits == 0, f"{label}: the float frame is not the mirrors'"
    assert steps == 0, f"{label}: the bytes are not the finalise of the float frame"
    assert np.array_equal(z_after.view(np.uint64), z.view(np.uint64)), f"{label}: the z-buffer is not the twin's"
    assert (h.max() >= 1) == moving, f"{label}: h up to {h.max()}"
    return z, winner, f, u, got


def _pair(api, recipe=scenes.cube_outward, resolution=SMALL, **settings):
    """The scene with motion blur and its twin without; *settings* go to both."""
    scene, twin = recipe(api, resolution=resolution), recipe(api, resolution=resolution)
    for s in (scene, twin):
        for name, value in settings.items():
            setattr(s, name, value)
    scene.motion_blur = _blur()
    return scene, twin


# ---------------------------------------------------------------------------- 1. the frames against the mirrors
def test_the_first_frame_is_render_s_and_a_camera_move_is_the_mirrors(api):
    scene, twin = _pair(api)
    plain = twin.render().copy()
    assert scene._backend().motion_debug() == (0, 0, 0)
    first = scene.render().copy()
    assert np.array_equal(first, plain), f"the first frame differs from render() in {int((first != plain).sum())} bytes"
    assert scene._backend().motion_debug() == (1,) + SMALL
    for s in (scene, twin):
        _look(api, s, (0.6, 1.0, 1.95))
    z, winner, f, u, got = _hold(scene, twin, "cube_outward, camera moved")
    assert np.isfinite(z).any() and (~np.isfinite(z)).any() and (winner >= 0).any()
    assert _bits(got, f) > 0 and u[np.isfinite(z)].any() and u[~np.isfinite(z)].any(), "the camera turned: the sky moves too"
    times = scene._backend().motion_times()
    assert times["velocity"] > 0 and times["mblur"] > 0
    # nothing moves any more: the next frame is the plain frame of that view again
    assert np.array_equal(scene.render(), twin.render())
    scene.close(), twin.close()


def _dilate(mask, r):
    out = mask.copy()
    for d in range(1, r + 1):
        out[:, d:] |= mask[:, :-d]
        out[:, :-d] |= mask[:, d:]
    wide = out.copy()
    for d in range(1, r + 1):
        out[d:] |= wide[:-d]
        out[:-d] |= wide[d:]
    return out


def test_a_model_whose_pose_changes_over_a_still_floor(api):
    from py_numpy_renderer_amd import translation
    scene, twin = _pair(api)
    scene.render()
    for s in (scene, twin):
        s.models[0].pose = np.asarray(translation((0.12, 0.0, -0.05)), dtype=np.float64)
    z, winner, f, u, got = _hold(scene, twin, "cube_outward, the cube moved")
    cube = (winner >= 0) & (winner < len(scene.models[0]._faces))
    floor = winner >= len(scene.models[0]._faces)
    assert cube.sum() > 500 and floor.sum() > 500
    far = ~_dilate(cube, 16)
    assert (floor & far).sum() > 300 and not _changed(got, f)[far].any(), "a sample farther than 16 samples from the model changed"
    assert np.hypot(u[cube, 0], u[cube, 1]).min() > 1, "the model's samples do not move"
    assert np.abs(u[floor]).max() < 1e-6 and np.abs(u[winner < 0]).max() < 1e-6, "the still floor or the sky moves"
    assert _changed(got, f)[cube].any()
    scene.close(), twin.close()


def test_supersampled(api):
    scene, twin = _pair(api, resolution=(68, 76), supersample=2)
    assert np.array_equal(scene.render(), twin.render())
    for s in (scene, twin):
        _look(api, s, (0.58, 1.0, 1.96))
    z, winner, f, u, got = _hold(scene, twin, "cube_outward (68, 76), supersample 2")
    assert got.shape == (136, 152, 3) and scene._backend().motion_debug()[1:] == (136, 152) and _bits(got, f) > 0
    scene.close(), twin.close()


def test_behind_the_obscurance_and_the_depth_of_field(api):
    from py_numpy_renderer_amd import AmbientOcclusion, DepthOfField
    scene, twin = _pair(api, ambient_occlusion=AmbientOcclusion(), depth_of_field=DepthOfField(lens_radius=0.1))
    assert np.array_equal(scene.render(), twin.render())
    for s in (scene, twin):
        _look(api, s, (0.6, 1.0, 1.95))
    z, winner, f, u, got = _hold(scene, twin, "cube_outward, obscurance, depth of field and motion blur")
    backend = scene._backend()
    assert backend.ao_debug()[0] == 2 and backend.dof_debug()[0] == 2 and backend.motion_debug()[0] == 2
    assert _bits(got, f) > 0
    # (and the second float frame went back and forth: a third frame, at rest again, is the twin's)
    assert np.array_equal(scene.render(), twin.render())
    scene.close(), twin.close()


def test_the_overlay_goes_on_top_and_stays_sharp(api):
    from py_numpy_renderer_amd import _native
    frames = {}
    for overlay in (False, True):
        scene = scenes.cube_outward(api, resolution=SMALL)
        scene.motion_blur = _blur()
        scene.draw_debug_frustum = overlay
        dbg = scene.debug_camera
        scene.render()
        scene.camera = api.Camera((0.6, 1.0, 1.95), (0, 0, 0), **KW)
        scene.debug_camera = dbg                               # (its frustum is what the overlay draws)
        out = scene.render().copy()
        backend = scene._backend()
        frames[overlay] = (out, backend.read_frame_f32().copy(), backend.read_z().copy())
        scene.close()
    twin = scenes.cube_outward(api, resolution=SMALL)
    twin.camera = api.Camera((0.6, 1.0, 1.95), (0, 0, 0), **KW)
    backend = twin._backend()
    backend.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=False)
    plain_off = backend.read_frame_f32().copy()
    backend.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=True)
    plain_on, z_on = backend.read_frame_f32().copy(), backend.read_z().copy()
    twin.close()
    untouched = ~_changed(plain_off, plain_on)
    assert 0 < int((~untouched).sum()) < untouched.size // 4, "the plain scene's overlay drew nothing, or everything"
    (out_off, f_off, _), (out_on, f_on, z_blur) = frames[False], frames[True]
    assert _bits(f_off, plain_off) > 0, "the motion blur changed nothing"
    assert _bits(f_on[untouched], f_off[untouched]) == 0, "the overlay changed a sample its lines do not touch"
    assert np.array_equal(z_blur.view(np.uint64), z_on.view(np.uint64)), "Z is not the plain scene's after its overlay"
    _, want_rgb = _native.host_accum(f_on[None], [1.0], shift=0, scale=1.0, want_acc=False)
    assert np.array_equal(out_on, want_rgb)
    red = (plain_on == np.array([1.0, 0.0, 0.0], dtype=np.float32)).all(axis=-1) & ~untouched
    assert red.any() and _bits(f_on[red], plain_on[red]) == 0, "a line of the overlay was blurred"


# ---------------------------------------------------------------------------- 2. the previous state follows the issue order
def _views(api):
    places = [((0.5, 1, 2), (0, 0, 0)), ((0.58, 1, 1.96), (0, 0, 0)), ((0.58, 1, 1.96), (0, 0, 0)), ((0.5, 1.1, 2.0), (0.05, 0, 0)),
              ((0.42, 1.1, 2.05), (0.05, 0, 0))]
    return [(api.Camera(p, c, **KW), api.Camera(p, c, **KW)) for p, c in places]


@pytest.fixture(scope="module")
def one_by_one(api):
    """The views of _views rendered one by one through render(): the frames, and a plain frame per view."""
    scene, twin = _pair(api)
    frames, plain = [], []
    for view in _views(api):
        scene.camera, scene.debug_camera = view
        twin.camera, twin.debug_camera = view
        frames.append(scene.render().copy())
        plain.append(twin.render().copy())
    scene.close(), twin.close()
    same = [np.array_equal(a, b) for a, b in zip(frames, plain)]
    assert same == [True, False, True, False, False], "the first view and the repeated one are at rest, the others are not"
    return frames


def test_render_frames_is_the_views_one_by_one(api, one_by_one):
    scene, _ = _pair(api)
    for depth in (1, 3):
        scene.reset_motion()
        got = [frame.copy() for frame in scene.render_frames(_views(api), depth=depth)]
        assert len(got) == len(one_by_one)
        for k, (a, b) in enumerate(zip(got, one_by_one)):
            assert np.array_equal(a, b), f"depth {depth}, view {k}: {int((a != b).sum())} bytes differ"
    scene.close()


def test_render_async_is_the_views_one_by_one(api, one_by_one):
    scene, _ = _pair(api)
    pending = []
    for view in _views(api)[:4]:
        scene.camera, scene.debug_camera = view
        pending.append(scene.render_async())
    for k, frame in enumerate(pending):
        assert np.array_equal(frame.result(), one_by_one[k]), f"view {k}"
    scene.camera, scene.debug_camera = _views(api)[4]
    assert np.array_equal(scene.render(), one_by_one[4]), "render() behind render_async(): the previous state is the last one issued"
    scene.close()


def test_reset_motion_gives_render_s_bytes_again(api, one_by_one):
    scene, twin = _pair(api)
    views = _views(api)
    scene.camera, scene.debug_camera = views[0]
    scene.render()
    scene.camera, scene.debug_camera = twin.camera, twin.debug_camera = views[1]
    assert np.array_equal(scene.render(), one_by_one[1])
    scene.camera, scene.debug_camera = twin.camera, twin.debug_camera = views[3]
    scene.reset_motion()
    assert np.array_equal(scene.render(), twin.render())
    scene.close(), twin.close()


def test_a_frame_that_overflows_ends_with_the_unstarved_frame(api):
    def sequence(squeeze, through_frames):
        scene = scenes.build(api, "diablo_floor_small")
        scene.motion_blur = _blur()
        first = scene.render().copy()
        backend = scene._backend()
        if squeeze:
            backend.set_list_capacities(**SQUEEZED)
        _look(api, scene, (0.56, 1.0, 1.97))
        view = (scene.camera, scene.debug_camera)
        before = backend.motion_debug()[0]
        out = next(iter(scene.render_frames([view]))).copy() if through_frames else scene.render().copy()
        got = first, out, backend.read_frame_f32().copy(), backend.read_velocity().copy(), backend.motion_debug()[0] - before
        scene.close()
        return got

    first, want_rgb, want, want_u, unstarved = sequence(False, False)
    assert not np.array_equal(first, want_rgb)
    for through_frames in (False, True):
        _, got_rgb, got, got_u, enqueued = sequence(True, through_frames)
        print(f"the pass enqueued {enqueued} times with the lists squeezed, {unstarved} without")
        assert enqueued >= 2 and enqueued > unstarved, "the frame did not overflow"
        assert _bits(got_u, want_u) == 0 and _bits(got, want) == 0 and np.array_equal(got_rgb, want_rgb)


# ---------------------------------------------------------------------------- 3. refusals on the device path
def test_refusals_and_switching_off(api):
    from py_numpy_renderer_amd import _native, multigpu
    scene = scenes.cube_outward(api, resolution=(64, 96))
    parent = scene.render().copy()
    backend = scene._backend()
    assert backend.motion_debug() == (0, 0, 0)
    with pytest.raises(RuntimeError, match="no frame with motion blur"):
        backend.motion_times()
    with pytest.raises(RuntimeError, match="without motion blur"):
        backend.read_velocity()
    band_desc, shape = backend._prepare_desc(scene, True, (0, 32), False, False, False, False, None, False, False)
    band_desc = _native.FrameDesc.from_buffer_copy(band_desc)
    scene.motion_blur = _blur()
    assert np.array_equal(scene.render(), parent) and backend.motion_debug() == (1, 64, 96)
    with pytest.raises(ValueError, match="whole frames"):
        scene.render(row_band=(0, 32))
    out = np.zeros(shape, dtype=np.uint8)
    rc = backend.lib.mr_render(backend.handle, C.byref(band_desc), out.ctypes.data, None)
    assert rc == _native.MR_E_INVALID and b"motion blur takes whole frames" in backend.lib.mr_last_error()
    assert backend.motion_debug() == (1, 64, 96) and not out.any(), "the refused band reached the device"
    with pytest.raises(ValueError, match="motion_blur"):
        multigpu.BandRenderer(scene)
    with pytest.raises(ValueError, match="accumulate"):
        scene.render_mean(2, lambda k: None)
    scene.motion_blur = None
    _look(api, scene, (0.6, 1.0, 1.95))
    moved = scene.render().copy()
    assert backend.motion_debug() == (1, 64, 96), "the counter moved with motion_blur = None"
    assert not np.array_equal(moved, parent)
    assert backend.ao_debug() == (0, 0, 0) and backend.dof_debug() == (0, 0, 0)
    assert scene.render(row_band=(0, 32)).shape == (32, 96, 3)           # (a band renders again)
    with scene.accumulate() as acc:                                     # (and so does an accumulation)
        acc.add(1.0)
        assert acc.result().shape == moved.shape
    scene.close()


# ---------------------------------------------------------------------------- 4. the workgroup shapes of k_mblur
_PAN = dict(position=(0.8, 3, 4.8), up=(0, 1, 0), fovy=90, near=0.0001, far=400, backface_culling=False, center=(0.2, 0, 0))

_CHILD = r"""
import hashlib, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import scenes
from py_numpy_renderer_amd import MotionBlur
api = scenes.product_api()
scene = scenes.diablo_floor_lh_gl(api, resolution=(135, 240))
scene.motion_blur = MotionBlur(shutter=1.0)
scene.render()
pan = dict({pan!r})
scene.camera = api.Camera(pan.pop("position"), up=np.array(pan.pop("up")), **pan)
scene.render()
print("digest", hashlib.sha256(np.ascontiguousarray(scene._backend().read_frame_f32()).tobytes()).hexdigest())
scene.close()
"""


def _panned(api, scene):
    pan = dict(_PAN)
    scene.camera = api.Camera(pan.pop("position"), up=np.array(pan.pop("up")), **pan)


@pytest.fixture(scope="module")
def panned_digest(api):
    """The digest of the float frame of diablo_floor_lh_gl (135, 240) behind a pan of the camera, rendered here with
    whatever shape this process took (MR_MBLUR_TILE unset: the default's); the frame is not the unblurred one."""
    scene = scenes.diablo_floor_lh_gl(api, resolution=(135, 240))
    scene.motion_blur = _blur()
    scene.render()
    _panned(api, scene)
    scene.render()
    got = scene._backend().read_frame_f32().copy()
    scene.close()
    twin = scenes.diablo_floor_lh_gl(api, resolution=(135, 240))
    _panned(api, twin)
    _, _, plain = _twin_taps(twin)
    twin.close()
    changed = _changed(got, plain)
    print(f"the pan blurs {changed.mean():.1%} of {changed.size} samples")
    assert changed.sum() > changed.size // 10, "the second frame is not blurred: equal digests would show nothing"
    return hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()


@pytest.mark.parametrize("shape", ["32x32", "32x32x256", "16x16", "8x8"])
def test_every_workgroup_shape_gives_the_same_bits(panned_digest, shape):
    """MR_MBLUR_TILE is read once per process: a fresh child renders with each shape.  8x8 is a spelling the library does
    not know: it takes the default shape, so its digest is the default's as well."""
    assert "MR_MBLUR_TILE" not in os.environ, "this process rendered the reference frame with a shape of its own"
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), pan=_PAN)
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MR_MBLUR_TILE=shape), timeout=300, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    lines = [ln.split()[1] for ln in proc.stdout.splitlines() if ln.startswith("digest ")]
    assert lines == [panned_digest], f"MR_MBLUR_TILE={shape}: the float frame is not the default shape's"


# ---------------------------------------------------------------------------- 5. the staged tables grow under the slot's frames
def _own_velocity(scene, label):
    """``read_velocity()`` of the frame just rendered against ``mr_host_velocity`` on that frame's own z-buffer and
    winner map; returns (U, winner)."""
    from py_numpy_renderer_amd import _native
    backend = scene._backend()
    u, z, winner = backend.read_velocity().copy(), backend.read_z().copy(), backend.read_winner().copy()
    want = _native.host_velocity(z, winner, _face_off(scene), _desc(scene))
    bits = _bits(u, want)
    print(f"{label}: {bits} of {u.size} velocity floats differ from the mirror, |U| up to {np.hypot(u[..., 0], u[..., 1]).max():.2f}")
    assert bits == 0, f"{label}: read_velocity() is not mr_host_velocity's on the frame's own taps"
    return u, winner


def test_the_staged_tables_regrow_between_two_frames_of_one_slot(api):
    """A frame with one motion class, then one whose table block is more than twice as large, on the same slot: the
    page-locked copy (StagedTable, host_pass.h) is allocated for twice the bytes it was first asked for, so only such a step
    reaches the branch that frees it and allocates again, behind the wait for the upload that last read it.

    The frames are rendered back to back with ``render()``.  ``render_async`` and ``render_wait`` on one lane would not
    keep the first upload in flight either: a lane takes one frame at a time, and ``render_wait`` drains its stream
    before the next frame is staged."""
    from py_numpy_renderer_amd import _pack, translation
    pose = lambda *t: np.asarray(translation(t), dtype=np.float64)
    scene = scenes.cube_outward(api, resolution=(135, 240))
    for x in (-0.9, 0.9):
        cube = api.Model.load_model(os.path.join(scenes.ASSETS, "cube", "cube.obj")) @ api.scale(0.3)
        scene.add_model(cube)
        cube.pose = pose(x, 0.0, 0.3)
    scene.motion_blur = _blur()
    scene.render()

    def table_bytes():                     # (of the frame about to be issued: the block motion_params assembles)
        _, matrices, background, class_of, _ = _pack.motion_matrices(scene, scene.__dict__["_motion_prev"])
        return matrices.nbytes + background.nbytes + 2 * class_of.nbytes, int(class_of.max()) + 1

    _look(api, scene, (0.6, 1.0, 1.95))
    first_bytes, first_classes = table_bytes()
    scene.render()
    u, winner = _own_velocity(scene, "the camera moved")
    assert first_classes == 1 and u[winner >= 0].any()

    scene.models[0].pose = pose(0.1, 0.0, -0.05)
    scene.models[2].pose = pose(-0.8, 0.05, 0.3)
    scene.models[3].pose = pose(0.78, 0.05, 0.3)
    second_bytes, second_classes = table_bytes()
    print(f"table blocks of {first_bytes} and {second_bytes} bytes, {first_classes} and {second_classes} classes")
    assert second_classes == 4 and second_bytes > 2 * first_bytes, "the second table fits the first one's staging copy"
    scene.render()
    u, winner = _own_velocity(scene, "three models moved, each its own way")
    faces = np.cumsum([0] + [len(m._faces) for m in scene.models])
    moved = [np.hypot(*u[(winner >= faces[m]) & (winner < faces[m + 1])].mean(axis=0)) for m in (0, 2, 3)]
    floor = (winner >= faces[1]) & (winner < faces[2])
    assert min(moved) > 0.5 and np.abs(u[floor]).max() < 1e-6, f"the three models' mean |U| {moved}; the floor stays"
    assert scene._backend().motion_debug() == (3, 135, 240)
    scene.close()
