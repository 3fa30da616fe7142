"""GPU: ``Scene.temporal_aa`` -- jittered frames blended over a reprojected history on the device (k_taa in kernels_taa.h,
host_taa.h, launch_after_tile in host_frame.h), the history the library keeps and the bookkeeping of the Python layer.

The yardstick: the host mirror ``mr_host_taa`` (held to the NumPy restatement taa_ref.py in test_taa_cpu.py) applied to
the float frame F that a TWIN of the scene -- the same recipe, camera and poses, no ``temporal_aa``, the frame's own
``_sample_jitter`` -- hands out through its tap, to U = ``read_velocity()`` and to the history P read before the frame.
The float frame and ``read_history()`` must match bit for bit, and the frame's bytes must be
``mr_host_accum([F'], [1], scale=1)`` byte for byte."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the capacities of test_accumulate_gpu.py's overflow test
SMALL = (120, 160)
KW = dict(fovy=60, near=0.1, far=20, backface_culling=True)
PAN = [((0.5, 1.0, 2.0), None), ((0.53, 1.0, 1.98), (0.05, 0.0, -0.02)), ((0.56, 1.01, 1.97), (0.09, 0.0, -0.03)),
       ((0.56, 1.01, 1.97), (0.09, 0.0, -0.03)), ((0.6, 1.0, 1.95), None)]         # (camera position, translation of model 0)


def _taa(blend=0.1, jitter=8):
    from py_numpy_renderer_amd import TemporalAA
    return TemporalAA(blend=blend, jitter=jitter)


def _bits(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def _look(api, scene, position, center=(0, 0, 0)):
    """Both cameras of *scene* at a new place (the debug camera clips like the camera)."""
    scene.camera, scene.debug_camera = api.Camera(position, center, **KW), api.Camera(position, center, **KW)


def _step(api, scene, place):
    from py_numpy_renderer_amd import translation
    position, move = place
    _look(api, scene, position)
    scene.models[0].pose = None if move is None else np.asarray(translation(move), dtype=np.float64)


def _pair(api, recipe=scenes.cube_outward, resolution=SMALL, taa=None, **settings):
    """The scene with temporal AA and its twin without; *settings* go to both."""
    scene, twin = recipe(api, resolution=resolution), recipe(api, resolution=resolution)
    for s in (scene, twin):
        for name, value in settings.items():
            setattr(s, name, value)
    scene.temporal_aa = taa if taa is not None else _taa()
    return scene, twin


def _history(scene):
    backend = scene._backend()
    return backend.read_history().copy() if backend.taa_debug()[5] else None


def _twin_taps(twin, jitter):
    """(Z, winner, F) of the twin as it is now under the sub-sample offset *jitter*: the frame in front of the pass."""
    twin.__dict__["_sample_jitter"] = jitter
    backend = twin._backend()
    backend.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=False)
    return backend.read_z().copy(), backend.read_winner().copy(), backend.read_frame_f32().copy()


def _hold(scene, twin, label):
    """Renders the scene's next frame and holds it to the mirror on the twin's tap; returns (F, U, P, F')."""
    from py_numpy_renderer_amd import _native
    assert not scene.draw_debug_frustum
    history = _history(scene)
    out = scene.render().copy()
    backend = scene._backend()
    got, u, kept = backend.read_frame_f32().copy(), backend.read_velocity().copy(), backend.read_history().copy()
    blend, jitter = scene.__dict__["_taa_frame"][0], scene.__dict__["_taa_frame"][4]
    assert "_sample_jitter" not in scene.__dict__, "the offset outlived the frame it was issued for"
    _, _, f = _twin_taps(twin, jitter)
    want = _native.host_taa(f, u, history, blend)
    s = scene.supersample
    _, want_rgb = _native.host_accum(got[None], [1.0], shift={1: 0, 2: 1, 4: 2}[s], scale=1.0, want_acc=False)
    bits, bits_kept = _bits(got, want), _bits(kept, want)
    steps = int(np.abs(out.astype(np.int16) - want_rgb.astype(np.int16)).max())
    print(f"{label}: jitter {jitter}, {'no' if history is None else 'a'} history, {bits} floats of the frame and {bits_kept} of the history "
          f"differ from the mirror, bytes differ by at most {steps}, |U| up to {np.hypot(u[..., 0], u[..., 1]).max():.2f}, "
          f"{_bits(got, f)} of {f.size} floats changed")
    assert got.shape == f.shape == kept.shape and u.shape == f.shape[:2] + (2,) and out.shape == want_rgb.shape
    assert bits == 0, f"{label}: the float frame is not mr_host_taa's"
    assert bits_kept == 0, f"{label}: the history is not the frame as k_taa left it"
    assert steps == 0, f"{label}: the bytes are not the finalise of the float frame"
    return f, u, history, got


# ---------------------------------------------------------------------------- 1. the frames against the mirror
@pytest.mark.parametrize("settings", [dict(), dict(supersample=2), dict(ambient_occlusion=True)], ids=["alone", "supersample2", "obscurance"])
def test_a_pan_with_a_posed_model_is_the_mirror_frame_by_frame(api, settings):
    from py_numpy_renderer_amd import AmbientOcclusion
    settings = dict(settings)
    if settings.pop("ambient_occlusion", False):
        settings["ambient_occlusion"] = AmbientOcclusion()
    resolution = (60, 80) if settings.get("supersample") else SMALL
    scene, twin = _pair(api, resolution=resolution, taa=_taa(blend=0.2, jitter=4), **settings)
    moved = blended = 0
    for k, place in enumerate(PAN):
        for s in (scene, twin):
            _step(api, s, place)
        f, u, history, got = _hold(scene, twin, f"cube_outward {settings}, frame {k}")
        assert (history is None) == (k == 0)
        moved += int(np.abs(u).max() > 0.5)
        blended += int(_bits(got, f) > 0)
    backend = scene._backend()
    grid = tuple(resolution[i] * scene.supersample for i in (0, 1))
    assert moved >= 3 and blended >= 4 and backend.taa_debug() == (len(PAN),) + grid + (len(PAN), len(PAN), 1)
    if "ambient_occlusion" in settings:
        assert backend.ao_debug()[0] == len(PAN)
    times = backend.taa_times()
    assert times["velocity"] > 0 and times["taa"] > 0
    assert backend.motion_debug() == (0, 0, 0), "k_mblur ran without a motion blur"
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 2. identities
def test_the_first_frame_after_every_forgetting_event_is_render_s(api):
    from py_numpy_renderer_amd import MotionBlur
    scene, twin = _pair(api, resolution=(60, 80))
    for event in ("assigned", "reset_motion", "temporal_aa", "motion_blur", "supersample", "resolution", "models"):
        if event == "reset_motion":
            scene.reset_motion()
        elif event == "temporal_aa":
            scene.temporal_aa = _taa(blend=0.3)
        elif event == "motion_blur":
            scene.motion_blur = MotionBlur()
        elif event == "supersample":
            scene.supersample = twin.supersample = 2
        elif event == "resolution":
            scene.resolution = twin.resolution = (64, 80)
        elif event == "models":
            for s in (scene, twin):
                s.models.append(s.models.pop(0))
        first, plain = scene.render().copy(), twin.render().copy()
        assert np.array_equal(first, plain), f"{event}: the first frame differs from render() in {int((first != plain).sum())} bytes"
        assert scene._backend().taa_debug()[5] == 1
        later = [scene.render().copy() for _ in range(3)]              # jittered frames over a history: no longer render()'s
        assert not all(np.array_equal(x, plain) for x in later), f"{event}: the jitter changed nothing"
        _look(api, scene, (0.55, 1.0, 1.97)), _look(api, twin, (0.55, 1.0, 1.97))
        scene.render()
        _look(api, scene, (0.5, 1.0, 2.0)), _look(api, twin, (0.5, 1.0, 2.0))
    scene.close(), twin.close()


def test_without_jitter_a_still_scene_repeats_render_s_bytes(api):
    scene, twin = _pair(api, taa=_taa(blend=0.1, jitter=0))
    plain = twin.render().copy()
    for k in range(5):
        frame = scene.render()
        assert np.array_equal(frame, plain), f"frame {k}: {int((frame != plain).sum())} bytes differ"
        # (U at rest is zero or a few 1e-14 -- (x * Z) / Z is x to within an ulp of float64 -- so x - U.x is x in float32:
        # the history is fetched at integer positions)
        u = scene._backend().read_velocity()
        ys, xs = np.mgrid[0:SMALL[0], 0:SMALL[1]]
        assert np.abs(u).max() < 1e-9
        assert np.array_equal(xs.astype(np.float32) - u[..., 0], xs) and np.array_equal(ys.astype(np.float32) - u[..., 1], ys)
    assert scene._backend().taa_debug()[:1] + scene._backend().taa_debug()[3:] == (5, 5, 5, 1)
    scene.close(), twin.close()


def test_a_scene_without_temporal_aa_issues_what_it_did(api):
    from py_numpy_renderer_amd import MotionBlur
    scene = scenes.cube_outward(api, resolution=SMALL)
    scene.render()
    backend = scene._backend()
    assert backend.taa_debug() == (0,) * 6 and backend.motion_debug() == (0, 0, 0)
    with pytest.raises(RuntimeError, match="no frame with temporal anti-aliasing"):
        backend.taa_times()
    scene.motion_blur = MotionBlur()
    for k in range(3):
        _look(api, scene, (0.5 + 0.03 * k, 1.0, 2.0))
        scene.render()
        assert backend.motion_debug()[0] == k + 1 and backend.taa_debug() == (0,) * 6
        assert backend.motion_times()["velocity"] > 0, "the motion blur's own k_velocity ran"
    scene.close()


# ---------------------------------------------------------------------------- 3. it anti-aliases
def test_a_still_scene_converges_towards_the_supersampled_frame(api):
    """32 frames of a still scene under jitter=8: on the pixels where render() and the supersample = 4 frame differ, the
    mean absolute error of the temporal-AA frame against the supersample = 4 frame is below render()'s own.  Two measured
    errors on the same pixels, no threshold."""
    scene, twin = _pair(api, taa=_taa(blend=0.1, jitter=8))
    plain = twin.render().astype(np.float64)
    twin.supersample = 4
    fine = twin.render().astype(np.float64)
    for _ in range(31):
        scene.render()
    got = scene.render().astype(np.float64)
    edge = (plain != fine).any(axis=-1)
    err_plain, err_taa = np.abs(plain - fine)[edge].mean(), np.abs(got - fine)[edge].mean()
    print(f"cube_outward {SMALL}: {int(edge.sum())} of {edge.size} pixels differ between render() and supersample = 4; mean absolute error there, "
          f"in steps of 1/255: render() {err_plain:.3f}, temporal AA after 32 frames {err_taa:.3f}")
    assert edge.sum() > 200
    assert err_taa < err_plain
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 4. composition and order
def test_in_front_of_the_depth_of_field_and_the_motion_blur(api):
    from py_numpy_renderer_amd import DepthOfField, MotionBlur, _native, _pack
    scene, twin = _pair(api, taa=_taa(blend=0.25, jitter=4))
    scene.depth_of_field = DepthOfField(lens_radius=0.1)
    scene.motion_blur = MotionBlur(shutter=1.0)
    face_off = np.cumsum([0] + [len(m._faces) for m in scene.models])[:-1].astype(np.int32)
    backend = scene._backend()
    for k, place in enumerate(PAN):
        for s in (scene, twin):
            _step(api, s, place)
        history = _history(scene)
        out = scene.render().copy()
        got, u, kept = backend.read_frame_f32().copy(), backend.read_velocity().copy(), backend.read_history().copy()
        blend, matrices, background, class_of, jitter = scene.__dict__["_taa_frame"]
        shutter, depth_map = scene.__dict__["_motion_frame"][:2]
        assert scene.__dict__["_motion_frame"][2:] == (matrices, background, class_of), "the two descriptions carry other tables"
        z, winner, f = _twin_taps(twin, jitter)
        motion = _native.fill_motion_desc(depth_map, shutter, np.frombuffer(matrices, dtype=np.float64), np.frombuffer(background, dtype=np.float64),
                                          np.frombuffer(class_of, dtype=np.int32))
        want_u = _native.host_velocity(z, winner, face_off, motion)
        stable = _native.host_taa(f, want_u, history, blend)
        lens = _native.host_dof(z, stable, _native.fill_dof_desc(*_pack.dof_constants(scene)))
        want = _native.host_motion_blur(z, want_u, lens, motion)
        _, want_rgb = _native.host_accum(got[None], [1.0], shift=0, scale=1.0, want_acc=False)
        print(f"frame {k}: {_bits(u, want_u)} velocity floats, {_bits(kept, stable)} history floats and {_bits(got, want)} floats of the frame differ "
              f"from the mirrors chained; the lens changed {_bits(lens, stable)} floats, the blur {_bits(want, lens)}")
        assert _bits(u, want_u) == 0 and _bits(kept, stable) == 0, "the history is not the frame as k_taa left it"
        assert _bits(got, want) == 0, "the frame is not k_taa, k_dof, k_mblur in that order"
        assert np.array_equal(out, want_rgb)
        assert _bits(lens, stable) > 0 and (k in (0, 3) or _bits(want, lens) > 0)
        # one k_velocity a frame: the one in front of k_taa; the motion blur went straight to k_mblur
        assert backend.taa_debug()[3] == k + 1 and backend.motion_debug()[0] == k + 1 and backend.dof_debug()[0] == k + 1
        assert backend.motion_times()["velocity"] == 0.0 and backend.motion_times()["mblur"] > 0 and backend.taa_times()["velocity"] > 0
    scene.close(), twin.close()


def test_the_overlay_goes_on_top_and_stays_out_of_the_history(api):
    scene, twin = _pair(api, taa=_taa(blend=0.1, jitter=0))
    scene.draw_debug_frustum = twin.draw_debug_frustum = True
    for s in (scene, twin):
        dbg = s.debug_camera
        s.camera = api.Camera((0.6, 1.0, 1.95), (0, 0, 0), **KW)
        s.debug_camera = dbg                                   # (its frustum is what the overlay draws)
    scene.draw_debug_frustum = True
    for _ in range(2):
        out = scene.render().copy()
    backend = scene._backend()
    got, kept = backend.read_frame_f32().copy(), backend.read_history().copy()
    tb = twin._backend()
    tb.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=True)
    with_lines = tb.read_frame_f32().copy()
    tb.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=False)
    bare = tb.read_frame_f32().copy()
    assert 0 < _bits(with_lines, bare) < bare.size // 4, "the plain scene's overlay drew nothing, or everything"
    assert _bits(got, with_lines) == 0, "the lines are not on top of the stabilised frame"
    assert _bits(kept, bare) == 0, "the history holds the overlay's lines"
    assert np.array_equal(out, twin.render())
    scene.close(), twin.close()


def _views(api):
    places = [((0.5, 1, 2), (0, 0, 0)), ((0.54, 1, 1.98), (0, 0, 0)), ((0.54, 1, 1.98), (0, 0, 0)), ((0.5, 1.05, 2.0), (0.03, 0, 0))]
    return [(api.Camera(p, c, **KW), api.Camera(p, c, **KW)) for p, c in places]


def test_render_frames_is_the_views_one_by_one(api):
    scene, _ = _pair(api, resolution=(60, 80))
    one_by_one = []
    for view in _views(api):
        scene.camera, scene.debug_camera = view
        one_by_one.append(scene.render().copy())
    assert len({hashlib.sha256(f.tobytes()).hexdigest() for f in one_by_one}) == len(one_by_one)
    for depth in (1, 3):
        scene.reset_motion()
        got = [frame.copy() for frame in scene.render_frames(_views(api), depth=depth)]
        assert len(got) == len(one_by_one)
        for k, (a, b) in enumerate(zip(got, one_by_one)):
            assert np.array_equal(a, b), f"depth {depth}, view {k}: {int((a != b).sum())} bytes differ"
    scene.close()


# ---------------------------------------------------------------------------- 5. overflow
def test_a_frame_that_overflows_ends_with_the_unstarved_frame_and_its_history(api):
    def sequence(squeeze, through_frames):
        scene = scenes.build(api, "diablo_floor_small")
        scene.temporal_aa = _taa(blend=0.2, jitter=4)
        scene.render()
        backend = scene._backend()
        if squeeze:
            backend.set_list_capacities(**SQUEEZED)
        _look(api, scene, (0.56, 1.0, 1.97))
        view = (scene.camera, scene.debug_camera)
        before = backend.taa_debug()
        out = next(iter(scene.render_frames([view]))).copy() if through_frames else scene.render().copy()
        after = backend.taa_debug()
        got = out, backend.read_frame_f32().copy(), backend.read_history().copy(), after[0] - before[0], after[4] - before[4]
        third = scene.render().copy()                       # (the frame behind it reads that history)
        scene.close()
        return got + (third,)

    want_rgb, want, want_kept, unstarved, adopted, want_third = sequence(False, False)
    assert (unstarved, adopted) == (1, 1)
    for through_frames in (False, True):
        got_rgb, got, kept, enqueued, adopted, third = sequence(True, through_frames)
        print(f"the pass enqueued {enqueued} times with the lists squeezed, {unstarved} without; histories handed over: {adopted}")
        assert enqueued >= 2, "the frame did not overflow"
        assert adopted == 1, "an attempt that overflowed handed its history over"
        assert _bits(got, want) == 0 and _bits(kept, want_kept) == 0 and np.array_equal(got_rgb, want_rgb)
        assert np.array_equal(third, want_third)


# ---------------------------------------------------------------------------- 6. refusals on the device path
def test_refusals_and_switching_off(api):
    from py_numpy_renderer_amd import MotionBlur, _native
    scene = scenes.cube_outward(api, resolution=(64, 96))
    parent = scene.render().copy()
    backend = scene._backend()
    lib = backend.lib
    with pytest.raises(ValueError, match="no temporal anti-aliasing history"):
        backend.read_history()
    band_desc, shape = backend._prepare_desc(scene, True, (0, 32), False, False, False, False, None, False, False)
    band_desc = _native.FrameDesc.from_buffer_copy(band_desc)
    scene.temporal_aa = _taa()
    assert np.array_equal(scene.render(), parent) and backend.taa_debug() == (1, 64, 96, 1, 1, 1)
    # split frames
    with pytest.raises(ValueError, match="whole frames"):
        scene.render(row_band=(0, 32))
    out = np.zeros(shape, dtype=np.uint8)
    assert lib.mr_render(backend.handle, C.byref(band_desc), out.ctypes.data, None) == _native.MR_E_INVALID
    assert b"temporal anti-aliasing takes whole frames" in lib.mr_last_error() and not out.any()
    with pytest.raises(ValueError, match="render_async"):
        backend.render_device(scene, 0)
    # the accumulation
    with pytest.raises(ValueError, match="accumulate"):
        scene.render_mean(2, lambda k: None)
    # a second frame while one is pending: the Python layer, and the library behind it
    pending = scene.render_async()
    with pytest.raises(ValueError, match="one frame of the scene at a time"):
        scene.render_async()
    with pytest.raises(ValueError, match="one frame of the scene at a time"):
        scene.render()
    pending.result()
    assert backend.taa_debug()[0] == 2
    desc, shape = backend._prepare_desc(scene, True, None, False, False, False, False, None, False, False)
    desc = _native.FrameDesc.from_buffer_copy(desc)
    first, second = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    assert lib.mr_render_async(backend.handle, C.byref(desc), first.ctypes.data, 0) == 0, lib.mr_last_error()
    assert lib.mr_render_async(backend.handle, C.byref(desc), second.ctypes.data, 1) == _native.MR_E_INVALID
    assert b"has not been waited for" in lib.mr_last_error()
    assert lib.mr_render(backend.handle, C.byref(desc), second.ctypes.data, None) == _native.MR_E_INVALID
    assert b"has not been waited for" in lib.mr_last_error()
    assert lib.mr_render_wait(backend.handle, 0, None) == 0 and not second.any() and first.any()
    assert backend.taa_debug()[0] == 3 and backend.taa_debug()[4] == 3
    # table blocks that differ from the motion blur's
    scene.motion_blur = MotionBlur()
    _look(api, scene, (0.55, 1.0, 1.97))
    scene.render()
    _look(api, scene, (0.6, 1.0, 1.95))
    scene.render()
    shutter, depth_map, matrices, background, class_of = scene.__dict__["_motion_frame"]
    other = np.frombuffer(matrices, dtype=np.float64).copy()
    other[0] *= 0.5
    wrong = _native.fill_motion_desc(depth_map, shutter, other, np.frombuffer(background, dtype=np.float64), np.frombuffer(class_of, dtype=np.int32))
    assert lib.mr_scene_set_motion_blur(backend.handle, C.byref(wrong)) == 0
    before = backend.taa_debug()
    assert lib.mr_render(backend.handle, C.byref(desc), second.ctypes.data, None) == _native.MR_E_INVALID
    assert b"velocity tables are not the motion blur's" in lib.mr_last_error() and backend.taa_debug() == before
    backend._motion_key = None                                    # (the next frame hands the scene's own description over again)
    scene.render()
    # switching off: the scene enqueues what it did, and the history goes
    scene.motion_blur = None
    scene.temporal_aa = None
    _look(api, scene, (0.5, 1.0, 2.0))
    count = backend.taa_debug()[0]
    assert np.array_equal(scene.render(), parent) and backend.taa_debug()[0] == count and backend.taa_debug()[5] == 0
    with pytest.raises(ValueError, match="no temporal anti-aliasing history"):
        backend.read_history()
    assert scene.render(row_band=(0, 32)).shape == (32, 96, 3)           # (a band renders again)
    with scene.accumulate() as acc:                                     # (and so does an accumulation)
        acc.add(1.0)
        assert acc.result().shape == parent.shape
    scene.close()


# ---------------------------------------------------------------------------- 7. the workgroup shapes of k_taa behind a frame
_CHILD = r"""
import hashlib, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import scenes
from py_numpy_renderer_amd import TemporalAA
api = scenes.product_api()
scene = scenes.cube_outward(api, resolution=(75, 131))
scene.temporal_aa = TemporalAA(blend=0.2, jitter=4)
kw = dict(fovy=60, near=0.1, far=20, backface_culling=True)
for position in ((0.5, 1.0, 2.0), (0.55, 1.0, 1.97), (0.6, 1.0, 1.95)):
    scene.camera = scene.debug_camera = api.Camera(position, (0, 0, 0), **kw)
    scene.render()
print("digest", hashlib.sha256(np.ascontiguousarray(scene._backend().read_frame_f32()).tobytes()).hexdigest())
scene.close()
"""


@pytest.mark.parametrize("shape", ["64x4", "16x16"])
def test_every_workgroup_shape_gives_the_same_bits(api, shape):
    """MR_TAA_TILE is read once per process: a fresh child renders with each of the other two shapes."""
    assert "MR_TAA_TILE" not in os.environ, "this process renders the reference frame with a shape of its own"
    scene = scenes.cube_outward(api, resolution=(75, 131))
    scene.temporal_aa = _taa(blend=0.2, jitter=4)
    for position in ((0.5, 1.0, 2.0), (0.55, 1.0, 1.97), (0.6, 1.0, 1.95)):
        scene.camera = scene.debug_camera = api.Camera(position, (0, 0, 0), **KW)
        scene.render()
    want = hashlib.sha256(np.ascontiguousarray(scene._backend().read_frame_f32()).tobytes()).hexdigest()
    scene.close()
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MR_TAA_TILE=shape), timeout=300, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    lines = [ln.split()[1] for ln in proc.stdout.splitlines() if ln.startswith("digest ")]
    assert lines == [want], f"MR_TAA_TILE={shape}: the float frame is not the default shape's"
