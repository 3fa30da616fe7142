"""GPU: ``Scene.bloom`` -- the glow from a resolution pyramid behind a frame's other passes (kernels_bloom.h, host_bloom.h,
launch_after_tile in host_frame.h) and the bookkeeping of the Python layer.

The yardstick: the host mirror ``mr_host_bloom`` (held to the NumPy restatement bloom_ref.py in test_bloom_cpu.py) applied to
the float frame F that a TWIN of the scene -- the same recipe, camera and poses, no ``bloom`` -- hands out through its tap,
run through the mirrors of the passes that stand in front.  The float frame must match bit for bit, and the frame's bytes
must be ``mr_host_accum([F'], [1], scale=1)`` byte for byte."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the capacities of test_accumulate_gpu.py's overflow test
SMALL = (120, 160)
KW = dict(fovy=60, near=0.1, far=20, backface_culling=True)
PAN = [((0.5, 1.0, 2.0), None), ((0.53, 1.0, 1.98), (0.05, 0.0, -0.02)), ((0.56, 1.01, 1.97), (0.09, 0.0, -0.03))]      # (camera position, translation of model 0)
SHIFT = {1: 0, 2: 1, 4: 2}


def _bloom(threshold=0.25, intensity=0.75, levels=4):
    from py_numpy_renderer_amd import Bloom
    return Bloom(threshold=threshold, intensity=intensity, levels=levels)


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


def _pair(api, recipe=scenes.cube_outward, resolution=SMALL, bloom=None, **settings):
    """The scene with bloom and its twin without; *settings* go to both."""
    scene, twin = recipe(api, resolution=resolution), recipe(api, resolution=resolution)
    for s in (scene, twin):
        s.draw_debug_frustum = False
        for name, value in settings.items():
            setattr(s, name, value)
    scene.bloom = bloom if bloom is not None else _bloom()
    return scene, twin


def _desc(scene):
    """The description the scene hands to the library for a frame of now."""
    from py_numpy_renderer_amd import _native, _pack
    return _native.fill_bloom_desc(*_pack.bloom_constants(scene))


def _twin_taps(twin, jitter=None):
    """(Z, winner, F) of the twin as it is now: the frame in front of every pass the twin does not have."""
    if jitter is not None:
        twin.__dict__["_sample_jitter"] = jitter
    backend = twin._backend()
    backend.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=False)
    twin.__dict__.pop("_sample_jitter", None)
    return backend.read_z().copy(), backend.read_winner().copy(), backend.read_frame_f32().copy()


def _bytes_of(frame, supersample=1):
    from py_numpy_renderer_amd import _native
    return _native.host_accum(frame[None], [1.0], shift=SHIFT[supersample], scale=1.0, want_acc=False)[1]


def _hold(scene, before, label):
    """Renders the scene's next frame and holds it to the bloom's mirror on *before*, the float frame in front of the pass."""
    from py_numpy_renderer_amd import _native
    out = scene.render().copy()
    got = scene._backend().read_frame_f32().copy()
    want = _native.host_bloom(before, _desc(scene))
    bits, glow = _bits(got, want), _bits(want, before)
    steps = int(np.abs(out.astype(np.int16) - _bytes_of(got, scene.supersample).astype(np.int16)).max())
    print(f"{label}: {bits} of {want.size} floats differ from the mirror, bytes differ by at most {steps}, the glow changed {glow} floats, "
          f"F up to {before.max():.3f}, F' up to {got.max():.3f}")
    assert got.shape == before.shape
    assert bits == 0, f"{label}: the float frame is not mr_host_bloom's"
    assert steps == 0, f"{label}: the bytes are not the finalise of the float frame"
    assert glow > 0, f"{label}: nothing glows: the pass was shown nothing"
    return out, got


# ---------------------------------------------------------------------------- 1. the frames against the mirror
@pytest.mark.parametrize("settings", [dict(), dict(supersample=2), dict(lights=3)], ids=["alone", "supersample2", "three_lights"])
def test_a_bloomed_frame_is_the_mirror_on_the_twin_s_tap(api, settings):
    settings = dict(settings)
    n_lights = settings.pop("lights", 1)
    resolution = (60, 80) if settings.get("supersample") else (121, 163)
    scene, twin = _pair(api, resolution=resolution, bloom=_bloom(levels=3), **settings)
    for s in (scene, twin):
        for position in ((-1.0, 2.0, 1.5), (2.0, 0.5, -1.0))[:n_lights - 1]:
            s.add_light(api.Light(position, color=(0.5, 0.5, 0.5), ambient_strength=0.1, specular_strength=0.3))
    for k, place in enumerate(PAN[:2]):
        for s in (scene, twin):
            _step(api, s, place)
        _hold(scene, _twin_taps(twin)[2], f"cube_outward {settings}, frame {k}")
    backend = scene._backend()
    s = scene.supersample
    assert backend.bloom_debug() == (2, resolution[0] * s, resolution[1] * s, 3 + SHIFT[s]), "levels + log2(supersample)"
    times = backend.bloom_times()
    assert times["down"] > 0 and times["up"] > 0 and times["composite"] > 0
    assert twin._backend().bloom_debug() == (0, 0, 0, 0)
    scene.close(), twin.close()


def test_a_threshold_no_sample_exceeds_gives_render_s_bytes(api):
    scene, twin = _pair(api, bloom=_bloom(threshold=0.9))
    for s in (scene, twin):                               # (a dim light: no sample reaches the clamp at 1, which exceeds every threshold a Bloom takes)
        s.light = api.Light((2, 3, 4), color=(0.4, 0.4, 0.4), ambient_strength=0.1, specular_strength=0.1)
    f = _twin_taps(twin)[2]
    assert 0.05 < f.max() <= 0.9, f"F up to {f.max()}: the scene is not what the test takes it for"
    out, plain = scene.render().copy(), twin.render().copy()
    assert np.array_equal(out, plain), f"{int((out != plain).sum())} bytes differ from render()"
    assert _bits(scene._backend().read_frame_f32(), f) == 0 and scene._backend().bloom_debug()[0] == 1, "the pass ran and changed no float"
    scene.bloom = _bloom(threshold=0.03)                   # the same frame glows under a threshold it exceeds
    _hold(scene, f, "the dim scene over a threshold of 0.03")
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 2. the other passes in front
def test_obscurance_temporal_aa_depth_of_field_and_motion_blur_stand_in_front(api):
    """Every pass on: the frame is the chain of mirrors k_ao, k_taa, k_dof, k_mblur, bloom on the plain twin's taps, and the
    history of temporal_aa is the frame as k_taa left it -- no glow in it."""
    from py_numpy_renderer_amd import AmbientOcclusion, DepthOfField, MotionBlur, TemporalAA, _native, _pack
    scene, twin = _pair(api, bloom=_bloom(levels=4))
    scene.ambient_occlusion = AmbientOcclusion()
    scene.temporal_aa = TemporalAA(blend=0.25, jitter=4)
    scene.depth_of_field = DepthOfField(lens_radius=0.1)
    scene.motion_blur = MotionBlur(shutter=1.0)
    face_off = np.cumsum([0] + [len(m._faces) for m in scene.models])[:-1].astype(np.int32)
    backend = scene._backend()
    for k, place in enumerate(PAN):
        for s in (scene, twin):
            _step(api, s, place)
        history = backend.read_history().copy() if backend.taa_debug()[5] else None
        out = scene.render().copy()
        got, kept = backend.read_frame_f32().copy(), backend.read_history().copy()
        blend, matrices, background, class_of, jitter = scene.__dict__["_taa_frame"]
        shutter, depth_map = scene.__dict__["_motion_frame"][:2]
        z, winner, f = _twin_taps(twin, jitter)
        motion = _native.fill_motion_desc(depth_map, shutter, np.frombuffer(matrices, dtype=np.float64), np.frombuffer(background, dtype=np.float64),
                                          np.frombuffer(class_of, dtype=np.int32))
        dark = _native.host_ao(z, f, _native.fill_ao_desc(scene.ambient_occlusion, *_pack.ao_constants(scene)))
        u = _native.host_velocity(z, winner, face_off, motion)
        stable = _native.host_taa(dark, u, history, blend)
        lens = _native.host_dof(z, stable, _native.fill_dof_desc(*_pack.dof_constants(scene)))
        blurred = _native.host_motion_blur(z, u, lens, motion)
        want = _native.host_bloom(blurred, _desc(scene))
        print(f"frame {k}: {_bits(got, want)} floats of the frame and {_bits(kept, stable)} of the history differ from the mirrors chained; "
              f"obscurance changed {_bits(dark, f)}, temporal AA {_bits(stable, dark)}, the lens {_bits(lens, stable)}, the blur {_bits(blurred, lens)}, "
              f"the glow {_bits(want, blurred)}")
        assert _bits(got, want) == 0, "the frame is not k_ao, k_taa, k_dof, k_mblur, bloom in that order"
        assert _bits(kept, stable) == 0, "the history is not the frame as k_taa left it: it holds glow"
        assert np.array_equal(out, _bytes_of(got))
        # (the obscurance finds no crease to darken in this scene: that k_ao ran is in the counts below)
        assert _bits(lens, stable) > 0 and _bits(want, blurred) > 0 and (k == 0 or _bits(blurred, lens) > 0)
        assert backend.bloom_debug()[0] == backend.ao_debug()[0] == backend.dof_debug()[0] == backend.motion_debug()[0] == backend.taa_debug()[0] == k + 1
    scene.close(), twin.close()


def test_the_overlay_is_drawn_over_the_glow_and_does_not_glow(api):
    from py_numpy_renderer_amd import _native
    scene, twin = _pair(api)
    for s in (scene, twin):
        dbg = s.debug_camera
        s.camera = api.Camera((0.6, 1.0, 1.95), (0, 0, 0), **KW)
        s.debug_camera = dbg                                   # (its frustum is what the overlay draws)
        s.draw_debug_frustum = True
    out = scene.render().copy()
    got = scene._backend().read_frame_f32().copy()
    tb = twin._backend()
    tb.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=True)
    with_lines = tb.read_frame_f32().copy()
    tb.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=False)
    bare = tb.read_frame_f32().copy()
    lines = (with_lines.view(np.uint32) != bare.view(np.uint32)).any(axis=-1)
    assert 0 < lines.sum() < lines.size // 4, "the plain scene's overlay drew nothing, or everything"
    glowing = _native.host_bloom(bare, _desc(scene))
    assert _bits(got[~lines], glowing[~lines]) == 0, "off the lines the frame is not the glow of the frame without them"
    # (the overlay blends a line's edge samples with what lies under them -- here the glowing frame, in the twin the bare one:
    # only the samples a line covers whole are the line's colour in both)
    solid = lines & (with_lines == np.float32([1.0, 0.0, 0.0])).all(axis=-1)
    assert solid.sum() > 20, "the overlay covers no sample whole"
    assert _bits(got[solid], with_lines[solid]) == 0, "a sample a line covers whole is not the line's colour: the lines glow, or lie under the glow"
    assert (glowing[solid] != with_lines[solid]).any(), "no glow lies under the lines: the test shows nothing"
    assert _bits(got, _native.host_bloom(with_lines, _desc(scene))) > 0, "bloom behind the overlay would give the same frame: the test shows nothing"
    assert np.array_equal(out, _bytes_of(got))
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 3. frames in flight, sums, overflow
def test_two_frames_in_flight_keep_their_own_bloom_and_pyramid(api):
    from py_numpy_renderer_amd import _native
    scene, twin = _pair(api)
    blooms = [_bloom(threshold=0.25, intensity=0.75, levels=2), _bloom(threshold=0.5, intensity=1.5, levels=5)]
    places = [(0.5, 1.0, 2.0), (0.6, 1.0, 1.95)]
    want = []
    for bloom, place in zip(blooms, places):
        _look(api, twin, place)
        scene.bloom = bloom
        want.append(_bytes_of(_native.host_bloom(_twin_taps(twin)[2], _desc(scene))))
    scene.render()                                       # (the work lists grow outside the pair)
    pending = []
    for bloom, place in zip(blooms, places):
        _look(api, scene, place)
        scene.bloom = bloom
        pending.append(scene.render_async())
    got = [p.result().copy() for p in pending]
    for k in range(2):
        assert np.array_equal(got[k], want[k]), f"frame {k}: {int((got[k] != want[k]).sum())} bytes differ"
    assert not np.array_equal(got[0], got[1]) and scene._backend().bloom_debug()[0] == 3 and scene._backend().bloom_debug()[3] == 5
    # render_frames: the same two views, two in flight
    scene.bloom = blooms[0]
    views = [(api.Camera(p, (0, 0, 0), **KW), api.Camera(p, (0, 0, 0), **KW)) for p in places]
    frames = [f.copy() for f in scene.render_frames(views, depth=2)]
    assert np.array_equal(frames[0], want[0]) and len(frames) == 2
    scene.close(), twin.close()


def test_render_mean_sums_bloomed_sub_frames(api):
    from py_numpy_renderer_amd import _native
    scene, twin = _pair(api, resolution=(60, 80))
    places = [(0.5, 1.0, 2.0), (0.53, 1.0, 1.98), (0.56, 1.01, 1.97)]
    subs = []
    for place in places:
        _look(api, twin, place)
        subs.append(_native.host_bloom(_twin_taps(twin)[2], _desc(scene)))
    _, want = _native.host_accum(np.stack(subs), [1.0] * 3, shift=0, scale=1.0 / 3.0, want_acc=False)
    got = scene.render_mean(3, lambda k: _look(api, scene, places[k]))
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from the mean of the mirrors' frames"
    assert scene._backend().bloom_debug()[0] == 3
    scene.close(), twin.close()


def test_a_frame_rendered_again_after_a_list_overflow_is_the_unstarved_frame(api):
    def frame(squeeze):
        scene = scenes.build(api, "diablo_floor_small")
        scene.draw_debug_frustum = False
        scene.bloom = _bloom()
        scene.render()
        backend = scene._backend()
        if squeeze:
            backend.set_list_capacities(**SQUEEZED)
        _look(api, scene, (0.56, 1.0, 1.97))
        before = backend.bloom_debug()[0]
        out = scene.render().copy()
        got = out, backend.read_frame_f32().copy(), backend.bloom_debug()[0] - before
        scene.close()
        return got

    want_rgb, want, once = frame(False)
    got_rgb, got, enqueued = frame(True)
    print(f"the pass enqueued {enqueued} times with the lists squeezed, {once} without")
    assert once == 1 and enqueued >= 2, "the frame did not overflow"
    assert _bits(got, want) == 0 and np.array_equal(got_rgb, want_rgb)


# ---------------------------------------------------------------------------- 4. switching off, refusals
def test_none_restores_the_old_frame_and_split_frames_are_refused(api):
    import ctypes as C
    from py_numpy_renderer_amd import _native
    scene = scenes.cube_outward(api, resolution=(64, 96))
    parent = scene.render().copy()
    backend = scene._backend()
    assert backend.bloom_debug() == (0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="no frame with bloom yet"):
        backend.bloom_times()
    band_desc, shape = backend._prepare_desc(scene, True, (0, 32), False, False, False, False, None, False, False)
    band_desc = _native.FrameDesc.from_buffer_copy(band_desc)
    scene.bloom = _bloom()
    bloomed = scene.render().copy()
    assert not np.array_equal(bloomed, parent) and backend.bloom_debug() == (1, 64, 96, 4)
    with pytest.raises(ValueError, match="whole frames"):
        scene.render(row_band=(0, 32))
    out = np.zeros(shape, dtype=np.uint8)
    assert backend.lib.mr_render(backend.handle, C.byref(band_desc), out.ctypes.data, None) == _native.MR_E_INVALID
    assert b"bloom takes whole frames" in backend.lib.mr_last_error() and not out.any()
    scene.bloom = None
    again = scene.render().copy()
    assert np.array_equal(again, parent), f"{int((again != parent).sum())} bytes differ from the frame before the pass"
    assert backend.bloom_debug()[0] == 1, "the pass ran with bloom = None"
    assert scene.render(row_band=(0, 32)).shape == (32, 96, 3)           # (a band renders again)
    scene.close()
