"""GPU: ``Scene.light_shafts`` -- the sky's light marched towards a light behind a frame's other passes and in front of its
bloom (kernels_shafts.h, host_shafts.h, launch_after_tile in host_frame.h) and the bookkeeping of the Python layer.

The yardstick: the host mirror ``mr_host_light_shafts`` (held to the NumPy restatement shafts_ref.py in test_shafts_cpu.py)
applied to the float frame F and the z-buffer Z that a TWIN of the scene -- the same recipe, camera, lights and poses, no
``light_shafts`` -- hands out through its taps, run through the mirrors of the passes that stand in front.  The float frame
must match bit for bit, and the frame's bytes must be ``mr_host_accum([F'], [1], scale=1)`` byte for byte."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the capacities of test_accumulate_gpu.py's overflow test
SMALL = (96, 128)
KW = dict(fovy=60, near=0.1, far=20, backface_culling=True)
PAN = [((0.5, 1.0, 2.0), None), ((0.53, 1.0, 1.98), (0.05, 0.0, -0.02)), ((0.56, 1.01, 1.97), (0.09, 0.0, -0.03))]      # (camera position, translation of model 0)
SHIFT = {1: 0, 2: 1, 4: 2}
SKY = (0.9, 0.8, 0.55)                # a colour sky, bright against the scene
FRONT = (-0.5, 0.5, -3.0)             # a light in front of the cameras of PAN and in view, above the cube, where the sky is
BEHIND = (2.0, 3.0, 4.0)              # the recipes' own: behind those cameras


def _shafts(**kw):
    from py_numpy_renderer_amd import LightShafts
    return LightShafts(**dict(dict(intensity=0.75, density=0.9, samples=48, threshold=0.25), **kw))


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


def _pair(api, recipe=scenes.cube_outward, resolution=SMALL, shafts=None, light=FRONT, sky=SKY, **settings):
    """The scene with light shafts and its twin without, both lit from *light* under *sky*; *settings* go to both."""
    scene, twin = recipe(api, resolution=resolution), recipe(api, resolution=resolution)
    for s in (scene, twin):
        s.draw_debug_frustum = False
        s.light = api.Light(light, ambient_strength=0.1, specular_strength=0.1)
        if sky is not None:
            s.skybox = sky
        for name, value in settings.items():
            setattr(s, name, value)
    scene.light_shafts = shafts if shafts is not None else _shafts()
    return scene, twin


def _desc(scene):
    """The description the scene hands to the library for a frame of now."""
    from py_numpy_renderer_amd import _native, _pack
    constants = _pack.light_shafts_constants(scene)
    assert constants is not None, "the light has no place on the screen: the scene is not what the test takes it for"
    return _native.fill_light_shafts_desc(*constants)


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


def _hold(scene, z, before, label):
    """Renders the scene's next frame and holds it to the mirror on *before*, the float frame in front of the pass, and *z*."""
    from py_numpy_renderer_amd import _native
    out = scene.render().copy()
    got = scene._backend().read_frame_f32().copy()
    want, source, march = _native.host_light_shafts(before, z, _desc(scene), fields=True)
    bits, rays = _bits(got, want), _bits(want, before)
    steps = int(np.abs(out.astype(np.int16) - _bytes_of(got, scene.supersample).astype(np.int16)).max())
    sky = ~np.isfinite(z)
    print(f"{label}: {bits} of {want.size} floats differ from the mirror, bytes differ by at most {steps}, the rays changed {rays} floats, "
          f"{int(sky.sum())} of {sky.size} samples are sky, S up to {source.max():.3f}, R up to {march.max():.3f}, F up to {before.max():.3f}, F' up to {got.max():.3f}")
    assert got.shape == before.shape
    assert 0 < sky.sum() < sky.size, f"{label}: the frame is all sky or has none: the pass was shown nothing"
    assert bits == 0, f"{label}: the float frame is not mr_host_light_shafts's"
    assert steps == 0, f"{label}: the bytes are not the finalise of the float frame"
    assert rays > 0, f"{label}: no ray: the pass was shown nothing"
    return out, got


# ---------------------------------------------------------------------------- 1. the frames against the mirror
@pytest.mark.parametrize("settings", [dict(), dict(halvings=1), dict(supersample=2), dict(skybox=True)], ids=["alone", "halvings1", "supersample2", "skybox"])
def test_a_frame_with_shafts_is_the_mirror_on_the_twin_s_taps(api, settings):
    settings = dict(settings)
    halvings = settings.pop("halvings", 2)
    skybox = settings.pop("skybox", False)
    resolution = (48, 64) if settings.get("supersample") else SMALL
    recipe = scenes.cube_skybox if skybox else scenes.cube_outward
    scene, twin = _pair(api, recipe=recipe, resolution=resolution, shafts=_shafts(halvings=halvings, threshold=0.125 if skybox else 0.25),
                        sky=None if skybox else SKY, **settings)
    plain = []
    for k, place in enumerate(PAN[:2]):
        for s in (scene, twin):
            _step(api, s, place)
        z, _, f = _twin_taps(twin)
        out, _ = _hold(scene, z, f, f"{recipe.__name__} {settings}, halvings {halvings}, frame {k}")
        plain.append(twin.render().copy())
        assert not np.array_equal(out, plain[-1]), "the frame is the twin's: no ray reached a byte"
    backend = scene._backend()
    s = scene.supersample
    assert backend.light_shafts_debug() == (2, resolution[0] * s, resolution[1] * s, halvings + SHIFT[s]), "halvings + log2(supersample)"
    times = backend.light_shafts_times()
    assert times["source"] > 0 and times["march"] > 0 and times["composite"] > 0
    assert twin._backend().light_shafts_debug() == (0, 0, 0, 0)
    scene.close(), twin.close()


def test_a_light_behind_the_camera_gives_render_s_bytes_and_skips_the_pass(api):
    scene, twin = _pair(api, light=BEHIND)
    from py_numpy_renderer_amd import _pack
    assert _pack.light_shafts_constants(scene) is None
    out, plain = scene.render().copy(), twin.render().copy()
    assert np.array_equal(out, plain), f"{int((out != plain).sum())} bytes differ from render()"
    assert scene._backend().light_shafts_debug() == (0, 0, 0, 0), "the pass ran without a light on the screen"
    # the same scene with the light moved in front: the pass runs; moved back: it is skipped again
    for s in (scene, twin):
        s.light = api.Light(FRONT, ambient_strength=0.1, specular_strength=0.1)
    z, _, f = _twin_taps(twin)
    _hold(scene, z, f, "the light moved in front")
    assert scene._backend().light_shafts_debug()[0] == 1
    for s in (scene, twin):
        s.light = api.Light(BEHIND, ambient_strength=0.1, specular_strength=0.1)
    assert np.array_equal(scene.render(), twin.render()) and scene._backend().light_shafts_debug()[0] == 1
    scene.close(), twin.close()


def test_no_sky_above_the_threshold_gives_render_s_bytes(api):
    scene, twin = _pair(api, shafts=_shafts(threshold=0.95))
    z, _, f = _twin_taps(twin)
    sky = ~np.isfinite(z)
    assert sky.any() and f[sky].max() <= 0.95, "the sky is not what the test takes it for"
    out, plain = scene.render().copy(), twin.render().copy()
    assert np.array_equal(out, plain), f"{int((out != plain).sum())} bytes differ from render()"
    assert _bits(scene._backend().read_frame_f32(), f) == 0 and scene._backend().light_shafts_debug()[0] == 1, "the pass ran and changed no float"
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 2. the other passes in front, the bloom behind
def test_the_other_passes_stand_in_front_and_the_bloom_behind(api):
    """Every pass on: the frame is the chain of mirrors k_ao, k_taa, k_dof, k_mblur, the shafts, the bloom on the plain twin's
    taps, and the history of temporal_aa is the frame as k_taa left it -- no shafts in it."""
    from py_numpy_renderer_amd import AmbientOcclusion, Bloom, DepthOfField, MotionBlur, TemporalAA, _native, _pack
    scene, twin = _pair(api)
    scene.ambient_occlusion = AmbientOcclusion()
    scene.temporal_aa = TemporalAA(blend=0.25, jitter=4)
    scene.depth_of_field = DepthOfField(lens_radius=0.1)
    scene.motion_blur = MotionBlur(shutter=1.0)
    scene.bloom = Bloom(threshold=0.25, intensity=0.75, levels=3)
    face_off = np.cumsum([0] + [len(m._faces) for m in scene.models])[:-1].astype(np.int32)
    backend = scene._backend()
    still = None
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
        desc = _desc(scene)
        rays = _native.host_light_shafts(blurred, z, desc)
        want = _native.host_bloom(rays, _native.fill_bloom_desc(*_pack.bloom_constants(scene)))
        print(f"frame {k}: {_bits(got, want)} floats of the frame and {_bits(kept, stable)} of the history differ from the mirrors chained; "
              f"the lens changed {_bits(lens, stable)}, the blur {_bits(blurred, lens)}, the rays {_bits(rays, blurred)}, the glow {_bits(want, rays)}")
        assert _bits(got, want) == 0, "the frame is not k_ao, k_taa, k_dof, k_mblur, the shafts, the bloom in that order"
        assert _bits(kept, stable) == 0, "the history is not the frame as k_taa left it: it holds shafts"
        assert np.array_equal(out, _bytes_of(got))
        assert _bits(rays, blurred) > 0 and _bits(want, rays) > 0 and _bits(lens, stable) > 0
        # the shafts in front of the bloom and behind it are different frames: the order is shown
        swapped = _native.host_light_shafts(_native.host_bloom(blurred, _native.fill_bloom_desc(*_pack.bloom_constants(scene))), z, desc)
        assert _bits(swapped, want) > 0, "the bloom in front of the shafts would give the same frame: the test shows nothing"
        # the light stands still under the jitter of temporal_aa: the description's position is the un-jittered grid's
        if still is None:
            still = (desc.light_x, desc.light_y)
        assert jitter is not None and (k == 0 or (desc.light_x, desc.light_y) != still), "the camera moved and the light did not"
        assert backend.light_shafts_debug()[0] == backend.bloom_debug()[0] == backend.ao_debug()[0] == backend.dof_debug()[0] == backend.motion_debug()[0] == backend.taa_debug()[0] == k + 1
    scene.close(), twin.close()


def test_the_overlay_is_drawn_over_the_rays_and_is_no_source(api):
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
    bare, z = tb.read_frame_f32().copy(), tb.read_z().copy()
    lines = (with_lines.view(np.uint32) != bare.view(np.uint32)).any(axis=-1)
    assert 0 < lines.sum() < lines.size // 4, "the plain scene's overlay drew nothing, or everything"
    rays = _native.host_light_shafts(bare, z, _desc(scene))
    assert _bits(got[~lines], rays[~lines]) == 0, "off the lines the frame is not the rays of the frame without them"
    # (the overlay blends a line's edge samples with what lies under them -- here the frame with the rays, in the twin the bare
    # one: only the samples a line covers whole are the line's colour in both)
    solid = lines & (with_lines == np.float32([1.0, 0.0, 0.0])).all(axis=-1)
    assert solid.sum() > 20, "the overlay covers no sample whole"
    assert _bits(got[solid], with_lines[solid]) == 0, "a sample a line covers whole is not the line's colour: the lines are brightened, or lie under the rays"
    assert (rays[solid] != with_lines[solid]).any(), "no ray lies under the lines: the test shows nothing"
    assert _bits(got, _native.host_light_shafts(with_lines, z, _desc(scene))) > 0, "the shafts behind the overlay would give the same frame: the test shows nothing"
    assert np.array_equal(out, _bytes_of(got))
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 3. frames in flight, sums, overflow
def test_two_frames_in_flight_keep_their_own_light_and_levels(api):
    from py_numpy_renderer_amd import _native
    scene, twin = _pair(api)
    shafts = [_shafts(halvings=2, samples=32), _shafts(halvings=1, samples=64, intensity=1.25)]
    places = [(0.5, 1.0, 2.0), (0.9, 1.1, 1.8)]
    want, lights = [], []
    for each, place in zip(shafts, places):
        _look(api, twin, place)
        _look(api, scene, place)
        scene.light_shafts = each
        z, _, f = _twin_taps(twin)
        desc = _desc(scene)
        lights.append((desc.light_x, desc.light_y, desc.halvings))
        want.append(_bytes_of(_native.host_light_shafts(f, z, desc)))
    assert lights[0] != lights[1], "two cameras, two places of the light"
    scene.render()                                       # (the work lists grow outside the pair)
    pending = []
    for each, place in zip(shafts, places):
        _look(api, scene, place)
        scene.light_shafts = each
        pending.append(scene.render_async())
    got = [p.result().copy() for p in pending]
    for k in range(2):
        assert np.array_equal(got[k], want[k]), f"frame {k}: {int((got[k] != want[k]).sum())} bytes differ"
    assert not np.array_equal(got[0], got[1]) and scene._backend().light_shafts_debug()[0] == 3 and scene._backend().light_shafts_debug()[3] == 1
    # render_frames: two views, two in flight, each with the light where its own camera sees it
    scene.light_shafts = shafts[0]
    views = [(api.Camera(p, (0, 0, 0), **KW), api.Camera(p, (0, 0, 0), **KW)) for p in places]
    frames = [f.copy() for f in scene.render_frames(views, depth=2)]
    assert len(frames) == 2 and np.array_equal(frames[0], want[0])
    _look(api, twin, places[1])
    _look(api, scene, places[1])
    z, _, f = _twin_taps(twin)
    assert np.array_equal(frames[1], _bytes_of(_native.host_light_shafts(f, z, _desc(scene)))), "the second view's light is not where its camera sees it"
    scene.close(), twin.close()


def test_render_mean_sums_sub_frames_with_shafts(api):
    from py_numpy_renderer_amd import _native
    scene, twin = _pair(api, resolution=(48, 64))
    places = [(0.5, 1.0, 2.0), (0.53, 1.0, 1.98), (0.56, 1.01, 1.97)]
    subs = []
    for place in places:
        _look(api, twin, place)
        _look(api, scene, place)
        z, _, f = _twin_taps(twin)
        subs.append(_native.host_light_shafts(f, z, _desc(scene)))
    _, want = _native.host_accum(np.stack(subs), [1.0] * 3, shift=0, scale=1.0 / 3.0, want_acc=False)
    got = scene.render_mean(3, lambda k: _look(api, scene, places[k]))
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from the mean of the mirrors' frames"
    assert scene._backend().light_shafts_debug()[0] == 3
    scene.close(), twin.close()


def test_a_frame_rendered_again_after_a_list_overflow_is_the_unstarved_frame(api):
    def frame(squeeze):
        scene = scenes.build(api, "diablo_floor_small")
        scene.draw_debug_frustum = False
        scene.light = api.Light(FRONT, ambient_strength=0.1, specular_strength=0.1)
        scene.light_shafts = _shafts()
        scene.render()
        backend = scene._backend()
        if squeeze:
            backend.set_list_capacities(**SQUEEZED)
        _look(api, scene, (0.56, 1.0, 1.97))
        before = backend.light_shafts_debug()[0]
        out = scene.render().copy()
        got = out, backend.read_frame_f32().copy(), backend.light_shafts_debug()[0] - before
        scene.close()
        return got

    want_rgb, want, once = frame(False)
    got_rgb, got, enqueued = frame(True)
    print(f"the pass enqueued {enqueued} times with the lists squeezed, {once} without")
    assert once == 1 and enqueued >= 2, "the frame did not overflow"
    assert _bits(got, want) == 0 and np.array_equal(got_rgb, want_rgb)


# ---------------------------------------------------------------------------- 4. switching off, refusals
def test_none_restores_the_old_frame_and_a_missing_light_and_split_frames_are_refused(api):
    import ctypes as C
    from py_numpy_renderer_amd import _native
    scene = scenes.cube_outward(api, resolution=(64, 96))
    scene.light = api.Light(FRONT, ambient_strength=0.1, specular_strength=0.1)
    scene.skybox = SKY
    parent = scene.render().copy()
    backend = scene._backend()
    assert backend.light_shafts_debug() == (0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="no frame with light shafts yet"):
        backend.light_shafts_times()
    band_desc, shape = backend._prepare_desc(scene, True, (0, 32), False, False, False, False, None, False, False)
    band_desc = _native.FrameDesc.from_buffer_copy(band_desc)
    scene.light_shafts = _shafts()
    rays = scene.render().copy()
    assert not np.array_equal(rays, parent) and backend.light_shafts_debug() == (1, 64, 96, 2)
    with pytest.raises(ValueError, match="whole frames"):
        scene.render(row_band=(0, 32))
    out = np.zeros(shape, dtype=np.uint8)
    assert backend.lib.mr_render(backend.handle, C.byref(band_desc), out.ctypes.data, None) == _native.MR_E_INVALID
    assert b"light shafts takes whole frames" in backend.lib.mr_last_error() and not out.any()
    # a light index the scene does not have raises where the frame is issued, and the scene renders again once it has it
    scene.light_shafts = _shafts(light=1)
    with pytest.raises(ValueError, match="light 1 does not exist"):
        scene.render()
    scene.add_light(api.Light((-0.2, 0.8, -2.5), color=(0.5, 0.5, 0.5), ambient_strength=0.1, specular_strength=0.1))
    second = scene.render().copy()
    assert backend.light_shafts_debug()[0] == 2 and not np.array_equal(second, rays)
    scene.clear_lights()
    scene.light_shafts = None
    again = scene.render().copy()
    assert np.array_equal(again, parent), f"{int((again != parent).sum())} bytes differ from the frame before the pass"
    assert backend.light_shafts_debug()[0] == 2, "the pass ran with light_shafts = None"
    assert scene.render(row_band=(0, 32)).shape == (32, 96, 3)           # (a band renders again)
    scene.close()
