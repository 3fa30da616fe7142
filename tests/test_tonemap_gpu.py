"""GPU: ``Scene.tone_map`` -- the metered exposure and the tone curve behind a frame's other passes (kernels_tonemap.h,
host_tonemap.h, launch_after_tile in host_frame.h) and the bookkeeping of the Python layer.

The yardstick: the host mirror ``mr_host_tone_map`` (held to the NumPy restatement tonemap_ref.py in test_tonemap_cpu.py)
applied to the float frame F that a TWIN of the scene -- the same recipe, camera, poses and passes, no ``tone_map`` -- hands
out through its tap.  The float frame, the exposure and the histogram must match bit for bit, and the frame's bytes must be
``mr_host_accum([F'], [1], scale=1)`` byte for byte."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the capacities of test_accumulate_gpu.py's overflow test
SMALL = (64, 96)
KW = dict(fovy=60, near=0.1, far=20, backface_culling=True)
PAN = [(0.5, 1.0, 2.0), (0.9, 1.0, 1.8), (1.4, 1.2, 1.4)]
SHIFT = {1: 0, 2: 1, 4: 2}
SKY = (0.9, 0.8, 0.55)
FRONT = (-0.5, 0.5, -3.0)             # a light in front of the cameras of PAN and in view: light shafts have a source


def _tone(**kw):
    from py_numpy_renderer_amd import ToneMap
    return ToneMap(**kw)


def _bits(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def _look(api, scene, position, center=(0, 0, 0)):
    scene.camera, scene.debug_camera = api.Camera(position, center, **KW), api.Camera(position, center, **KW)


def _pair(api, recipe=scenes.cube_outward, resolution=SMALL, tone=None, **settings):
    """The scene with tone mapping and its twin without; *settings* go to both."""
    scene, twin = recipe(api, resolution=resolution), recipe(api, resolution=resolution)
    for s in (scene, twin):
        s.draw_debug_frustum = False
        for name, value in settings.items():
            setattr(s, name, value)
    scene.tone_map = tone if tone is not None else _tone()
    return scene, twin


def _desc(scene):
    from py_numpy_renderer_amd import _native, _pack
    return _native.fill_tone_map_desc(*_pack.tone_map_constants(scene))


def _tap(twin):
    """The twin's float frame as it is now, in front of the pass the twin does not have."""
    backend = twin._backend()
    backend.render(twin, keep_float=True, counters=False, keep_buffers=True, overlay=False)
    return backend.read_frame_f32().copy()


def _bytes_of(frame, supersample=1):
    from py_numpy_renderer_amd import _native
    return _native.host_accum(frame[None], [1.0], shift=SHIFT[supersample], scale=1.0, want_acc=False)[1]


def _hold(scene, before, label, e_prev=None):
    """Renders the scene's next frame and holds it, its exposure and its histogram to the mirror on *before*."""
    from py_numpy_renderer_amd import _native
    out = scene.render().copy()
    backend = scene._backend()
    got = backend.read_frame_f32().copy()
    want, hist, e = _native.host_tone_map(before, _desc(scene), e_prev)
    got_e = backend.read_exposure()
    steps = int(np.abs(out.astype(np.int16) - _bytes_of(got, scene.supersample).astype(np.int16)).max())
    print(f"{label}: {_bits(got, want)} of {want.size} floats differ from the mirror, e = {got_e!r} (mirror {e!r}), bytes differ by at most {steps}, "
          f"F up to {before.max():.3f}, F' up to {got.max():.3f}")
    assert got.shape == before.shape
    assert _bits(got, want) == 0, f"{label}: the float frame is not mr_host_tone_map's"
    assert _bits(np.float32([got_e]), np.float32([e])) == 0, f"{label}: the exposure is not the mirror's"
    if scene.tone_map.exposure is None:
        assert (backend.read_luminance_histogram() == hist).all() and hist.sum() > 0, f"{label}: the histogram is not the mirror's"
    else:
        with pytest.raises(ValueError, match="nothing was metered"):
            backend.read_luminance_histogram()
    assert steps == 0, f"{label}: the bytes are not the finalise of the float frame"
    assert _bits(want, before) > 0, f"{label}: no float changed: the pass was shown nothing"
    return out, got, got_e


# ---------------------------------------------------------------------------- 1. the frames against the mirror
@pytest.mark.parametrize("settings", [dict(), dict(supersample=2, operator="reinhard"), dict(exposure=1.7, operator="linear"),
                                      dict(low=0.5, high=0.95, key=0.3)], ids=["aces", "supersample2_reinhard", "fixed_linear", "trimmed"])
def test_a_tone_mapped_frame_is_the_mirror_on_the_twin_s_tap(api, settings):
    settings = dict(settings)
    s = settings.pop("supersample", 1)
    scene, twin = _pair(api, tone=_tone(**settings), supersample=s)
    for k, place in enumerate(PAN[:2]):
        for sc in (scene, twin):
            _look(api, sc, place)
        _hold(scene, _tap(twin), f"cube_outward {settings}, supersample {s}, frame {k}")
    backend = scene._backend()
    fixed = scene.tone_map.exposure is not None
    rows, cols = SMALL[0] * s, SMALL[1] * s
    grid = min(256, -(-(rows * cols // 4) // 256))
    assert backend.tone_map_debug() == (2, rows, cols, 0 if fixed else grid, 0, 0), "two frames, nothing handed over: not adaptive"
    times = backend.tone_map_times()
    assert times["tone_apply"] > 0 and (fixed or (times["lum_hist"] > 0 and times["exposure"] > 0))
    assert twin._backend().tone_map_debug() == (0, 0, 0, 0, 0, 0)
    scene.close(), twin.close()


def test_linear_at_exposure_one_is_render_s_frame(api):
    scene, twin = _pair(api, tone=_tone(operator="linear", exposure=1.0))
    for frustum in (False, True):
        for sc in (scene, twin):
            sc.draw_debug_frustum = frustum
        out, plain = scene.render().copy(), twin.render().copy()
        assert np.array_equal(out, plain), f"frustum {frustum}: {int((out != plain).sum())} bytes differ from render()"
    assert scene._backend().tone_map_debug()[0] == 2, "the pass ran"
    assert scene._backend().read_exposure() == 1.0
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 2. the other passes in front
def test_bloom_and_light_shafts_in_front_no_longer_burn_out(api):
    from py_numpy_renderer_amd import Bloom, LightShafts
    scene, twin = _pair(api)
    for sc in (scene, twin):
        sc.light = api.Light(FRONT, ambient_strength=0.1, specular_strength=0.1)
        sc.skybox = SKY
        sc.light_shafts = LightShafts(intensity=1.5, density=0.9, samples=48, threshold=0.25)
        sc.bloom = Bloom(threshold=0.25, intensity=2.0, levels=3)
        _look(api, sc, PAN[0])
    before = _tap(twin)
    plain = twin.render().copy()
    out, got, e = _hold(scene, before, "bloom and light shafts in front")
    burnt, kept = int((before >= 1.0).all(axis=-1).sum()), int((got >= 1.0).all(axis=-1).sum())
    print(f"samples at or above 1 in every channel: {burnt} without the pass, {kept} with it; bytes at 255: {int((plain == 255).sum())} and {int((out == 255).sum())}")
    assert before.max() > 1.25 and burnt > 50, "the frame does not burn out without the pass: the test shows nothing"
    assert kept < burnt // 4 and got.max() <= 1.0 and (out == 255).sum() < (plain == 255).sum()
    backend = scene._backend()
    assert backend.bloom_debug()[0] == backend.light_shafts_debug()[0] == backend.tone_map_debug()[0] == 1
    scene.close(), twin.close()


def test_the_overlay_keeps_its_colours(api):
    from py_numpy_renderer_amd import _native
    scene, twin = _pair(api, tone=_tone(operator="reinhard", key=0.4))
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
    bare = _tap(twin)
    lines = (with_lines.view(np.uint32) != bare.view(np.uint32)).any(axis=-1)
    assert 0 < lines.sum() < lines.size // 4, "the plain scene's overlay drew nothing, or everything"
    mapped = _native.host_tone_map(bare, _desc(scene))[0]
    assert _bits(got[~lines], mapped[~lines]) == 0, "off the lines the frame is not the tone-mapped frame without them"
    solid = lines & (with_lines == np.float32([1.0, 0.0, 0.0])).all(axis=-1)
    assert solid.sum() > 20, "the overlay covers no sample whole"
    assert _bits(got[solid], with_lines[solid]) == 0, "a sample a line covers whole is not the line's colour: the lines were tone-mapped"
    assert _bits(got, _native.host_tone_map(with_lines, _desc(scene))[0]) > 0, "the pass behind the overlay would give the same frame: the test shows nothing"
    assert np.array_equal(out, _bytes_of(got))
    scene.close(), twin.close()


def test_the_history_of_temporal_aa_holds_no_tone_mapped_colours(api):
    from py_numpy_renderer_amd import TemporalAA
    scene, twin = _pair(api, temporal_aa=TemporalAA(blend=0.25, jitter=4))
    for k, place in enumerate(PAN):
        for sc in (scene, twin):
            _look(api, sc, place)
        _hold(scene, _tap(twin), f"temporal_aa in front, frame {k}")
        kept, plain = scene._backend().read_history(), twin._backend().read_history()
        assert _bits(kept, plain) == 0, f"frame {k}: the history is not the twin's: it holds tone-mapped colours"
    assert scene._backend().taa_debug()[4] == 3
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 3. adaptation: the scene's previous exposure
def test_an_adaptive_sequence_is_the_mirror_chained_by_hand(api):
    from py_numpy_renderer_amd import _native
    scene, twin = _pair(api, tone=_tone(speed=0.25, key=0.4))
    lights = [dict(color=(1.0, 1.0, 1.0)), dict(color=(0.3, 0.3, 0.3)), dict(color=(0.6, 0.6, 0.6))]
    e_prev, seen = None, []
    for k, (place, light) in enumerate(zip(PAN, lights)):
        for sc in (scene, twin):
            _look(api, sc, place)
            sc.light = api.Light((2, 3, 4), ambient_strength=0.1, specular_strength=0.3, **light)
        before = _tap(twin)
        alone = _native.host_tone_map(before, _desc(scene))[2]
        e_prev = _hold(scene, before, f"adaptive frame {k}", e_prev)[2]
        seen.append((float(e_prev), float(alone)))
        assert scene._backend().tone_map_debug()[4:] == (k + 1, 1), "the frame's exposure was handed over"
    print(f"(e, e_t) frame by frame: {seen}")
    assert seen[0][0] == seen[0][1] and all(e != e_t for e, e_t in seen[1:]), "from the second frame on the exposure lags its target"
    # reset_motion() forgets it: the next frame meters alone
    scene.reset_motion()
    _hold(scene, _tap(twin), "after reset_motion()", None)
    assert scene._backend().tone_map_debug()[4:] == (4, 1)
    # ... and so does a new description, and None
    scene.tone_map = _tone(speed=0.5, key=0.4)
    _hold(scene, _tap(twin), "after a new description", None)
    scene.tone_map = None
    scene.render()
    assert scene._backend().tone_map_debug()[5] == 0
    scene.close(), twin.close()


def test_a_frame_rendered_again_after_a_list_overflow_reads_the_same_previous_exposure(api):
    from py_numpy_renderer_amd import _native

    def frames(squeeze):
        scene = scenes.build(api, "diablo_floor_small")
        scene.draw_debug_frustum = False
        scene.tone_map = _tone(speed=0.25)
        scene.render()
        backend = scene._backend()
        first = backend.read_exposure()
        if squeeze:
            backend.set_list_capacities(**SQUEEZED)
        _look(api, scene, (0.56, 1.0, 1.97))
        scene.light = api.Light((2, 3, 4), color=(0.4, 0.4, 0.4), ambient_strength=0.1, specular_strength=0.1)
        before = backend.tone_map_debug()
        out = scene.render().copy()
        after = backend.tone_map_debug()
        got = out, backend.read_frame_f32().copy(), first, backend.read_exposure(), after[0] - before[0], after[4] - before[4]
        scene.close()
        return got

    want_rgb, want, first, want_e, once, adopted = frames(False)
    got_rgb, got, got_first, got_e, enqueued, got_adopted = frames(True)
    print(f"the pass enqueued {enqueued} times with the lists squeezed, {once} without; e {first!r} then {got_e!r}")
    assert once == 1 and enqueued >= 2, "the frame did not overflow"
    assert adopted == got_adopted == 1, "one exposure handed over, whatever the attempts"
    assert got_first == first and got_e == want_e and got_e != first, "the second attempt read another previous exposure"
    assert _bits(got, want) == 0 and np.array_equal(got_rgb, want_rgb)


# ---------------------------------------------------------------------------- 4. frames in flight, sums
def test_frames_in_flight_and_render_mean_meter_every_frame_alone(api):
    from py_numpy_renderer_amd import _native
    scene, twin = _pair(api)
    want = []
    for place in PAN[:2]:
        _look(api, twin, place)
        want.append(_native.host_tone_map(_tap(twin), _desc(scene))[0])
    scene.render()                                       # (the work lists grow outside the pair)
    pending = []
    for place in PAN[:2]:
        _look(api, scene, place)
        pending.append(scene.render_async())
    got = [p.result().copy() for p in pending]
    for k in range(2):
        assert np.array_equal(got[k], _bytes_of(want[k])), f"frame {k}: {int((got[k] != _bytes_of(want[k])).sum())} bytes differ"
    assert not np.array_equal(got[0], got[1])
    views = [(api.Camera(p, (0, 0, 0), **KW), api.Camera(p, (0, 0, 0), **KW)) for p in PAN[:2]]
    frames = [f.copy() for f in scene.render_frames(views, depth=2)]
    assert np.array_equal(frames[0], got[0]) and np.array_equal(frames[1], got[1])
    # render_mean: sub-frames are tone-mapped before they are summed
    _, mean = _native.host_accum(np.stack(want), [1.0] * 2, shift=0, scale=0.5, want_acc=False)
    before = scene._backend().tone_map_debug()[0]
    summed = scene.render_mean(2, lambda k: _look(api, scene, PAN[k]))
    assert np.array_equal(summed, mean), f"{int((summed != mean).sum())} bytes differ from the mean of the mirrors' frames"
    assert scene._backend().tone_map_debug()[0] == before + 2 and scene._backend().tone_map_debug()[4:] == (0, 0)
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 5. switching off, refusals
def test_none_restores_the_old_frame_and_the_refusals(api):
    import ctypes as C
    from py_numpy_renderer_amd import _native
    scene = scenes.cube_outward(api, resolution=SMALL)
    parent = scene.render().copy()
    backend = scene._backend()
    assert backend.tone_map_debug() == (0, 0, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="no frame with tone mapping yet"):
        backend.tone_map_times()
    with pytest.raises(ValueError, match="without tone mapping"):
        backend.read_exposure()
    band_desc, shape = backend._prepare_desc(scene, True, (0, 32), False, False, False, False, None, False, False)
    band_desc = _native.FrameDesc.from_buffer_copy(band_desc)
    scene.tone_map = _tone()
    mapped = scene.render().copy()
    assert not np.array_equal(mapped, parent) and backend.tone_map_debug()[:3] == (1, *SMALL)
    # split frames
    with pytest.raises(ValueError, match="whole frames"):
        scene.render(row_band=(0, 32))
    out = np.zeros(shape, dtype=np.uint8)
    assert backend.lib.mr_render(backend.handle, C.byref(band_desc), out.ctypes.data, None) == _native.MR_E_INVALID
    assert b"tone mapping takes whole frames" in backend.lib.mr_last_error() and not out.any()
    # adaptive: one frame at a time, no accumulation, no caller's stream
    scene.tone_map = _tone(speed=0.5)
    first = scene.render_async()
    with pytest.raises(ValueError, match="one frame of the scene at a time"):
        scene.render_async()
    with pytest.raises(ValueError, match="one frame of the scene at a time"):
        scene.render()
    first.result()
    with pytest.raises(ValueError, match="accumulate"):
        scene.accumulate()
    with pytest.raises(ValueError, match="render\\(\\) / render_async\\(\\)"):
        backend.render_device(scene, 0)
    full_desc, full_shape = backend._prepare_desc(scene, True, None, True, False, False, False, None, False, False)
    assert backend.lib.mr_accum_begin(backend.handle) == 0
    assert backend.lib.mr_accum_add(backend.handle, C.byref(full_desc), C.c_double(1.0)) == _native.MR_E_INVALID
    assert b"adaptive tone mapping" in backend.lib.mr_last_error()
    assert backend.lib.mr_render_device(backend.handle, C.byref(full_desc), C.c_void_p(out.ctypes.data), None) == _native.MR_E_INVALID      # (refused before the pointer is looked at)
    assert b"adaptive tone mapping" in backend.lib.mr_last_error()
    # the library's own one-frame rule: a second frame of the adaptive scene while the first has not been waited for
    out_a, out_b = backend._pinned.array(full_shape), backend._pinned.array(full_shape)
    assert backend.lib.mr_render_async(backend.handle, C.byref(full_desc), out_a.ctypes.data, 0) == 0
    assert backend.lib.mr_render_async(backend.handle, C.byref(full_desc), out_b.ctypes.data, 1) == _native.MR_E_INVALID
    assert b"has not been waited for" in backend.lib.mr_last_error()
    assert backend.lib.mr_render_wait(backend.handle, 0, None) == 0
    # off again
    scene.tone_map = None
    again = scene.render().copy()
    assert np.array_equal(again, parent), f"{int((again != parent).sum())} bytes differ from the frame before the pass"
    frames = backend.tone_map_debug()[0]
    scene.render()
    assert backend.tone_map_debug()[0] == frames, "the pass ran with tone_map = None"
    assert scene.render(row_band=(0, 32)).shape == (32, SMALL[1], 3)           # (a band renders again)
    scene.close()
