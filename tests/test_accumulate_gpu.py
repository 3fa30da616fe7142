"""GPU: ``Scene.accumulate`` -- sub-frames summed with weights on the device and finalised once (host_accum.h;
k_accum_add and k_accum_resolve in kernels_accum.h).

The yardstick is the host mirror ``mr_host_accum`` (held to the NumPy restatement in test_accumulate_cpu.py) applied to
the float frames F_k the same scene hands out through the ``keep_float`` tap right before each ``add()``: the sum must
match it bit for bit and the finalised frame byte for byte.  Beside it: identities with ``Scene.render()``, and the
oracle's frames through accumulate_ref.py at the project's standing bar for the uint8 frame (+-1)."""
import numpy as np
import pytest

import accumulate_ref as ref
import scenes
from multilight_ref import extra_lights

pytestmark = pytest.mark.gpu

LIGHTS = [(2.0, 3.0, 4.0), (2.6, 3.0, 3.1), (1.2, 3.4, 4.4), (2.2, 2.2, 4.8)]
SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the smallest lists the overflow tests set


def _move_light(scene, k):
    scene.light.position = np.array(LIGHTS[k % len(LIGHTS)])


def _tap(scene, shadows=True):
    """F_k: the float frame the scene gives as it is now (after the overlay, where it draws one)."""
    backend = scene._backend()
    backend.render(scene, shadows=shadows, keep_float=True, counters=False, keep_buffers=False, overlay=scene.draw_debug_frustum)
    return backend.read_frame_f32().copy()


def _run(scene, weights, step=_move_light):
    """An accumulation over ``step(scene, k)``; returns (the F_k, the sum, the finalised frame, mr_debug_accum)."""
    frames = []
    with scene.accumulate() as acc:
        for k, w in enumerate(weights):
            step(scene, k)
            frames.append(_tap(scene))
            acc.add(w)
        assert acc.count == len(weights) and acc.weight_sum == sum(weights)
        return frames, acc.float_frame(), acc.result().copy(), scene._backend().accum_debug()


def _hold_to_the_mirror(frames, weights, s, got_acc, got_rgb, label):
    from py_numpy_renderer_amd import _native
    want_acc, want_rgb = _native.host_accum(frames, weights, shift={1: 0, 2: 1, 4: 2}[s], scale=float(ref.default_scale(weights)))
    assert got_acc.shape == want_acc.shape and got_acc.dtype == np.float32, label
    assert got_rgb.shape == want_rgb.shape and got_rgb.dtype == np.uint8, label
    bits = int((got_acc.view(np.uint32) != want_acc.view(np.uint32)).sum())
    steps = int(np.abs(got_rgb.astype(np.int16) - want_rgb.astype(np.int16)).max())
    print(f"{label}: {bits} floats of the sum differ, bytes differ by at most {steps}")
    assert bits == 0, f"{label}: the sum is not the pinned one"
    assert steps == 0, f"{label}: the finalised frame is not the mirror's"
    assert 0.0 <= float(got_acc.min()) and float(np.max(frames)) <= 1.0, f"{label}: a colour outside [0, 1]"


# ---------------------------------------------------------------------------- 1. the buffer is the pinned sum
def test_the_buffer_is_the_pinned_sum(api):
    scene = scenes.cube_small(api)
    weights = (0.5, 0.3, 0.2)
    frames, acc, rgb, debug = _run(scene, weights)
    _hold_to_the_mirror(frames, weights, 1, acc, rgb, "cube_small, three lights")
    assert debug == (3, 0, 120, 160)
    times = scene._backend().accum_times()
    assert times["accum_add"] > 0 and times["accum_resolve"] > 0
    scene.close()


# ---------------------------------------------------------------------------- 2. sizes at which the add kernel can go wrong
@pytest.mark.parametrize("resolution", [(16, 16), (37, 41), (120, 160)])
def test_sizes(api, resolution):
    """(16, 16): one tile, 192 float4s, fewer than a block's lanes.  (37, 41): 4551 floats, so three take the scalar tail,
    and partial tiles.  (120, 160): 56 blocks."""
    scene = scenes.cube_outward(api, resolution=resolution)
    weights = (0.7, 0.3)
    frames, acc, rgb, debug = _run(scene, weights)
    assert not np.array_equal(frames[0], frames[1]), "the light did not move"
    _hold_to_the_mirror(frames, weights, 1, acc, rgb, f"cube_outward at {resolution}")
    assert debug == (2, 0) + resolution and rgb.shape == resolution + (3,)
    scene.close()


# ---------------------------------------------------------------------------- 3. supersampled
@pytest.mark.parametrize("s", [2, 4])
def test_supersampled(api, s):
    scene = scenes.diablo_small(api, resolution=(30, 40))
    scene.supersample = s
    weights = (0.5, 0.3, 0.2)
    frames, acc, rgb, debug = _run(scene, weights)
    assert acc.shape == (30 * s, 40 * s, 3) and rgb.shape == (30, 40, 3) and debug == (3, 0, 30 * s, 40 * s)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2]), "the light did not move"
    _hold_to_the_mirror(frames, weights, s, acc, rgb, f"diablo_small, supersample {s}")
    scene.close()


# ---------------------------------------------------------------------------- 4. identities, byte for byte
def _plain(api):
    return scenes.cube_small(api)


def _supersampled(api):
    scene = scenes.diablo_small(api, resolution=(60, 80))
    scene.supersample = 2
    return scene


def _overlaid(api):
    scene = scenes.cube_outward(api)
    scene.draw_debug_frustum = True
    return scene


def _two_lights(api):
    scene = scenes.torus_spot(api)
    scene.add_light(extra_lights(api)[0])
    return scene


def _skybox(api):
    return scenes.cube_skybox(api)


@pytest.mark.parametrize("build", [_plain, _supersampled, _overlaid, _two_lights, _skybox])
def test_one_sub_frame_is_the_frame(api, build):
    """One ``add(1.0)`` and ``result(scale=1)`` is ``render()`` of the same state; and so are three adds of the
    unchanged scene with weights 0.25, 0.25, 0.5 (exact in float32)."""
    scene = build(api)
    want = scene.render().copy()
    with scene.accumulate() as acc:
        acc.add(1.0)
        assert np.array_equal(acc.result(scale=1), want), f"{build.__name__}: one sub-frame"
    with scene.accumulate() as acc:
        for w in (0.25, 0.25, 0.5):
            acc.add(w)
        assert acc.weight_sum == 1.0
        assert np.array_equal(acc.result(scale=1), want), f"{build.__name__}: three parts of one frame"
        assert np.array_equal(acc.result(), want), f"{build.__name__}: the default scale of weights that sum to 1"
    assert np.array_equal(scene.render(), want)
    scene.close()


# ---------------------------------------------------------------------------- 5. against the oracle
def test_four_lights_against_the_oracle(api, oracle_mod):
    """A point light averaged over four positions.  +-1 per channel is the bar BASELINE.json sets for the uint8 frame;
    a convex combination does not widen the 2e-6 float bar beneath it."""
    scene = scenes.torus_spot(api)
    frames = []
    with scene.accumulate() as acc:
        for k in range(4):
            _move_light(scene, k)
            frames.append(oracle_mod.render(scene, shadows=True).frame.copy())
            acc.add(1.0)
        got, tap = acc.result().copy(), acc.float_frame()
    want_acc, want = ref.result(frames, (1.0,) * 4)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print(f"torus_spot, four lights: bytes differ by at most {diff.max()} ({int((diff > 0).any(axis=-1).sum())} pixels), "
          f"the sum by at most {np.abs(tap.astype(np.float64) - want_acc.astype(np.float64)).max():.3g}")
    assert diff.max() <= 1
    scene.close()


# ---------------------------------------------------------------------------- 6. moving models
def _pose(k):
    a = 0.05 * k
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    m[3, 1] = 0.02 * k
    return m


def test_a_pose_pass_between_sub_frames(api):
    scene = scenes.diablo_small(api, resolution=(120, 160))
    weights = (0.4, 0.3, 0.2, 0.1)

    def step(scene, k):
        scene.models[0].pose = _pose(k + 1)

    frames, acc, rgb, debug = _run(scene, weights, step)
    assert all(not np.array_equal(frames[k], frames[k + 1]) for k in range(3)), "the model did not move"
    assert scene._backend().pose_counters()[1] >= 4, "no pose pass ran between the sub-frames"
    _hold_to_the_mirror(frames, weights, 1, acc, rgb, "diablo_small, four poses")
    assert debug == (4, 0, 120, 160)
    scene.close()


# ---------------------------------------------------------------------------- 7. overflow
def test_a_sub_frame_that_overflows_is_rendered_again(api):
    free = scenes.build(api, "diablo_floor_small")
    with free.accumulate() as acc:
        for k in range(2):
            _move_light(free, k)
            acc.add(0.5)
        want_acc, want_rgb = acc.float_frame(), acc.result().copy()
    unstarved = free._backend().accum_debug()          # (the lists a scene starts with may be too short for it as well)
    assert unstarved[0] == 2
    free.close()

    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    backend.sync_scene(scene)                              # (an upload resets the capacities)
    backend.set_list_capacities(**SQUEEZED)
    with scene.accumulate() as acc:
        for k in range(2):
            _move_light(scene, k)
            acc.add(0.5)
        debug = backend.accum_debug()
        assert np.array_equal(acc.float_frame().view(np.uint32), want_acc.view(np.uint32))
        assert np.array_equal(acc.result(), want_rgb)
    print(f"sub-frames rendered again: {debug[1]} with the lists squeezed, {unstarved[1]} without")
    assert debug[0] == 2 and debug[1] >= 1, debug
    scene.close()


# ---------------------------------------------------------------------------- 8. progressive
def test_progressive_refinement_and_frames_in_between(api):
    scene = scenes.cube_outward(api)
    with scene.accumulate() as acc:
        for k in range(4):
            _move_light(scene, k)
            acc.add(1.0)
        want_four = acc.result().copy()
    with scene.accumulate() as acc:
        for k in range(2):
            _move_light(scene, k)
            acc.add(1.0)
        want_two = acc.result().copy()

    with scene.accumulate() as acc:
        for k in range(2):
            _move_light(scene, k)
            acc.add(1.0)
        first = acc.result().copy()
        assert np.array_equal(acc.result(), first), "a second result() of the same sum differs"
        held = acc.float_frame()
        _move_light(scene, 3)
        plain = scene.render().copy()                      # the library's stream, the slot the sub-frames use
        pending = scene.render_async()
        assert np.array_equal(pending.result(), plain)
        assert np.array_equal(acc.float_frame().view(np.uint32), held.view(np.uint32)), "a frame in between disturbed the sum"
        for k in range(2, 4):
            _move_light(scene, k)
            acc.add(1.0)
        second = acc.result().copy()
        assert acc.count == 4 and acc.weight_sum == 4.0
    assert np.array_equal(first, want_two)
    assert np.array_equal(second, want_four)
    assert not np.array_equal(first, second)
    scene.close()


# ---------------------------------------------------------------------------- 9. refusals on the device path
def test_refusals(api):
    scene = scenes.cube_small(api, resolution=(32, 48))
    backend = scene._backend()
    acc = scene.accumulate()
    with pytest.raises(RuntimeError, match="open accumulation"):
        scene.accumulate()
    acc.add(1.0)
    assert backend.accum_debug() == (1, 0, 32, 48)
    scene.resolution = (48, 64)
    with pytest.raises(ValueError, match="share one resolution"):
        acc.add(1.0)
    scene.resolution = (32, 48)
    scene.supersample = 2
    with pytest.raises(ValueError, match="share one resolution"):
        acc.add(1.0)
    scene.supersample = 1
    assert acc.count == 1 and backend.accum_debug() == (1, 0, 32, 48)
    acc.add(2.0)
    assert acc.count == 2 and acc.weight_sum == 3.0 and backend.accum_debug() == (2, 0, 32, 48)
    assert acc.result().shape == (32, 48, 3)
    acc.close()
    with pytest.raises(RuntimeError, match="closed"):
        acc.result()
    with scene.accumulate() as other:                      # a new accumulation starts empty, at another size
        scene.supersample = 2
        other.add(1.0)
        assert backend.accum_debug() == (1, 0, 64, 96) and other.float_frame().shape == (64, 96, 3)
    scene.close()


# ---------------------------------------------------------------------------- 10. render_mean
def test_render_mean_is_the_explicit_loop(api):
    scene = scenes.cube_outward(api)
    with scene.accumulate() as acc:
        for k in range(3):
            _move_light(scene, k)
            acc.add(1.0)
        want = acc.result().copy()
    calls = []
    got = scene.render_mean(3, lambda k: (calls.append(k), _move_light(scene, k)))
    assert calls == [0, 1, 2]
    assert np.array_equal(got, want)
    assert scene.__dict__.get("_accumulation") is None
    scene.close()
