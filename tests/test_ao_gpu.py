"""GPU: ``Scene.ambient_occlusion`` -- screen-space obscurance from the z-buffer, applied to the float frame on the device
(k_ao in kernels_ao.h, host_ao.h, launch_after_tile in host_frame.h).

The yardstick is the host mirror ``mr_host_ao`` (held to the NumPy restatement ao_ref.py in test_ao_cpu.py) applied to
the z-buffer Z and the float frame F the same scene hands out through its taps WITHOUT obscurance: the float frame F' of
the scene with obscurance must match it bit for bit, and the frame's bytes must be ``mr_host_accum([F'], [1], scale=1)``
byte for byte.  Beside it: identities with ``render()``, the overlay, frames in flight, the accumulation, overflow."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ao_ref
import scenes
from multilight_ref import extra_lights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the capacities of test_accumulate_gpu.py's overflow test
NO_PAIR = 1e30                                                      # a bias no pair passes: t < 0 everywhere, ao == 1


def _ao(**kw):
    from py_numpy_renderer_amd import AmbientOcclusion
    return AmbientOcclusion(**kw)


def _desc(scene):
    from py_numpy_renderer_amd import _native, _pack
    return _native.fill_ao_desc(scene.ambient_occlusion, *_pack.ao_constants(scene))


def _plain_taps(scene, overlay=False):
    """(Z, F) of the scene as it is now, rendered without obscurance: the taps after the overlay where one is drawn."""
    held, scene.ambient_occlusion = scene.ambient_occlusion, None
    backend = scene._backend()
    try:
        backend.render(scene, keep_float=True, counters=False, keep_buffers=True, overlay=overlay)
        return backend.read_z().copy(), backend.read_frame_f32().copy()
    finally:
        scene.ambient_occlusion = held


def _ao_frame(scene):
    """(bytes, F', Z) of ``render()`` with the scene's obscurance: the library keeps the taps by itself."""
    out = scene.render().copy()
    backend = scene._backend()
    return out, backend.read_frame_f32().copy(), backend.read_z().copy()


def _bits(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def _hold(scene, label, want_share=None):
    """The yardstick on the scene as it is (no overlay); returns (Z, F, F')."""
    from py_numpy_renderer_amd import _native
    assert not scene.draw_debug_frustum
    z, f = _plain_taps(scene)
    out, got, z_after = _ao_frame(scene)
    want = _native.host_ao(z, f, _desc(scene))
    s = scene.supersample
    _, want_rgb = _native.host_accum(got[None], [1.0], shift={1: 0, 2: 1, 4: 2}[s], scale=1.0, want_acc=False)
    covered = np.isfinite(z)
    darkened = (got < f).any(axis=-1)
    share = float(darkened[covered].mean()) if covered.any() else 0.0
    bits, steps = _bits(got, want), int(np.abs(out.astype(np.int16) - want_rgb.astype(np.int16)).max())
    print(f"{label}: {bits} floats differ from the mirror, bytes differ by at most {steps}, "
          f"{share:.1%} of {int(covered.sum())} covered samples darkened")
    assert got.shape == f.shape and out.shape == want_rgb.shape
    assert bits == 0, f"{label}: the float frame is not the mirror's"
    assert steps == 0, f"{label}: the bytes are not the finalise of the float frame"
    assert np.array_equal(z_after.view(np.uint64), z.view(np.uint64)), f"{label}: the z-buffer changed"
    assert _bits(got[~covered], f[~covered]) == 0, f"{label}: a background sample changed"
    if want_share is not None:
        assert share >= want_share, f"{label}: only {share:.1%} of the covered samples darkened"
    return z, f, got


# ---------------------------------------------------------------------------- 1. shapes at which the kernel can go wrong
@pytest.mark.parametrize("resolution, radius", [((16, 16), 2.0), ((16, 16), 16.0), ((37, 41), 2.0), ((37, 41), 0.1)])
def test_small_frames(api, resolution, radius):
    """(16, 16): one workgroup whose halo is larger than the frame.  With radius 2 (k = 27.7) the footprint stays under
    the clamp, at about half the frame, so every pair of the outer ring leaves the frame somewhere; with radius 16 it is
    clamped to 32 at every sample and no outer pair stays inside.  (37, 41): partial workgroups in both directions and
    rows of 123 bytes, which start at every alignment the in-place accesses know."""
    scene = scenes.cube_outward(api, resolution=resolution)
    scene.ambient_occlusion = _ao(radius=radius)
    z, f, got = _hold(scene, f"cube_outward at {resolution}, radius {radius}")
    if radius == 16.0:
        from py_numpy_renderer_amd import _pack
        m, k, _ = _pack.ao_constants(scene)
        e = ao_ref.eye_depth(z, m)
        assert (np.float32(k) / e[np.isfinite(e)]).min() >= 32, "the footprint is not clamped everywhere"
    assert scene._backend().ao_debug()[1:] == resolution
    assert scene._backend().ao_time() > 0
    scene.close()


_CHILD = r"""
import hashlib, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import scenes
from py_numpy_renderer_amd import AmbientOcclusion
api = scenes.product_api()
scene = scenes.cube_outward(api, resolution=(37, 41))
scene.ambient_occlusion = AmbientOcclusion(radius=2.0)
scene.render()
print("digest", hashlib.sha256(np.ascontiguousarray(scene._backend().read_frame_f32()).tobytes()).hexdigest())
scene.close()
"""


@pytest.fixture(scope="module")
def small_digest(api):
    scene = scenes.cube_outward(api, resolution=(37, 41))
    scene.ambient_occlusion = _ao(radius=2.0)
    z, f, got = _hold(scene, "cube_outward at (37, 41), radius 2.0, the default shape")
    assert _bits(got, f) > 0
    scene.close()
    return hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()


@pytest.mark.parametrize("shape", ["32x32", "64x16"])
def test_every_workgroup_shape_gives_the_same_bits(small_digest, shape):
    """MR_AO_TILE is read once per process: a fresh child renders with each of the other shapes (ao_shape's parsing;
    test_post_fields_gpu.py reaches the shapes without it)."""
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MR_AO_TILE=shape), timeout=300, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    lines = [ln.split()[1] for ln in proc.stdout.splitlines() if ln.startswith("digest ")]
    assert lines == [small_digest], f"MR_AO_TILE={shape}: the float frame is not the default shape's"


def test_diablo_small_with_the_defaults(api):
    scene = scenes.diablo_small(api)
    scene.ambient_occlusion = _ao()
    _hold(scene, "diablo_small (240, 320), defaults", want_share=0.20)
    scene.close()


@pytest.mark.parametrize("s", [2, 4])
def test_supersampled(api, s):
    """k scales with the sample grid's height, and the footprint's clamp is in samples."""
    scene = scenes.diablo_small(api, resolution=(30, 40))
    scene.supersample = s
    scene.ambient_occlusion = _ao()
    z, f, got = _hold(scene, f"diablo_small (30, 40), supersample {s}")
    assert got.shape == (30 * s, 40 * s, 3) and _bits(got, f) > 0
    scene.close()


def test_orthographic(api):
    """A constant footprint, and a background whose z is -inf."""
    scene = scenes.tetra_ortho(api)
    scene.ambient_occlusion = _ao()
    z, f, got = _hold(scene, "tetra_ortho")
    assert (z[~np.isfinite(z)] < 0).all() and _bits(got, f) > 0
    scene.close()


def test_left_handed_opengl_with_extreme_planes(api):
    scene = scenes.diablo_floor_lh_gl(api, resolution=(135, 240))
    scene.ambient_occlusion = _ao()
    z, f, got = _hold(scene, "diablo_floor_lh_gl (135, 240)")
    assert _bits(got, f) > 0
    scene.close()


def test_skybox_samples_keep_the_sky(api):
    scene = scenes.cube_skybox(api)
    scene.ambient_occlusion = _ao(radius=0.3)
    z, f, got = _hold(scene, "cube_skybox")
    sky = ~np.isfinite(z)
    assert sky.any() and len(np.unique(f[sky], axis=0)) > 16, "no sky in the frame"
    assert _bits(got[sky], f[sky]) == 0 and _bits(got, f) > 0
    scene.close()


def test_two_lights_are_darkened_once(api):
    scene = scenes.torus_spot(api)
    scene.add_light(extra_lights(api)[0])
    scene.ambient_occlusion = _ao(radius=0.3)
    z, f, got = _hold(scene, "torus_spot, two lights")
    assert _bits(got, f) > 0
    scene.close()


# ---------------------------------------------------------------------------- 2. the overlay goes on F' and Z
def test_overlay(api):
    from py_numpy_renderer_amd import _native
    scene = scenes.cube_outward(api)
    scene.ambient_occlusion = _ao(radius=0.3)
    z_off, f_off = _plain_taps(scene, overlay=False)
    z_on, f_on = _plain_taps(scene, overlay=True)
    _, ao_off, _ = _ao_frame(scene)
    scene.draw_debug_frustum = True
    out, ao_on, z_ao = _ao_frame(scene)
    untouched = (f_off.view(np.uint32) == f_on.view(np.uint32)).all(axis=-1)
    assert 0 < int((~untouched).sum()) < untouched.size // 4, "the plain scene's overlay drew nothing, or everything"
    assert _bits(ao_on[untouched], ao_off[untouched]) == 0, "the overlay changed a sample its lines do not touch"
    assert _bits(ao_off, f_off) > 0, "the obscurance darkened nothing"
    assert np.array_equal(z_ao.view(np.uint64), z_on.view(np.uint64)), "Z is not the plain scene's after its overlay"
    _, want_rgb = _native.host_accum(ao_on[None], [1.0], shift=0, scale=1.0, want_acc=False)
    assert np.array_equal(out, want_rgb)
    # the lines are not darkened: where the plain overlay left the line's own red, the obscured frame shows it too
    red = (f_on == np.array([1.0, 0.0, 0.0], dtype=np.float32)).all(axis=-1) & ~untouched
    assert red.any() and _bits(ao_on[red], f_on[red]) == 0, "a line of the overlay was darkened"
    scene.close()


# ---------------------------------------------------------------------------- 3. identity: the full resolve against the in-tile bytes
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


@pytest.mark.parametrize("build", [_plain, _supersampled, _overlaid])
def test_no_pair_passes_is_the_plain_frame(api, build):
    scene = build(api)
    want = scene.render().copy()
    before = scene._backend().ao_debug()[0]
    scene.ambient_occlusion = _ao(bias=NO_PAIR)
    got = scene.render().copy()
    assert scene._backend().ao_debug()[0] == before + 1, "k_ao did not run"
    assert np.array_equal(got, want), f"{build.__name__}: {int((got != want).sum())} bytes differ"
    scene.ambient_occlusion = None
    assert np.array_equal(scene.render(), want) and scene._backend().ao_debug()[0] == before + 1
    scene.close()


# ---------------------------------------------------------------------------- 4. frames in flight, a map per view
def _views(api):
    kw = dict(near=0.1, backface_culling=True)
    return [(api.Camera((0.5, 1, 2), (0, 0, 0), fovy=fovy, far=far, **kw), api.Camera((0.5, 1, 2), (0, 0, 0), fovy=fovy, far=far, **kw))
            for fovy, far in ((50, 20), (60, 15), (70, 25), (80, 30))]


def test_render_frames_sets_the_map_per_view(api):
    from py_numpy_renderer_amd import _pack
    scene = scenes.diablo_small(api, resolution=(120, 160))
    scene.ambient_occlusion = _ao()
    views = _views(api)
    want, descs = [], set()
    for cam, dbg in views:
        scene.camera, scene.debug_camera = cam, dbg
        want.append(scene.render().copy())
        descs.add(_pack.ao_constants(scene))
    assert len(descs) == 4, "the views share a description"
    got = [frame.copy() for frame in scene.render_frames(views, depth=3)]
    assert len(got) == 4
    for k in range(4):
        assert np.array_equal(got[k], want[k]), f"view {k}: {int((got[k] != want[k]).sum())} bytes differ"
    scene.ambient_occlusion = None
    scene.camera, scene.debug_camera = views[0]
    assert not np.array_equal(scene.render(), want[0]), "the obscurance changed nothing in view 0"
    scene.close()


def test_render_async(api):
    scene = scenes.cube_outward(api)
    scene.ambient_occlusion = _ao(radius=0.3)
    want = scene.render().copy()
    pending = [scene.render_async() for _ in range(3)]
    for frame in pending:
        assert np.array_equal(frame.result(), want)
    scene.close()


# ---------------------------------------------------------------------------- 5. the accumulation sums F'
def test_accumulate_sums_the_darkened_frames(api):
    from py_numpy_renderer_amd import _native
    scene = scenes.cube_outward(api)
    scene.ambient_occlusion = _ao(radius=0.3)
    weights, frames = (0.5, 0.3, 0.2), []
    plain = []
    with scene.accumulate() as acc:
        for k, w in enumerate(weights):
            scene.light.position = np.array([(2.0, 3.0, 4.0), (2.6, 3.0, 3.1), (1.2, 3.4, 4.4)][k])
            plain.append(_plain_taps(scene)[1])
            frames.append(_ao_frame(scene)[1])
            acc.add(w)
        got_acc, got_rgb = acc.float_frame(), acc.result(scale=1).copy()
    assert _bits(frames[0], frames[1]) > 0 and _bits(frames[0], plain[0]) > 0
    want_acc, want_rgb = _native.host_accum(frames, weights, shift=0, scale=1.0)
    assert _bits(got_acc, want_acc) == 0
    assert np.array_equal(got_rgb, want_rgb)
    scene.close()


# ---------------------------------------------------------------------------- 6. overflow
def test_a_frame_that_overflows_ends_with_the_unstarved_frame(api):
    free = scenes.build(api, "diablo_floor_small")
    free.ambient_occlusion = _ao()
    want_rgb, want, _ = _ao_frame(free)
    unstarved = free._backend().ao_debug()[0]
    free.close()

    scene = scenes.build(api, "diablo_floor_small")
    scene.ambient_occlusion = _ao()
    backend = scene._backend()
    backend.sync_scene(scene)                              # (an upload resets the capacities)
    backend.set_list_capacities(**SQUEEZED)
    got_rgb, got, _ = _ao_frame(scene)
    enqueued = backend.ao_debug()[0]
    print(f"k_ao enqueued {enqueued} times with the lists squeezed, {unstarved} without")
    assert enqueued >= 2 and enqueued > unstarved, "the frame did not overflow"
    assert _bits(got, want) == 0 and np.array_equal(got_rgb, want_rgb)
    scene.close()


# ---------------------------------------------------------------------------- 7. refusals on the device path
def test_refusals_and_switching_off(api):
    from py_numpy_renderer_amd import _native, multigpu
    scene = scenes.cube_outward(api, resolution=(64, 96))
    parent = scene.render().copy()
    backend = scene._backend()
    assert backend.ao_debug() == (0, 0, 0)
    with pytest.raises(RuntimeError, match="no frame with ambient occlusion"):
        backend.ao_time()
    band_desc, shape = backend._prepare_desc(scene, True, (0, 32), False, False, False, False, None, False, False)
    band_desc = _native.FrameDesc.from_buffer_copy(band_desc)
    scene.ambient_occlusion = _ao(radius=1.0)
    darkened = scene.render().copy()
    assert not np.array_equal(darkened, parent) and backend.ao_debug() == (1, 64, 96)
    with pytest.raises(ValueError, match="whole frames"):
        scene.render(row_band=(0, 32))
    out = np.zeros(shape, dtype=np.uint8)
    rc = backend.lib.mr_render(backend.handle, C.byref(band_desc), out.ctypes.data, None)
    assert rc == _native.MR_E_INVALID and b"whole frames" in backend.lib.mr_last_error()
    assert backend.ao_debug() == (1, 64, 96) and not out.any(), "the refused band reached the device"
    with pytest.raises(ValueError, match="ambient_occlusion"):
        multigpu.BandRenderer(scene)
    scene.ambient_occlusion = None
    assert np.array_equal(scene.render(), parent) and backend.ao_debug() == (1, 64, 96)
    assert scene.render(row_band=(0, 32)).shape == (32, 96, 3)           # (a band renders again)
    scene.close()
