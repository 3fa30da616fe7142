"""GPU: ``Scene.depth_of_field`` -- a thin lens' blur gathered from the float frame and the z-buffer on the device (k_dof in
kernels_dof.h, host_dof.h, launch_after_tile in host_frame.h).

The yardstick is test_ao_gpu.py's: the host mirror ``mr_host_dof`` (held to the NumPy restatement dof_ref.py in
test_dof_cpu.py) applied to the z-buffer Z and the float frame F the same scene hands out through its taps WITHOUT the
feature.  The float frame F' of the scene with it must match bit for bit, the frame's bytes must be
``mr_host_accum([F'], [1], scale=1)`` byte for byte, and Z must be unchanged.  Beside it: the obscurance in front of it, the
overlay, identities with ``render()``, frames in flight, the accumulation, overflow, refusals."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import dof_ref
import scenes
from multilight_ref import extra_lights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the capacities of test_accumulate_gpu.py's overflow test
IN_FOCUS = 1e-4                                                     # a lens so small that c < 0.5 everywhere in these scenes


def _dof(**kw):
    from py_numpy_renderer_amd import DepthOfField
    return DepthOfField(**kw)


def _desc(scene):
    from py_numpy_renderer_amd import _native, _pack
    return _native.fill_dof_desc(*_pack.dof_constants(scene))


def _circle(scene, z):
    from py_numpy_renderer_amd import _pack
    return dof_ref.circle(z, *_pack.dof_constants(scene))


def _plain_taps(scene, overlay=False):
    """(Z, F) of the scene as it is now, rendered without depth of field and without obscurance: the taps after the
    overlay where one is drawn."""
    held = scene.depth_of_field, scene.ambient_occlusion
    scene.depth_of_field = scene.ambient_occlusion = None
    backend = scene._backend()
    try:
        backend.render(scene, keep_float=True, counters=False, keep_buffers=True, overlay=overlay)
        return backend.read_z().copy(), backend.read_frame_f32().copy()
    finally:
        scene.depth_of_field, scene.ambient_occlusion = held


def _dof_frame(scene):
    """(bytes, F', Z) of ``render()`` with the scene's depth of field: the library keeps the taps by itself."""
    out = scene.render().copy()
    backend = scene._backend()
    return out, backend.read_frame_f32().copy(), backend.read_z().copy()


def _bits(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def _changed(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1)


def _hold(scene, label):
    """The yardstick on the scene as it is (no overlay); returns (Z, F, F')."""
    from py_numpy_renderer_amd import _native
    assert not scene.draw_debug_frustum
    z, f = _plain_taps(scene)
    out, got, z_after = _dof_frame(scene)
    before = f
    if scene.ambient_occlusion is not None:
        from py_numpy_renderer_amd import _pack
        before = _native.host_ao(z, f, _native.fill_ao_desc(scene.ambient_occlusion, *_pack.ao_constants(scene)))
    want = _native.host_dof(z, before, _desc(scene))
    s = scene.supersample
    _, want_rgb = _native.host_accum(got[None], [1.0], shift={1: 0, 2: 1, 4: 2}[s], scale=1.0, want_acc=False)
    c = np.minimum(np.abs(_circle(scene, z)), 16)
    bits, steps = _bits(got, want), int(np.abs(out.astype(np.int16) - want_rgb.astype(np.int16)).max())
    print(f"{label}: {bits} floats differ from the mirror, bytes differ by at most {steps}, c in [{c.min():.3f}, {c.max():.3f}], "
          f"{_changed(got, before).mean():.1%} of {z.size} samples changed")
    assert got.shape == f.shape and out.shape == want_rgb.shape
    assert bits == 0, f"{label}: the float frame is not the mirror's"
    assert steps == 0, f"{label}: the bytes are not the finalise of the float frame"
    assert np.array_equal(z_after.view(np.uint64), z.view(np.uint64)), f"{label}: the z-buffer changed"
    return z, before, got


# ---------------------------------------------------------------------------- 1. shapes at which the kernel can go wrong
@pytest.mark.parametrize("resolution, lens", [((16, 16), dict(lens_radius=0.5)), ((16, 16), dict(focus=0.25, lens_radius=2.0)),
                                              ((37, 41), dict(lens_radius=0.215)), ((37, 41), dict(focus=0.25, lens_radius=2.0))])
def test_small_frames(api, resolution, lens):
    """(16, 16): one workgroup whose halo is larger than the frame.  (37, 41): partial workgroups in both directions.
    Each with a lens whose largest circle is about 3 samples (the sky's, kf) and with one focused so near, and so wide,
    that every sample is clamped at 16: then every tap of the 33 x 33 inside the frame and the disc passes."""
    scene = scenes.cube_outward(api, resolution=resolution)
    scene.depth_of_field = _dof(**lens)
    z, f, got = _hold(scene, f"cube_outward at {resolution}, {lens}")
    c = np.abs(_circle(scene, z))
    assert np.isfinite(z).any() and (~np.isfinite(z)).any()
    if "focus" in lens:
        assert c.min() >= 16, "the circle is not clamped everywhere"
    else:
        assert 2.5 <= c.max() <= 3.5
    assert _bits(got, f) > 0
    assert scene._backend().dof_debug()[1:] == resolution
    assert scene._backend().dof_time() > 0
    scene.close()


def test_diablo_small_with_the_defaults(api):
    scene = scenes.diablo_small(api)
    scene.depth_of_field = _dof()
    z, f, got = _hold(scene, "diablo_small (240, 320), defaults")
    changed = _changed(got, f)
    assert changed.any() and not changed.all(), "some samples change, some do not"
    scene.close()


@pytest.mark.parametrize("s", [2, 4])
def test_supersampled(api, s):
    """kf scales with the sample grid's height, and the clamp is in samples."""
    scene = scenes.diablo_small(api, resolution=(30, 40))
    scene.supersample = s
    scene.depth_of_field = _dof(lens_radius=0.2)
    z, f, got = _hold(scene, f"diablo_small (30, 40), supersample {s}")
    assert got.shape == (30 * s, 40 * s, 3) and _bits(got, f) > 0
    scene.close()


def test_orthographic(api):
    """A circle that grows linearly with the depth, and a background whose z is -inf: clamped."""
    scene = scenes.tetra_ortho(api)
    scene.depth_of_field = _dof(lens_radius=0.05)
    z, f, got = _hold(scene, "tetra_ortho")
    sky = ~np.isfinite(z)
    assert (z[sky] < 0).all() and np.isinf(_circle(scene, z)[sky]).all() and _bits(got, f) > 0
    scene.close()


# diablo_floor_lh_gl at (135, 240) focused far behind the model: the sky's circle is 0.4 samples, the model's up to 3.5, so
# workgroups that see the model walk a disc and the others take one tap
_LH_GL = dict(focus=50.0, lens_radius=0.3)


def _digest(frame):
    return hashlib.sha256(np.ascontiguousarray(frame).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lh_gl_digest(api):
    scene = scenes.diablo_floor_lh_gl(api, resolution=(135, 240))
    scene.depth_of_field = _dof(**_LH_GL)
    z, f, got = _hold(scene, "diablo_floor_lh_gl (135, 240)")
    rr = dof_ref.squared_radius(_circle(scene, z))
    tops = set()
    for y0 in range(0, 135, 32):                     # the largest rr a 32 x 32 workgroup stages, halo included
        for x0 in range(0, 240, 32):
            tops.add(int(rr[max(y0 - 16, 0):y0 + 48, max(x0 - 16, 0):x0 + 48].max()))
    print(f"largest squared radii the workgroups meet: {sorted(tops)}")
    assert min(tops) == 0 and max(tops) >= 9, "the workgroups do not meet different bounds"
    changed = _changed(got, f)
    assert changed.any() and not changed.all()
    scene.close()
    return _digest(got)


def test_workgroups_that_meet_different_bounds(lh_gl_digest):
    assert len(lh_gl_digest) == 64


_CHILD = r"""
import hashlib, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import scenes
from py_numpy_renderer_amd import DepthOfField, _native, _pack
api = scenes.product_api()
scene = scenes.diablo_floor_lh_gl(api, resolution=(135, 240))
scene.draw_debug_frustum = False
scene.depth_of_field = DepthOfField(**{lens!r})
scene.render()
print("digest", hashlib.sha256(np.ascontiguousarray(scene._backend().read_frame_f32()).tobytes()).hexdigest())
scene.close()
"""


@pytest.mark.parametrize("shape", ["32x32", "32x32x256", "16x16"])
def test_every_workgroup_shape_gives_the_same_bits(lh_gl_digest, shape):
    """MR_DOF_TILE is read once per process: a fresh child renders with each shape."""
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lens=_LH_GL)
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MR_DOF_TILE=shape), timeout=300, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    lines = [ln.split()[1] for ln in proc.stdout.splitlines() if ln.startswith("digest ")]
    assert lines == [lh_gl_digest], f"MR_DOF_TILE={shape}: the float frame is not the default shape's"


def test_the_sky_blurs(api):
    scene = scenes.cube_skybox(api)
    scene.depth_of_field = _dof(lens_radius=0.1)
    z, f, got = _hold(scene, "cube_skybox")
    sky = ~np.isfinite(z)
    assert sky.any() and len(np.unique(f[sky], axis=0)) > 16, "no sky in the frame"
    ys, xs = np.nonzero(~sky)
    beside = np.zeros_like(sky)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        beside[np.clip(ys + dy, 0, sky.shape[0] - 1), np.clip(xs + dx, 0, sky.shape[1] - 1)] = True
    beside &= sky
    # (such a sample becomes the mean of the sky samples of its disc: it keeps its bits only where the sky is constant there)
    share = float(_changed(got, f)[beside].mean())
    print(f"{int(beside.sum())} sky samples touch the cube, {share:.1%} of them changed")
    assert beside.sum() > 50 and share > 0.5, "the sky next to the cube kept its colours"
    scene.close()


def test_two_lights(api):
    scene = scenes.torus_spot(api)
    scene.add_light(extra_lights(api)[0])
    scene.depth_of_field = _dof(lens_radius=0.1)
    z, f, got = _hold(scene, "torus_spot, two lights")
    assert _bits(got, f) > 0
    scene.close()


# ---------------------------------------------------------------------------- 2. composition
def test_the_obscurance_runs_in_front_of_it(api):
    from py_numpy_renderer_amd import AmbientOcclusion
    scene = scenes.diablo_small(api, resolution=(120, 160))
    scene.ambient_occlusion = AmbientOcclusion()
    scene.depth_of_field = _dof(lens_radius=0.1)
    z, darkened, got = _hold(scene, "diablo_small (120, 160), obscurance and depth of field")
    _, plain = _plain_taps(scene)
    assert _bits(darkened, plain) > 0 and _bits(got, darkened) > 0
    assert scene._backend().ao_debug()[0] >= 1 and scene._backend().dof_debug()[0] >= 1
    scene.close()


def test_overlay(api):
    """As test_ao_gpu.test_overlay: the lines go on F' and Z, and stay sharp."""
    from py_numpy_renderer_amd import _native
    scene = scenes.cube_outward(api)
    scene.depth_of_field = _dof(lens_radius=0.3)
    z_off, f_off = _plain_taps(scene, overlay=False)
    z_on, f_on = _plain_taps(scene, overlay=True)
    _, dof_off, _ = _dof_frame(scene)
    scene.draw_debug_frustum = True
    out, dof_on, z_dof = _dof_frame(scene)
    untouched = (f_off.view(np.uint32) == f_on.view(np.uint32)).all(axis=-1)
    assert 0 < int((~untouched).sum()) < untouched.size // 4, "the plain scene's overlay drew nothing, or everything"
    assert _bits(dof_on[untouched], dof_off[untouched]) == 0, "the overlay changed a sample its lines do not touch"
    assert _bits(dof_off, f_off) > 0, "the depth of field changed nothing"
    assert np.array_equal(z_dof.view(np.uint64), z_on.view(np.uint64)), "Z is not the plain scene's after its overlay"
    _, want_rgb = _native.host_accum(dof_on[None], [1.0], shift=0, scale=1.0, want_acc=False)
    assert np.array_equal(out, want_rgb)
    # the lines are sharp: where the plain overlay left the line's own red, the blurred frame shows it too
    red = (f_on == np.array([1.0, 0.0, 0.0], dtype=np.float32)).all(axis=-1) & ~untouched
    assert red.any() and _bits(dof_on[red], f_on[red]) == 0, "a line of the overlay was blurred"
    scene.close()


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
def test_a_lens_that_blurs_nothing_gives_the_plain_frame(api, build):
    scene = build(api)
    want = scene.render().copy()
    before = scene._backend().dof_debug()[0]
    scene.depth_of_field = _dof(lens_radius=IN_FOCUS)
    got = scene.render().copy()
    assert scene._backend().dof_debug()[0] == before + 1, "k_dof did not run"
    assert np.abs(_circle(scene, _plain_taps(scene)[0])).max() < 0.5
    assert np.array_equal(got, want), f"{build.__name__}: {int((got != want).sum())} bytes differ"
    scene.depth_of_field = None
    assert np.array_equal(scene.render(), want) and scene._backend().dof_debug()[0] == before + 1
    scene.close()


def test_render_frames_sets_the_description_per_view(api):
    from py_numpy_renderer_amd import _pack
    scene = scenes.diablo_small(api, resolution=(120, 160))
    scene.depth_of_field = _dof(lens_radius=0.1)                    # focus=None: the eye depth of each camera's center
    kw = dict(fovy=60, near=0.1, far=20, backface_culling=True)
    views = [(api.Camera((0.5, 1, 2), center, **kw), api.Camera((0.5, 1, 2), center, **kw))
             for center in ((0, 0, 0), (0.1, 0.3, -1.5), (0, 0, 0), (-0.1, 0.2, 0.8))]
    want, focuses = [], []
    for cam, dbg in views:
        scene.camera, scene.debug_camera = cam, dbg
        want.append(scene.render().copy())
        focuses.append(_pack.dof_constants(scene)[3])
    assert len(set(focuses)) == 3, "the views share a plane in focus"
    got = [frame.copy() for frame in scene.render_frames(views, depth=3)]
    assert len(got) == 4
    for k in range(4):
        assert np.array_equal(got[k], want[k]), f"view {k}: {int((got[k] != want[k]).sum())} bytes differ"
    scene.depth_of_field = None
    scene.camera, scene.debug_camera = views[1]
    assert not np.array_equal(scene.render(), want[1]), "the depth of field changed nothing in view 1"
    scene.close()


def test_render_async(api):
    scene = scenes.cube_outward(api)
    scene.depth_of_field = _dof(lens_radius=0.3)
    want = scene.render().copy()
    pending = [scene.render_async() for _ in range(3)]
    for frame in pending:
        assert np.array_equal(frame.result(), want)
    scene.close()


def test_accumulate_sums_the_blurred_frames(api):
    from py_numpy_renderer_amd import _native
    scene = scenes.cube_outward(api)
    scene.depth_of_field = _dof(lens_radius=0.3)
    weights, frames = (0.5, 0.3, 0.2), []
    plain = []
    with scene.accumulate() as acc:
        for k, w in enumerate(weights):
            scene.light.position = np.array([(2.0, 3.0, 4.0), (2.6, 3.0, 3.1), (1.2, 3.4, 4.4)][k])
            plain.append(_plain_taps(scene)[1])
            frames.append(_dof_frame(scene)[1])
            acc.add(w)
        got_acc, got_rgb = acc.float_frame(), acc.result(scale=1).copy()
    assert _bits(frames[0], frames[1]) > 0 and _bits(frames[0], plain[0]) > 0
    want_acc, want_rgb = _native.host_accum(frames, weights, shift=0, scale=1.0)
    assert _bits(got_acc, want_acc) == 0
    assert np.array_equal(got_rgb, want_rgb)
    scene.close()


def test_a_frame_that_overflows_ends_with_the_unstarved_frame(api):
    free = scenes.build(api, "diablo_floor_small")
    free.depth_of_field = _dof(lens_radius=0.05)
    want_rgb, want, _ = _dof_frame(free)
    unstarved = free._backend().dof_debug()[0]
    free.close()

    scene = scenes.build(api, "diablo_floor_small")
    scene.depth_of_field = _dof(lens_radius=0.05)
    backend = scene._backend()
    backend.sync_scene(scene)                              # (an upload resets the capacities)
    backend.set_list_capacities(**SQUEEZED)
    got_rgb, got, _ = _dof_frame(scene)
    enqueued = backend.dof_debug()[0]
    print(f"k_dof enqueued {enqueued} times with the lists squeezed, {unstarved} without")
    assert enqueued >= 2 and enqueued > unstarved, "the frame did not overflow"
    assert _bits(got, want) == 0 and np.array_equal(got_rgb, want_rgb)
    scene.close()


# ---------------------------------------------------------------------------- 3. refusals on the device path
def test_refusals_and_switching_off(api):
    from py_numpy_renderer_amd import _native, multigpu
    scene = scenes.cube_outward(api, resolution=(64, 96))
    parent = scene.render().copy()
    backend = scene._backend()
    assert backend.dof_debug() == (0, 0, 0)
    with pytest.raises(RuntimeError, match="no frame with depth of field"):
        backend.dof_time()
    band_desc, shape = backend._prepare_desc(scene, True, (0, 32), False, False, False, False, None, False, False)
    band_desc = _native.FrameDesc.from_buffer_copy(band_desc)
    scene.depth_of_field = _dof(lens_radius=0.3)
    blurred = scene.render().copy()
    assert not np.array_equal(blurred, parent) and backend.dof_debug() == (1, 64, 96)
    with pytest.raises(ValueError, match="whole frames"):
        scene.render(row_band=(0, 32))
    out = np.zeros(shape, dtype=np.uint8)
    rc = backend.lib.mr_render(backend.handle, C.byref(band_desc), out.ctypes.data, None)
    assert rc == _native.MR_E_INVALID and b"depth of field takes whole frames" in backend.lib.mr_last_error()
    assert backend.dof_debug() == (1, 64, 96) and not out.any(), "the refused band reached the device"
    with pytest.raises(ValueError, match="depth_of_field"):
        multigpu.BandRenderer(scene)
    scene.depth_of_field = None
    assert np.array_equal(scene.render(), parent) and backend.dof_debug() == (1, 64, 96)
    assert backend.ao_debug() == (0, 0, 0)
    assert scene.render(row_band=(0, 32)).shape == (32, 96, 3)           # (a band renders again)
    scene.close()
