"""GPU: ``Scene.layers`` -- the per-sample data layers of rendered frames (k_layers in kernels_layers.h, host_layers.h).

The yardstick is the host mirror ``mr_host_layers`` (held to the NumPy restatement and to exact arithmetic by
tests/test_layers_cpu.py), fed with the frame's own winner map (``read_winner``), the face records the device holds after its
pose pass (``read_face_records``) and the description the frame was issued with: ``read_layers()`` must match bit for bit, and
no sample of these scenes may be degenerate.  What the description must hold -- the jittered sample grid, the eye depth -- is
checked on its own: against ``_pack.layer_matrix``, by projecting every covered sample's position back to its own (x, y),
and against the z-buffer's eye depth on a quad that faces the camera.

``test_depth_is_the_z_buffer_s_eye_depth_on_a_quad_that_faces_the_camera``: measured on the CPU from the oracle's z-buffer of
that scene, the largest difference between the mirror's depth and ``float32(ao_eye_depth(Z))`` is 6.92e-06 at eye depths
2.499993 .. 2.500007 (the z-buffer interpolates its linearised z with float32 barycentrics, about 3e-6 of the value; the
mirror's own error is a float32 step, 2.4e-07); the test allows four times that."""
import numpy as np
import pytest

import layers_fields as lf
import layers_ref as ref
import pose_ref
import scenes
import skin_ref

pytestmark = pytest.mark.gpu

SMALL = (48, 64)
KW = dict(fovy=60, near=0.1, far=20, backface_culling=True)
PAN = [(0.5, 1.0, 2.0), (0.9, 1.0, 1.8), (1.4, 1.2, 1.4)]
SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)      # the capacities of test_accumulate_gpu.py's overflow test
MEASURED_DEPTH_DIFFERENCE = 6.92e-06                                # (module docstring)


def _layers(names=ref.NAMES):
    from py_numpy_renderer_amd import Layers
    return Layers(tuple(names))


def _look(api, scene, position, center=(0, 0, 0)):
    scene.camera, scene.debug_camera = api.Camera(position, center, **KW), api.Camera(position, center, **KW)


def _face_off(scene):
    return np.cumsum([0] + [len(m._faces) for m in scene.models[:-1]]).astype(np.int32)


def _issued(scene):
    """The description the scene's last frame was issued with."""
    from py_numpy_renderer_amd import _native
    return _native.LayersDesc.from_buffer_copy(scene._backend()._layers_key)


def _mirror(scene, pos=None, attr=None):
    """(layers, degenerate samples, winner) of the mirror for the scene's last frame."""
    from py_numpy_renderer_amd import _native
    backend = scene._backend()
    winner = backend.read_winner()
    records = backend.read_face_records()
    desc = _issued(scene)
    full = _native.fill_layers_desc(np.frombuffer(bytes(desc), dtype=np.float64, count=16).reshape(4, 4), 0x1ff, desc.n_models)
    got, degenerate = _native.host_layers(winner, records[0] if pos is None else pos, records[1] if attr is None else attr, _face_off(scene), full)
    return got, degenerate, winner


def _hold(scene, label, names=ref.NAMES):
    """Holds ``read_layers()`` of the scene's last frame to the mirror; returns (layers, winner)."""
    want, degenerate, winner = _mirror(scene)
    assert degenerate == 0, f"{label}: {degenerate} degenerate samples"
    assert (winner >= 0).sum() > winner.size // 20, f"{label}: the scene shows next to nothing"
    got = scene.read_layers()
    assert sorted(got) == sorted(names), label
    for name in names:
        assert got[name].shape[:2] == winner.shape
        assert lf.same_bits(got[name], want[name]) == 0, f"{label}: {lf.same_bits(got[name], want[name])} words of {name} are not the mirror's"
    return got, winner


def _matrix_is_the_packer_s(scene):
    from py_numpy_renderer_amd import _pack
    s = np.frombuffer(bytes(_issued(scene)), dtype=np.float64, count=16).reshape(4, 4)
    assert np.array_equal(s, _pack.layer_matrix(scene))
    return s


# ---------------------------------------------------------------------------- 1. frames against the mirror
@pytest.mark.parametrize("recipe, settings, names", [
    ("cube_outward", {}, ref.NAMES),
    ("cube_outward", {"supersample": 2}, ref.NAMES),
    ("tetra_ortho", {}, ref.NAMES),
    ("wall_nine_materials", {}, ("material", "depth", "uv")),
], ids=["cube", "supersample2", "orthographic", "nine_materials_subset"])
def test_read_layers_is_the_mirror_and_the_frame_is_unchanged(api, recipe, settings, names):
    scene, twin = getattr(scenes, recipe)(api, resolution=SMALL), getattr(scenes, recipe)(api, resolution=SMALL)
    for s in (scene, twin):
        for name, value in settings.items():
            setattr(s, name, value)
    scene.layers = _layers(names)
    frame, plain = scene.render().copy(), twin.render().copy()
    assert np.array_equal(frame, plain), f"{int((frame != plain).sum())} bytes of the frame changed with layers set"
    got, winner = _hold(scene, recipe, names)
    ss = settings.get("supersample", 1)
    assert winner.shape == (ss * SMALL[0], ss * SMALL[1])
    assert scene._backend().layers_debug() == (1, *winner.shape, sum(1 << ref.NAMES.index(n) for n in names))
    assert scene._backend().layers_time() > 0
    _matrix_is_the_packer_s(scene)
    covered = winner >= 0
    if "depth" in got:
        # (upstream's one-sample boxes can hand a sample to a face it lies outside of -- in wall_nine_materials one sample goes
        # to a face of the cube seen edge-on, 0.8 sample beside it: such a sample is extrapolated on the face's plane like any
        # other, here to barycentrics (1/6, -11/6, 8/3) and the camera plane.  The mirror's barycentrics say which they are.)
        in_front = covered & (_mirror(scene)[0]["barycentric"] > -1e-3).all(axis=2)
        assert in_front.sum() >= covered.sum() - 2
        assert np.isinf(got["depth"][~covered]).all() and (got["depth"][in_front] > 0).all() and np.isfinite(got["depth"][covered]).all()
    if "model" in got:
        assert (got["model"][~covered] == -1).all() and set(got["model"][covered].tolist()) == set(range(len(scene.models))[recipe == "tetra_ortho":])      # (the small orthographic view shows the floor alone)
        lam = got["barycentric"][covered]
        assert (lam > -1e-3).all() and np.allclose(lam.sum(axis=1), 1, atol=1e-5), "a covered sample lies inside its face"
        assert np.allclose(np.linalg.norm(got["normal"][covered], axis=1), 1, atol=1e-5)
        assert np.allclose(np.linalg.norm(got["face_normal"][covered], axis=1), 1, atol=1e-5)
    if "material" in got:
        assert len(set(got["material"][covered].tolist())) >= (3 if recipe == "wall_nine_materials" else 1)
    # the taps and the plain frame afterwards: off again is the old frame, and nothing is left to read
    scene.layers = None
    assert np.array_equal(scene.render(), plain)
    with pytest.raises(ValueError, match="without data layers"):
        scene.read_layers()
    scene.close(), twin.close()


def _records_from_models(scene, vertices):
    """FacePos64 records built from the models' own arrays: corners = vertices[face corner]; material and flags zero."""
    from py_numpy_renderer_amd import _native
    corners = []
    for m, v in zip(scene.models, vertices):
        corners.append(np.asarray(v, dtype=np.float64)[np.asarray(m._faces)[:, :, 0].astype(np.int64)])
    corners = np.concatenate(corners)
    pos = np.zeros(len(corners), dtype=_native.FACE_POS_DTYPES[False])
    pos["v"] = corners[:, :, :4]
    return pos, np.zeros(len(corners), dtype=_native.FACE_ATTR_DTYPE)


def test_a_posed_float32_model_with_pose_normals(api):
    scene, index = pose_ref.build(api, (lambda a: scenes.torus_spot(a, resolution=SMALL, nu=16, nv=10), 0))
    model = scene.models[index]
    assert np.asarray(model.vertices).dtype == np.float32
    matrix = pose_ref.matrices(api)["rotation"]
    model.pose, model.pose_normals = matrix, True
    scene.layers = _layers()
    scene.render()
    pos, _ = scene._backend().read_face_records()
    assert pos.dtype["v"].base == np.float64, "a posed float32 model: the records are FacePos64"
    got, winner = _hold(scene, "posed torus")
    # once more with the corners built independently: the geometric layers do not read the normals
    vertices = [pose_ref.posed_vertices(m, matrix) if k == index else np.asarray(m.vertices, dtype=np.float64) for k, m in enumerate(scene.models)]
    mine, attr = _records_from_models(scene, vertices)
    assert np.array_equal(mine["v"][:, :, :3], pos["v"][:, :, :3]), "the device's corners are pose_ref's"
    want, degenerate, _ = _mirror(scene, pos=mine, attr=attr)
    assert degenerate == 0
    for name in ("model", "face", "barycentric", "depth", "position", "face_normal"):
        assert lf.same_bits(got[name], want[name]) == 0, name
    # the shading normals follow the pose: they differ from the unposed model's
    model.pose_normals = False
    scene.render()
    other = scene.read_layers()["normal"]
    assert lf.same_bits(other, got["normal"]) > 0 and lf.same_bits(scene.read_layers()["position"], got["position"]) == 0
    scene.close()


def test_a_skinned_model_with_auto_normals(api):
    from py_numpy_renderer_amd import Skin
    scene = scenes.cube_outward(api, resolution=SMALL)
    cube = scene.models[0]
    joints, weights, bones = skin_ref.rig(api, cube, "bend", frame=1)
    cube.skin, cube.bones = Skin(joints, weights), bones
    scene.layers = _layers()
    scene.render()
    stiff, _ = _hold(scene, "skinned cube")
    cube.auto_normals = True
    scene.render()
    rebuilt, _ = _hold(scene, "skinned cube, auto_normals")
    assert lf.same_bits(rebuilt["normal"], stiff["normal"]) > 0, "the rebuilt normals are the stiff ones"
    assert lf.same_bits(rebuilt["position"], stiff["position"]) == 0
    scene.close()


# ---------------------------------------------------------------------------- 2. the description
def test_temporal_aa_layers_follow_the_jittered_grid(api):
    """Each covered sample's position, projected through the S the frame was issued with, returns the sample's own (x, y)
    within 0.01 sample: float32 rounding of a unit-scale position gives about 1e-4 sample, a dropped jitter at least 0.1."""
    from py_numpy_renderer_amd import TemporalAA, _pack
    scene = scenes.cube_outward(api, resolution=SMALL)
    scene.temporal_aa = TemporalAA(blend=0.2, jitter=8)
    scene.layers = _layers(("position", "depth"))
    jittered = 0
    for k in range(4):
        scene.render()
        got, winner = _hold(scene, f"taa frame {k}", ("position", "depth"))
        s = np.frombuffer(bytes(_issued(scene)), dtype=np.float64, count=16).reshape(4, 4)
        plain = _pack.layer_matrix(scene)                      # (the jitter lives only while a frame is issued: this is the grid without it)
        ys, xs = np.nonzero(winner >= 0)
        p = np.c_[got["position"][ys, xs].astype(np.float64), np.ones(len(ys))]

        def miss(matrix):
            q = p @ matrix
            return np.abs(np.c_[q[:, 0] / q[:, 2] - xs, q[:, 1] / q[:, 2] - ys]).max()
        print(f"frame {k}: through the issued S {miss(s):.2e} sample, through the un-jittered grid {miss(plain):.2e}")
        assert miss(s) < 0.01, f"frame {k}: a position lands {miss(s)} sample from its own sample"
        # the issued S is the plain grid moved by the frame's offset, w times it in homogeneous terms
        moved = np.abs((p @ s)[:, :2] / (p @ s)[:, 2:3] - (p @ plain)[:, :2] / (p @ plain)[:, 2:3]).max()
        if moved >= 0.1:
            jittered += 1
            assert miss(plain) >= 0.09, "the un-jittered grid is told apart"
        assert np.allclose((p @ s)[:, 3], got["depth"][ys, xs], rtol=1e-5)
    assert jittered >= 2, "the sequence had no frame with an offset of a tenth of a sample"
    scene.close()


def _facing_quad(api):
    """quad_negative_uv seen along the quad's normal: every sample of the quad has one eye depth."""
    scene = scenes.quad_negative_uv(api, resolution=SMALL)
    normal = np.array([0.0, 0.25, 1.1]) / np.hypot(0.25, 1.1)
    centre = np.array([0.0, 0.05, 0.075])
    _look(api, scene, tuple(centre + 2.5 * normal), tuple(centre))
    return scene


def depth_against_z(scene, z, winner, depth):
    """The largest |depth - float32(ao_eye_depth(Z))| over the samples of model 0 (the quad)."""
    from py_numpy_renderer_amd import _pack
    m = _pack.depth_map(scene, scene.camera)
    quad = (winner >= 0) & (winner < len(scene.models[0]._faces))
    assert quad.sum() > 200
    eye = ((m[0] * z[quad] + m[1]) / (m[2] * z[quad] + m[3])).astype(np.float32)
    return float(np.abs(depth[quad].astype(np.float64) - eye.astype(np.float64)).max()), float(eye.min()), float(eye.max())


def test_depth_is_the_z_buffer_s_eye_depth_on_a_quad_that_faces_the_camera(api):
    scene = _facing_quad(api)
    scene.layers = _layers(("depth",))
    scene.render()
    got, winner = _hold(scene, "facing quad", ("depth",))
    largest, near, far = depth_against_z(scene, scene._backend().read_z(), winner, got["depth"])
    print(f"largest |depth - eye depth of Z| on the quad: {largest:.3e} (eye depths {near} .. {far}); measured on the CPU: {MEASURED_DEPTH_DIFFERENCE:.3e}")
    assert far - near < 1e-4, "the quad faces the camera"
    assert largest <= 4 * MEASURED_DEPTH_DIFFERENCE
    scene.close()


# ---------------------------------------------------------------------------- 3. composition
def test_render_frames_with_two_views_in_flight(api):
    scene = scenes.cube_outward(api, resolution=SMALL)
    scene.layers = _layers(("depth", "face"))
    want = []
    for place in PAN[:3]:
        _look(api, scene, place)
        scene.render()
        want.append({k: v.copy() for k, v in scene.read_layers().items()})
    assert lf.same_bits(want[0]["depth"], want[1]["depth"]) > 0
    views = [(api.Camera(p, (0, 0, 0), **KW), api.Camera(p, (0, 0, 0), **KW)) for p in PAN[:3]]
    # read_layers() reads the frame enqueued last: while frame k is handed out, frame k + 1 is in flight and is that frame
    for k, _ in enumerate(scene.render_frames(views, depth=2)):
        newest = min(k + 1, 2)
        got = scene.read_layers()
        for name in ("depth", "face"):
            assert lf.same_bits(got[name], want[newest][name]) == 0, f"after frame {k}: {name} is not view {newest}'s"
    # two frames in flight own their buffers: the first one's layers are still its own when the second has been issued
    _look(api, scene, PAN[0])
    first = scene.render_async()
    _look(api, scene, PAN[1])
    second = scene.render_async()
    first.result(), second.result()
    assert lf.same_bits(scene.read_layers()["depth"], want[1]["depth"]) == 0
    scene.close()


def test_a_frame_rendered_again_after_a_list_overflow(api):
    def frames(squeeze):
        scene = scenes.build(api, "diablo_floor_small")
        scene.draw_debug_frustum = False
        scene.layers = _layers(("face", "depth", "normal"))
        scene.render()
        backend = scene._backend()
        if squeeze:
            backend.set_list_capacities(**SQUEEZED)
        _look(api, scene, (0.56, 1.0, 1.97))
        before = backend.layers_debug()[0]
        out = scene.render().copy()
        got = {k: v.copy() for k, v in scene.read_layers().items()}
        _hold(scene, f"squeezed {squeeze}", ("face", "depth", "normal"))
        enqueued = backend.layers_debug()[0] - before
        scene.close()
        return out, got, enqueued

    want_rgb, want, once = frames(False)
    got_rgb, got, enqueued = frames(True)
    assert once == 1 and enqueued >= 2, "the frame did not overflow"
    assert np.array_equal(got_rgb, want_rgb)
    for name in want:
        assert lf.same_bits(got[name], want[name]) == 0, name


def test_every_other_pass_switched_on_beside_it(api):
    from py_numpy_renderer_amd import AmbientOcclusion, Bloom, DepthOfField, LightShafts, MotionBlur, ToneMap
    scene, twin = scenes.cube_outward(api, resolution=SMALL), scenes.cube_outward(api, resolution=SMALL)
    for s in (scene, twin):
        s.add_light(api.Light((-2, 3, 1), ambient_strength=0.05, specular_strength=0.1))
        s.ambient_occlusion, s.depth_of_field, s.motion_blur = AmbientOcclusion(), DepthOfField(), MotionBlur()
        s.bloom, s.light_shafts, s.tone_map = Bloom(threshold=0.3), LightShafts(), ToneMap()
        s.draw_debug_frustum = True
    scene.layers = _layers()
    for k, place in enumerate(PAN[:2]):
        _look(api, scene, place), _look(api, twin, place)
        frame, plain = scene.render().copy(), twin.render().copy()
        assert np.array_equal(frame, plain), f"frame {k}: {int((frame != plain).sum())} bytes changed with layers set"
        _hold(scene, f"all passes, frame {k}")
    assert scene._backend().read_velocity().shape == (*SMALL, 2)
    scene.close(), twin.close()


# ---------------------------------------------------------------------------- 4. refusals
def test_the_refusals(api):
    import ctypes as C
    from py_numpy_renderer_amd import _native, multigpu
    scene = scenes.cube_outward(api, resolution=SMALL)
    scene.render()
    backend = scene._backend()
    assert backend.layers_debug() == (0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="no frame with data layers yet"):
        backend.layers_time()
    with pytest.raises(ValueError, match="without data layers"):
        scene.read_layers()
    band_desc, shape = backend._prepare_desc(scene, True, (0, 16), False, False, False, False, None, False, False)
    band_desc = _native.FrameDesc.from_buffer_copy(band_desc)
    full_desc, _ = backend._prepare_desc(scene, True, None, True, False, False, False, None, False, False)
    full_desc = _native.FrameDesc.from_buffer_copy(full_desc)
    scene.layers = _layers(("depth",))
    scene.render()
    assert sorted(scene.read_layers()) == ["depth"]
    assert backend.lib.mr_read_layers(backend.handle, 5, np.zeros(4).ctypes.data) == _native.MR_E_INVALID
    assert b"without this layer" in backend.lib.mr_last_error()
    assert backend.lib.mr_read_layers(backend.handle, 9, np.zeros(4).ctypes.data) == _native.MR_E_INVALID
    # split frames, with the sentence the other passes use
    with pytest.raises(ValueError, match="takes whole frames \\(no row band, no stripes\\): its taps cross the bands"):
        scene.render(row_band=(0, 16))
    out = np.zeros(shape, dtype=np.uint8)
    assert backend.lib.mr_render(backend.handle, C.byref(band_desc), out.ctypes.data, None) == _native.MR_E_INVALID
    assert b"data layers takes whole frames (no row band, no stripes): its taps cross the bands" in backend.lib.mr_last_error() and not out.any()
    with pytest.raises(ValueError, match="does not support layers"):
        multigpu.BandRenderer(scene, 0, 2)
    # a caller's stream, an accumulation
    with pytest.raises(ValueError, match="render\\(\\) / render_async\\(\\)"):
        backend.render_device(scene, 0)
    assert backend.lib.mr_render_device(backend.handle, C.byref(full_desc), C.c_void_p(out.ctypes.data), None) == _native.MR_E_INVALID      # (refused before the pointer is looked at)
    assert b"data layers" in backend.lib.mr_last_error()
    with pytest.raises(ValueError, match="accumulate"):
        scene.accumulate()
    assert backend.lib.mr_accum_begin(backend.handle) == 0
    assert backend.lib.mr_accum_add(backend.handle, C.byref(full_desc), C.c_double(1.0)) == _native.MR_E_INVALID
    assert b"data layers are not available" in backend.lib.mr_last_error()
    # the description's own checks
    s = np.eye(4)
    for bad, text in ((_native.fill_layers_desc(s, 0, 2), b"mask"), (_native.fill_layers_desc(s, 1, 3), b"n_models"),
                      (_native.fill_layers_desc(s * np.nan, 1, 2), b"not finite")):
        assert backend.lib.mr_scene_set_layers(backend.handle, C.byref(bad)) == _native.MR_E_INVALID
        assert text in backend.lib.mr_last_error()
    assert sorted(scene.read_layers()) == ["depth"], "a refusal left the last frame's layers alone"
    scene.close()
