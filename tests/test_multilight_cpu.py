"""Several lights in one frame (``Scene.add_light``; ``mr_scene_set_extra_lights``): what can be checked without a
GPU -- the premises of the definition (``multilight_ref``) on the oracle, the Python API, the packed descriptors and
the C ABI's argument validation on the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes
from multilight_ref import compose, compose_frames, extra_lights, per_light

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENES = ["cube_small", "diablo_small", "diablo_floor", "diablo_floor_lh_gl", "torus_spot", "cube_skybox",
          "cube_tetra_nodepth", "kat_house", "fins_nonmanifold", "tetra_ortho", "wall_nine_materials"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_native()
    from py_numpy_renderer_amd import _native
    return _native.load_library()


# ---------------------------------------------------------------------------- the definition's premises
@pytest.mark.parametrize("name", SCENES)
def test_composer_with_one_light_is_the_oracles_frame(api, oracle_mod, name):
    scene = getattr(scenes, name)(api)
    want = oracle_mod.render(scene)
    got = compose(oracle_mod, scene, [scene.light])
    assert np.array_equal(got.frame.view(np.uint32), want.frame.view(np.uint32))
    assert np.array_equal(got.out, want.out)
    assert np.array_equal(got.stencils[0], want.stencil)


@pytest.mark.parametrize("name", SCENES)
def test_visibility_and_background_do_not_depend_on_the_light(api, oracle_mod, name):
    scene = getattr(scenes, name)(api)
    per = per_light(oracle_mod, scene, [scene.light, *extra_lights(api)])
    uncovered = per[0].winner < 0
    for r in per[1:]:
        assert np.array_equal(r.z.view(np.uint64), per[0].z.view(np.uint64))
        assert np.array_equal(r.winner, per[0].winner)
        assert np.array_equal(r.frame[uncovered].view(np.uint32), per[0].frame[uncovered].view(np.uint32))


def test_compose_frames_adds_in_float32_in_order_and_clamps():
    a = np.full((1, 3, 3), 0.3, np.float32)
    b = np.full((1, 3, 3), 0.6, np.float32)
    c = np.full((1, 3, 3), 0.05, np.float32)
    winner = np.array([[0, -1, 5]])
    f = compose_frames([a, b, c], winner)
    assert f.dtype == np.float32
    assert f[0, 0, 0] == (np.float32(0.3) + np.float32(0.6)) + np.float32(0.05)
    assert f[0, 1, 0] == np.float32(0.3)                       # uncovered: the first frame's background
    assert compose_frames([b, b], winner)[0, 2, 1] == np.float32(1.0)


# ---------------------------------------------------------------------------- the Python API
def test_add_light_lights_clear_lights(api):
    scene = scenes.cube_small(api)
    assert scene.lights == [scene.light]
    extras = extra_lights(api)
    for k, light in enumerate(extras):
        scene.add_light(light)
        assert scene.lights == [scene.light, *extras[:k + 1]]
        assert light.scene is scene
    listed = scene.lights
    listed.append(None)                                        # the list is a copy
    assert len(scene.lights) == 4
    with pytest.raises(ValueError, match="at most 4"):
        scene.add_light(api.Light((0, 5, 0)))
    assert len(scene.lights) == 4
    scene.clear_lights()
    assert scene.lights == [scene.light]
    with pytest.raises(TypeError):
        scene.add_light("lamp")


def test_verbose_is_refused_with_several_lights(api):
    scene = scenes.cube_small(api)
    scene.add_light(extra_lights(api)[0])
    scene.verbose = True
    with pytest.raises(ValueError, match="verbose"):
        scene.render()                                         # raised before any device work
    with pytest.raises(ValueError, match="verbose"):
        scene.render_async()


def test_band_renderer_refuses_several_lights(api):
    pytest.importorskip("torch")
    from py_numpy_renderer_amd import multigpu
    scene = scenes.cube_small(api)
    scene.add_light(extra_lights(api)[0])
    with pytest.raises(ValueError, match="more than one light"):
        multigpu.BandRenderer(scene, rank=0, world=2)


def test_show_light_gets_its_gizmo(api, tmp_path, monkeypatch):
    """add_light(show=True) adds the gizmo model exactly as assigning scene.light does."""
    scenes.gizmo_files()
    monkeypatch.chdir(scenes.GENERATED)
    a = scenes.cube_small(api)
    n = len(a.models)
    a.add_light(api.Light((-3, 2.5, 1.5), show=True))
    b = scenes.cube_small(api)
    b.light = api.Light((-3, 2.5, 1.5), show=True)
    assert len(a.models) == len(b.models) == n + 1
    assert np.array_equal(np.asarray(a.models[-1].vertices), np.asarray(b.models[-1].vertices))


# ---------------------------------------------------------------------------- packing
def _desc_bytes(d):
    return bytes(C.string_at(C.addressof(d), C.sizeof(d)))


@pytest.mark.parametrize("name", ["cube_small", "diablo_floor_lh_gl", "torus_spot"])
def test_extra_lights_are_packed_like_the_first_light(api, name):
    from py_numpy_renderer_amd import _native
    from py_numpy_renderer_amd._pack import pack_frame, pack_light
    scene = getattr(scenes, name)(api)
    own = scene.light
    extras = extra_lights(api)
    for light in extras:
        scene.add_light(light)
    pf = pack_frame(scene)
    assert len(pf.extra_lights) == 3
    for light, packed in zip(extras, pf.extra_lights):
        solo = getattr(scenes, name)(api)
        solo.light = light
        ps = pack_frame(solo)
        assert ps.extra_lights == ()
        d, f = _native.fill_light_desc(packed), _native.fill_frame_desc(ps)
        assert d.type == f.light_type
        for mine, theirs in (("pos", "light_pos"), ("dir", "light_dir"), ("color", "light_color"), ("ambient", "light_ambient")):
            assert list(getattr(d, mine)) == list(getattr(f, theirs)), mine
        for field in ("specular_strength", "att_constant", "att_linear", "att_quadratic", "spot_edge0", "spot_edge1"):
            assert getattr(d, field) == getattr(f, field), field
        assert _desc_bytes(d) == _desc_bytes(_native.fill_light_desc(pack_light(light)))
    # light 0 is untouched by the extras
    scene.clear_lights()
    assert scene.light is own
    plain = _native.fill_frame_desc(pack_frame(scene))
    assert _desc_bytes(plain) == _desc_bytes(_native.fill_frame_desc(pf))


def test_frame_key_follows_an_extra_light(api):
    """The host's one-entry cache of the packed frame must notice an extra light that moved, changed or left."""
    from py_numpy_renderer_amd._native import DeviceRenderer
    scene = scenes.cube_small(api)
    key = lambda: DeviceRenderer._frame_key(scene, True)
    k0 = key()
    light = extra_lights(api)[0]
    scene.add_light(light)
    k1 = key()
    assert k1 != k0
    light.set_position(np.array((-2.0, 2.5, 1.5)))
    k2 = key()
    assert k2 != k1
    light.color = np.array((0.2, 0.3, 0.4))
    assert key() != k2
    scene.clear_lights()
    assert key() == k0


# ---------------------------------------------------------------------------- the C ABI, no device
def test_light_desc_layout_and_abi_version(lib):
    from py_numpy_renderer_amd import _native
    assert lib.mr_abi_struct_size(5) == C.sizeof(_native.LightDesc) == 8 + 12 * 8 + 6 * 8
    assert lib.mr_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "mi355rast.h")).read()
    assert "#define MR_MAX_LIGHTS 4" in header


def test_set_extra_lights_validates_its_arguments(lib, api):
    from py_numpy_renderer_amd import _native
    from py_numpy_renderer_amd._pack import pack_light
    handle = lib.mr_scene_create()
    assert handle
    descs = (_native.LightDesc * 4)(*[_native.fill_light_desc(pack_light(x)) for x in extra_lights(api) + extra_lights(api)[:1]])
    assert lib.mr_scene_set_extra_lights(None, descs, 1) == -1
    assert lib.mr_scene_set_extra_lights(handle, descs, 4) == -1 and b"at most" in lib.mr_last_error()
    assert lib.mr_scene_set_extra_lights(handle, descs, -1) == -1
    assert lib.mr_scene_set_extra_lights(handle, None, 1) == -1 and b"NULL" in lib.mr_last_error()
    bad = (_native.LightDesc * 1)(_native.fill_light_desc(pack_light(extra_lights(api)[0])))
    bad[0].type = 3
    assert lib.mr_scene_set_extra_lights(handle, bad, 1) == -1 and b"light type" in lib.mr_last_error()
    for n in (3, 2, 1, 0):
        assert lib.mr_scene_set_extra_lights(handle, descs, n) == 0
    assert lib.mr_scene_set_extra_lights(handle, None, 0) == 0
    lib.mr_scene_destroy(handle)


def test_frames_that_extra_lights_refuse(lib, api):
    """MR_FRAME_FACE_STATUS and striped frames with extra lights: MR_E_INVALID before any device is looked for."""
    from py_numpy_renderer_amd import _native
    from py_numpy_renderer_amd._pack import pack_frame, pack_light
    scene = scenes.cube_small(api)
    pf = pack_frame(scene)
    handle = lib.mr_scene_create()
    descs = (_native.LightDesc * 1)(_native.fill_light_desc(pack_light(extra_lights(api)[0])))
    assert lib.mr_scene_set_extra_lights(handle, descs, 1) == 0
    out = np.zeros((pf.height, pf.width, 3), np.uint8)
    status = _native.fill_frame_desc(pf, face_status=True)
    striped = _native.fill_frame_desc(pf, stripe=(0, 2))
    for what, d, word in (("face status", status, b"FACE_STATUS"), ("stripes", striped, b"striped")):
        assert lib.mr_render(handle, C.byref(d), out.ctypes.data, None) == -1, what
        assert word in lib.mr_last_error(), what
        assert lib.mr_render_async(handle, C.byref(d), out.ctypes.data, 0) == -1, what
        assert lib.mr_render_device(handle, C.byref(d), out.ctypes.data, None) == -1, what
    # without the extra light the same descriptors get past validation (and fail only for want of a device, if there is none)
    assert lib.mr_scene_set_extra_lights(handle, None, 0) == 0
    rc = lib.mr_render(handle, C.byref(status), out.ctypes.data, None)
    assert rc == 0 or b"FACE_STATUS" not in lib.mr_last_error()
    lib.mr_scene_destroy(handle)
