"""``Model.pose`` (``mr_scene_set_model_pose``): what can be checked without a GPU -- the setter, the scene signature,
the packed scene the oracle renders, the C ABI's argument validation on the built library (a scene is created and filled
without a device), and that the poses the GPU tests use move something."""
import ctypes as C

import numpy as np
import pytest

import pose_ref
import scenes

MR_E_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_native()
    from py_numpy_renderer_amd import _native
    return _native.load_library()


# ---------------------------------------------------------------------------- the Python API
def test_pose_defaults_to_none_and_stores_a_float64_copy(api):
    cube = scenes.cube_small(api).models[0]
    assert cube.pose is None
    m = np.eye(4, dtype=np.float32)
    m[3, 0] = 0.25
    cube.pose = m
    assert cube.pose.dtype == np.float64 and cube.pose.shape == (4, 4)
    assert np.array_equal(cube.pose, m.astype(np.float64))
    m[3, 0] = 7                                                    # a copy: the caller's array is not looked at again
    assert cube.pose[3, 0] == 0.25
    with pytest.raises(ValueError):
        cube.pose[0, 0] = 2.0                                      # read-only: a new pose is assigned, not edited in
    cube.pose = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [1, 2, 3, 1]]       # anything float64 can be made of
    assert cube.pose[3].tolist() == [1.0, 2.0, 3.0, 1.0]
    cube.pose = None
    assert cube.pose is None


@pytest.mark.parametrize("bad, error", [
    (np.eye(3), ValueError), (np.zeros((4, 4, 1)), ValueError), (np.zeros(16), ValueError), (1.0, ValueError),
    (np.full((4, 4), np.nan), ValueError), (np.diag([1, 1, 1, np.inf]), ValueError),
    ("rotate", TypeError), (b"0123456789abcdef", TypeError), ([["a"] * 4] * 4, ValueError), (object(), TypeError),
    ([[None] * 4] * 4, ValueError),                                # (NumPy reads None as NaN)
])
def test_pose_setter_rejects(api, bad, error):
    cube = scenes.cube_small(api).models[0]
    keep = np.diag([2.0, 2.0, 2.0, 1.0])
    cube.pose = keep
    with pytest.raises(error):
        cube.pose = bad
    assert np.array_equal(cube.pose, keep)                         # a rejected pose leaves the last one


def test_pose_never_touches_vertices_and_is_absolute(api):
    from py_numpy_renderer_amd._pack import posed_vertices
    cube = scenes.cube_small(api).models[0]
    before = cube.vertices.copy()
    poses = pose_ref.matrices(api)
    cube.pose = poses["rotation"]
    once = posed_vertices(cube)
    cube.pose = poses["translation"]
    cube.pose = poses["rotation"]
    assert np.array_equal(posed_vertices(cube).view(np.uint64), once.view(np.uint64))
    assert once.dtype == np.float64
    assert np.array_equal(once.view(np.uint64), pose_ref.posed_vertices(cube, poses["rotation"]).view(np.uint64))
    assert cube.vertices.dtype == before.dtype and np.array_equal(cube.vertices, before)


def test_pose_is_not_part_of_the_scene_signature(api):
    from py_numpy_renderer_amd._native import DeviceRenderer
    scene = scenes.cube_outward(api)
    sig = DeviceRenderer._scene_signature(scene)
    for m in pose_ref.matrices(api).values():
        scene.models[0].pose = m
        assert DeviceRenderer._scene_signature(scene) == sig
    scene.models[1].pose = np.eye(4)
    assert DeviceRenderer._scene_signature(scene) == sig


@pytest.mark.parametrize("name", ["cube_outward", "torus_spot"])
def test_packed_scene_of_a_posed_model_is_the_twins(api, name):
    """``pack_scene`` -- what the oracle renders -- of a posed scene holds the twin's arrays: float64 posed vertices,
    ``vertices_are_f32`` off, everything else untouched."""
    from py_numpy_renderer_amd._pack import pack_scene
    m = pose_ref.matrices(api)["product"]
    scene, index = pose_ref.build(api, name)
    plain = pack_scene(scene)
    scene.models[index].pose = m
    posed, want = pack_scene(scene), pack_scene(pose_ref.twin(api, name, m))
    for k, (a, b) in enumerate(zip(posed.models, want.models)):
        assert np.array_equal(a.vertices.view(np.uint64), b.vertices.view(np.uint64)), k
        assert a.vertices_are_f32 == b.vertices_are_f32 and np.array_equal(a.faces, b.faces)
        assert (a.normals is None and b.normals is None) or np.array_equal(a.normals, plain.models[k].normals)
    assert not posed.models[index].vertices_are_f32
    assert not np.array_equal(posed.models[index].vertices, plain.models[index].vertices)


# ---------------------------------------------------------------------------- the C ABI
def _scene_with_a_triangle(lib, f32=True):
    from py_numpy_renderer_amd import _native
    handle = lib.mr_scene_create()
    assert handle
    verts = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1]], dtype=np.float64)
    faces = np.array([[[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]]], dtype=np.int32)
    mats = (_native.MaterialDesc * 1)()
    mats[0].tex_kd = mats[0].tex_norm = mats[0].tex_ks = -1
    d = _native.ModelDesc()
    d.vertices, d.faces, d.materials = verts.ctypes.data, faces.ctypes.data, mats
    d.n_vertices, d.n_faces, d.n_materials = 3, 1, 1
    d.vertices_are_f32, d.clip, d.depth_test = int(f32), 1, 1
    assert lib.mr_scene_add_model(handle, C.byref(d)) == 0
    return handle


def test_abi_version_is_still_4(lib):
    from py_numpy_renderer_amd import _native
    assert lib.mr_abi_version() == 4 and _native.ABI_VERSION == 4


def test_set_model_pose_validates_its_arguments(lib):
    handle = _scene_with_a_triangle(lib)
    m = np.ascontiguousarray(np.diag([2.0, 2.0, 2.0, 1.0]))
    counters = (C.c_int32 * 4)()
    assert lib.mr_debug_pose(handle, counters) == 0 and list(counters) == [0, 0, 0, 0]
    assert lib.mr_scene_set_model_pose(None, 0, m.ctypes.data) == MR_E_INVALID
    for index in (-1, 1, 2 ** 31 - 1):
        assert lib.mr_scene_set_model_pose(handle, index, m.ctypes.data) == MR_E_INVALID, index
        assert b"model index" in lib.mr_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        broken = m.copy()
        broken[2, 1] = bad
        assert lib.mr_scene_set_model_pose(handle, 0, broken.ctypes.data) == MR_E_INVALID
        assert b"finite" in lib.mr_last_error()
    assert lib.mr_debug_pose(handle, counters) == 0 and counters[2] == 0          # a rejected pose is not kept
    assert lib.mr_scene_set_model_pose(handle, 0, None) == 0                      # NULL on an un-posed model: nothing to do
    assert lib.mr_scene_set_model_pose(handle, 0, m.ctypes.data) == 0
    assert lib.mr_debug_pose(handle, counters) == 0 and list(counters) == [0, 0, 1, 0]
    assert lib.mr_scene_set_model_pose(handle, 0, None) == 0                      # NULL removes it
    assert lib.mr_debug_pose(handle, counters) == 0 and list(counters) == [0, 0, 0, 0]
    assert lib.mr_debug_pose(handle, None) == MR_E_INVALID
    out = np.zeros(16, np.uint32)
    assert lib.mr_debug_read_clusters(handle, out.ctypes.data, 1) == MR_E_INVALID  # nothing committed yet
    assert lib.mr_scene_set_model_pose(handle, 0, m.ctypes.data) == 0
    assert lib.mr_scene_clear(handle) == 0                                        # the models go, and their poses with them
    assert lib.mr_debug_pose(handle, counters) == 0 and counters[2] == 0
    assert lib.mr_scene_set_model_pose(handle, 0, m.ctypes.data) == MR_E_INVALID
    lib.mr_scene_destroy(handle)


# ---------------------------------------------------------------------------- the poses move something
def test_the_rotation_is_no_no_op_for_the_oracle(api, oracle_mod):
    """The oracle's frame of cube_outward's twin under the rotation differs from the un-posed frame at more than 1 % of
    the pixels; posing through ``Model.pose`` gives the oracle the same scene as the twin."""
    rotation = pose_ref.matrices(api)["rotation"]
    scene, index = pose_ref.build(api, "cube_outward")
    plain = oracle_mod.render(scene)
    want = oracle_mod.render(pose_ref.twin(api, "cube_outward", rotation))
    changed = (plain.out != want.out).any(axis=2).mean()
    assert changed > 0.01, changed
    scene.models[index].pose = rotation
    posed = oracle_mod.render(scene)
    assert np.array_equal(posed.out, want.out) and np.array_equal(posed.z.view(np.uint64), want.z.view(np.uint64))


@pytest.mark.parametrize("name", pose_ref.MATRIX_NAMES)
def test_every_pose_of_the_tests_moves_vertices(api, name):
    cube = scenes.cube_small(api).models[0]
    moved = pose_ref.posed_vertices(cube, pose_ref.matrices(api)[name])
    assert moved.dtype == np.float64 and np.array_equal(moved[:, 3], np.ones(len(moved)))
    assert np.abs(moved[:, :3] - cube.vertices[:, :3]).max() > 0.05
