"""``Model.pose_normals`` (``mr_scene_set_model_pose_normals``): what can be checked without a GPU -- the setter, the
normal matrix, the posed normals and maps, the packed scene the oracle renders, the oracle's frames of posed scene and
twin, and the C ABI's argument validation on the built library."""
import ctypes as C
import math

import numpy as np
import pytest

import pose_normals_ref as ref
import pose_ref
import scenes
from py_numpy_renderer_amd import _fp

MR_E_INVALID = -1
SINGULAR = np.diag([1.0, 0.0, 1.0, 1.0])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_native()
    from py_numpy_renderer_amd import _native
    return _native.load_library()


# ---------------------------------------------------------------------------- the setter
def test_pose_normals_defaults_to_false(api):
    cube = scenes.cube_small(api).models[0]
    assert cube.pose_normals is False
    assert api.Model(np.zeros((3, 4)), None, None, np.zeros((1, 3, 4), dtype=np.int32)).pose_normals is False


@pytest.mark.parametrize("value, want", [(True, True), (False, False), (np.True_, True), (np.False_, False), (1, True), (0, False),
                                         (np.int32(1), True), (np.uint8(0), False)])
def test_pose_normals_accepts(api, value, want):
    cube = scenes.cube_small(api).models[0]
    cube.pose_normals = not want
    cube.pose_normals = value
    assert cube.pose_normals is want


@pytest.mark.parametrize("bad", [2, -1, 1.0, 0.0, "yes", "", None, [True], np.ones(1, dtype=bool), np.eye(3), object()])
def test_pose_normals_rejects(api, bad):
    cube = scenes.cube_small(api).models[0]
    for keep in (True, False):
        cube.pose_normals = keep
        with pytest.raises(TypeError):
            cube.pose_normals = bad
        assert cube.pose_normals is keep                          # a rejected value leaves the last one


def test_a_singular_pose_raises_only_together_with_pose_normals(api):
    cube = scenes.cube_small(api).models[0]
    rotation = pose_ref.matrices(api)["rotation"]
    cube.pose = SINGULAR                                           # legal, as it always was
    with pytest.raises(ValueError, match="pose_normals needs an invertible pose"):
        cube.pose_normals = True                                   # this assignment completes the pair
    assert cube.pose_normals is False and np.array_equal(cube.pose, SINGULAR)
    cube.pose = rotation
    cube.pose_normals = True
    with pytest.raises(ValueError, match="pose_normals needs an invertible pose"):
        cube.pose = SINGULAR                                       # ... and so does this one
    assert cube.pose_normals is True and np.array_equal(cube.pose, rotation)
    cube.pose = None                                               # no pose: nothing to invert
    cube.pose_normals = True
    with pytest.raises(ValueError, match="pose_normals needs an invertible pose"):
        cube.pose = SINGULAR
    assert cube.pose is None
    cube.pose_normals = False
    cube.pose = SINGULAR
    huge = np.diag([1e200, 1e200, 1e200, 1.0])                     # cofactors and determinant overflow: G is not finite
    cube.pose = huge
    with pytest.raises(ValueError, match="pose_normals needs an invertible pose"):
        cube.pose_normals = True
    assert cube.pose_normals is False


def test_pose_normals_is_not_part_of_the_scene_signature(api):
    from py_numpy_renderer_amd._native import DeviceRenderer
    scene = scenes.cube_outward(api)
    sig = DeviceRenderer._scene_signature(scene)
    scene.models[0].pose = pose_ref.matrices(api)["rotation"]
    scene.models[0].pose_normals = True
    assert DeviceRenderer._scene_signature(scene) == sig


# ---------------------------------------------------------------------------- the normal matrix
def test_normal_matrix_analytic_cases(api):
    from py_numpy_renderer_amd._pack import normal_matrix
    m = pose_ref.matrices(api)
    g = normal_matrix(m["translation"])
    assert g.dtype == np.float64 and g.shape == (3, 3)
    assert np.array_equal(g, np.eye(3))                            # exactly
    r = m["rotation"]
    # (pose_ref's rotation is a float32 matrix widened: orthogonal to float32's 6e-8, so its R^-T is R to that and no
    # better; the same three turns formed in float64 are a rotation to float64's precision and held to 1e-15)
    def turn(axis, degrees):
        c, s, out = math.cos(math.radians(degrees)), math.sin(math.radians(degrees)), np.eye(4)
        i, j = ((1, 2), (2, 0), (0, 1))[axis]
        out[i, i] = out[j, j] = c
        out[i, j], out[j, i] = s, -s
        return out
    exact = turn(0, 17) @ turn(1, 31) @ turn(2, -9)
    assert np.abs(normal_matrix(exact) - exact[:3, :3]).max() <= 1e-15
    print('float32 rotation: |G - R| <=', np.abs(normal_matrix(r) - r[:3, :3]).max())
    assert np.abs(normal_matrix(r) - r[:3, :3]).max() <= 4 * 2.0 ** -24
    assert np.array_equal(normal_matrix(np.diag([2.0, -4.0, 0.5, 1.0])), np.diag([0.5, -0.25, 2.0]))    # powers of two: exact
    # three roundings (two products, one quotient) on the way to 1/a: a few units of 2^-53, relative
    got, want = np.diag(normal_matrix(m["mirror"])), 1.0 / np.diag(m["mirror"])[:3]
    assert np.abs(got / want - 1).max() <= 4 * 2.0 ** -53
    assert np.array_equal(normal_matrix(m["mirror"]) - np.diag(got), np.zeros((3, 3)))
    p = m["product"]
    assert np.abs(normal_matrix(p) @ p[:3, :3].T - np.eye(3)).max() <= 1e-14
    for name in pose_ref.MATRIX_NAMES:                             # the helper's restatement is the same arithmetic
        assert np.array_equal(normal_matrix(m[name]).view(np.uint64), ref.normal_matrix(m[name]).view(np.uint64)), name
    with pytest.raises(ValueError):
        normal_matrix(SINGULAR)


def test_posed_normals_are_the_chain_in_float32(api):
    from py_numpy_renderer_amd._pack import normal_matrix, posed_normal_map, posed_normals
    scene, index = ref.build(api, "diablo_nm_object")
    model = scene.models[index]
    plain = np.asarray(model.normals, dtype=np.float32).copy()
    assert posed_normals(model) is model.normals                   # no pose: the array itself
    model.pose = pose_ref.matrices(api)["product"]
    assert posed_normals(model) is model.normals                   # pose_normals off: still
    model.pose_normals = True
    g = normal_matrix(model.pose)
    got = posed_normals(model)
    assert got.dtype == np.float32 and got.shape == plain.shape
    for row in (0, 1, len(plain) // 2, len(plain) - 1):
        n = [float(x) for x in plain[row]]
        for j in range(3):
            acc = n[0] * float(g[0, j])
            for k in (1, 2):
                acc = _fp.fma(n[k], float(g[k, j]), acc)
            assert got[row, j] == np.float32(acc), (row, j)
    lengths = np.linalg.norm(got.astype(np.float64), axis=1)
    assert np.abs(lengths - 1).max() > 0.05                        # not re-normalised (the product scales)
    assert np.array_equal(np.asarray(model.normals, dtype=np.float32), plain)          # the model's own stay
    texels = model.materials["default"].norm
    baked = posed_normal_map(texels, g)
    assert baked.dtype == np.float32 and baked.shape == texels.shape
    assert np.array_equal(baked, ref.chain_f32(texels, g)) and not np.array_equal(baked, texels)
    # G = I: the same normals, bit for bit -- but for a component that is -0.0 (diablo has one), which the chain's
    # sum with the two zero products makes +0.0: rn(-0.0 * 1) = -0.0, fma(n1, 0.0, -0.0) = +0.0
    model.pose = pose_ref.matrices(api)["translation"]
    same = posed_normals(model)
    assert np.array_equal(same, plain)
    assert np.array_equal(same.view(np.uint32)[plain != 0], plain.view(np.uint32)[plain != 0])


# ---------------------------------------------------------------------------- the packed scene
def _assert_packed_equal(got, want, label):
    assert len(got.models) == len(want.models) and len(got.textures) == len(want.textures), label
    for k, (a, b) in enumerate(zip(got.textures, want.textures)):
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label, "texture", k)
    for k, (a, b) in enumerate(zip(got.models, want.models)):
        assert np.array_equal(a.vertices.view(np.uint64), b.vertices.view(np.uint64)), (label, k)
        assert (a.normals is None) == (b.normals is None), (label, k)
        if a.normals is not None:
            assert a.normals.dtype == b.normals.dtype == np.float32
            assert np.array_equal(a.normals.view(np.uint32), b.normals.view(np.uint32)), (label, k)
        assert a.vertices_are_f32 == b.vertices_are_f32 and np.array_equal(a.faces, b.faces), (label, k)
        assert [(m.tex_kd, m.tex_norm, m.tex_ks, m.norm_tangent) for m in a.materials] == \
               [(m.tex_kd, m.tex_norm, m.tex_ks, m.norm_tangent) for m in b.materials], (label, k)


@pytest.mark.parametrize("name", ["diablo_floor", "diablo_nm_object", "quad_rect_object_nm", "torus_spot", "tetra_bare"])
def test_packed_scene_of_a_posed_model_is_the_twins(api, name):
    from py_numpy_renderer_amd._pack import pack_scene
    m = pose_ref.matrices(api)["product"]
    scene, index = ref.build(api, name)
    plain = pack_scene(scene)
    ref.pose(scene.models[index], m)
    posed = pack_scene(scene)
    _assert_packed_equal(posed, pack_scene(ref.twin(api, name, m)), name)
    model = scene.models[index]
    if model.normals is not None:
        assert not np.array_equal(posed.models[index].normals, plain.models[index].normals)
    for k, mat in enumerate(plain.models[index].materials):        # object-space maps are re-baked, the other maps are not
        after = posed.models[index].materials[k]
        for field in ("tex_kd", "tex_ks", "tex_norm"):
            a, b = getattr(mat, field), getattr(after, field)
            assert (a < 0) == (b < 0)
            if a >= 0:
                changed = not np.array_equal(plain.textures[a], posed.textures[b])
                assert changed == (field == "tex_norm" and not mat.norm_tangent), (name, k, field)
    scene.models[index].pose_normals = False                       # and without the attribute: today's packed scene
    _assert_packed_equal(pack_scene(scene), pack_scene(pose_ref.twin(api, ref.RECIPES[name], m)), name + ", pose_normals off")


def test_a_shared_map_gives_two_textures(api):
    from py_numpy_renderer_amd._pack import pack_scene
    m = pose_ref.matrices(api)
    scene, _ = ref.build(api, ref.TWO_QUADS)
    assert scene.models[0].materials["default"].norm is scene.models[1].materials["default"].norm
    plain = pack_scene(scene)
    assert plain.models[0].materials[0].tex_norm == plain.models[1].materials[0].tex_norm      # one entry today
    ref.pose(scene.models[0], m["rotation"])
    ref.pose(scene.models[1], m["mirror"], normals=False)
    posed = pack_scene(scene)
    a, b = posed.models[0].materials[0].tex_norm, posed.models[1].materials[0].tex_norm
    assert a != b and len(posed.textures) == len(plain.textures) + 1
    assert np.array_equal(posed.textures[b], plain.textures[plain.models[1].materials[0].tex_norm])    # the other keeps the original
    _assert_packed_equal(posed, pack_scene(ref.twin(api, ref.TWO_QUADS, {0: m["rotation"], 1: m["mirror"]}, normals=(0,))), "first")
    scene.models[1].pose_normals = True                            # both: a copy each, with its own G
    both = pack_scene(scene)
    assert len(both.textures) == len(plain.textures) + 1 and not np.array_equal(*(both.textures[mm.materials[0].tex_norm] for mm in both.models[:2]))
    _assert_packed_equal(both, pack_scene(ref.twin(api, ref.TWO_QUADS, {0: m["rotation"], 1: m["mirror"]})), "both")
    assert np.array_equal(scene.models[0].materials["default"].norm, plain.textures[plain.models[0].materials[0].tex_norm])    # the array stays


# ---------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", ["diablo_nm_object", "diablo_floor"])
def test_the_oracle_renders_the_twin_and_the_normals_matter(api, oracle_mod, name):
    """The oracle's frame of the posed scene is its frame of the twin, bit for bit; and so that nothing here passes
    vacuously, under the rotation the frame with ``pose_normals`` differs from the one without at a lit pixel."""
    rotation = pose_ref.matrices(api)["rotation"]
    scene, index = ref.build(api, name)
    ref.pose(scene.models[index], rotation)
    posed = oracle_mod.render(scene)
    want = oracle_mod.render(ref.twin(api, name, rotation))
    for key in ("out", "frame", "z", "winner", "stencil"):
        a, b = getattr(posed, key), getattr(want, key)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, key)
    scene.models[index].pose_normals = False
    without = oracle_mod.render(scene)
    assert np.array_equal(without.z.view(np.uint64), posed.z.view(np.uint64))           # the same geometry
    lit = (posed.stencil == 0) & (posed.winner >= 0)
    differs = (posed.out != without.out).any(axis=2) & lit
    print(f"{name}: {int(differs.sum())} of {int(lit.sum())} lit pixels differ")
    assert differs.any(), name


# ---------------------------------------------------------------------------- the C ABI
def _scene_with_a_triangle(lib):
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
    d.vertices_are_f32, d.clip, d.depth_test = 0, 1, 1
    assert lib.mr_scene_add_model(handle, C.byref(d)) == 0
    return handle


def test_the_symbol_is_bound_and_the_abi_version_is_still_4(lib):
    from py_numpy_renderer_amd import _native
    assert lib.mr_abi_version() == 4 and _native.ABI_VERSION == 4
    assert _native._PROTOTYPES["mr_scene_set_model_pose_normals"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p])
    fn = lib.mr_scene_set_model_pose_normals
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int32, C.c_void_p]
    assert _native._PROTOTYPES["mr_debug_pose_normals_times"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float)])
    assert _native.DeviceRenderer.POSE_TIME_NAMES == ("pose_vertices", "face_normals", "edge_normals", "face_static", "clusters")


def test_set_model_pose_normals_validates_its_arguments(lib):
    """On a scene filled without a device (the library's usual behaviour there: the call keeps the matrix and launches
    nothing)."""
    handle = _scene_with_a_triangle(lib)
    m = np.ascontiguousarray(np.diag([2.0, 2.0, 2.0, 1.0]))
    g = np.ascontiguousarray(np.diag([0.5, 0.5, 0.5]))
    counters = (C.c_int32 * 4)()
    assert lib.mr_scene_set_model_pose_normals(None, 0, g.ctypes.data) == MR_E_INVALID
    assert lib.mr_scene_set_model_pose_normals(handle, 0, g.ctypes.data) == MR_E_INVALID      # no pose yet
    assert b"pose" in lib.mr_last_error()
    assert lib.mr_scene_set_model_pose_normals(handle, 0, None) == MR_E_INVALID
    assert lib.mr_scene_set_model_pose(handle, 0, m.ctypes.data) == 0
    for index in (-1, 1, 2 ** 31 - 1):
        assert lib.mr_scene_set_model_pose_normals(handle, index, g.ctypes.data) == MR_E_INVALID, index
        assert b"model index" in lib.mr_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        broken = g.copy()
        broken[2, 1] = bad
        assert lib.mr_scene_set_model_pose_normals(handle, 0, broken.ctypes.data) == MR_E_INVALID
        assert b"finite" in lib.mr_last_error()
    assert lib.mr_scene_set_model_pose_normals(handle, 0, None) == 0                          # NULL on a model without one
    assert lib.mr_scene_set_model_pose_normals(handle, 0, g.ctypes.data) == 0
    assert lib.mr_scene_set_model_pose_normals(handle, 0, g.ctypes.data) == 0                 # the same again
    assert lib.mr_scene_set_model_pose_normals(handle, 0, None) == 0                          # NULL removes it
    assert lib.mr_scene_set_model_pose_normals(handle, 0, g.ctypes.data) == 0
    assert lib.mr_scene_set_model_pose(handle, 0, None) == 0                                  # the pose goes, and the matrix with it
    assert lib.mr_scene_set_model_pose_normals(handle, 0, None) == MR_E_INVALID
    assert lib.mr_debug_pose(handle, counters) == 0 and list(counters) == [0, 0, 0, 0]        # nothing ran
    times = (C.c_float * 2)()
    assert lib.mr_debug_pose_normals_times(handle, times) == MR_E_INVALID                     # no pass yet
    assert lib.mr_debug_pose_normals_times(handle, None) == MR_E_INVALID
    assert lib.mr_scene_set_model_pose(handle, 0, m.ctypes.data) == 0
    assert lib.mr_scene_set_model_pose_normals(handle, 0, g.ctypes.data) == 0
    assert lib.mr_scene_clear(handle) == 0                                                    # the models go
    assert lib.mr_scene_set_model_pose_normals(handle, 0, g.ctypes.data) == MR_E_INVALID
    lib.mr_scene_destroy(handle)


def test_sync_poses_hands_the_matrix_over_once(api, lib):
    """``sync_poses`` keys a model by (pose, G): the library is called when either changed and not otherwise."""
    from py_numpy_renderer_amd import _native
    calls = []

    class Spy:
        def __init__(self, name):
            self.name = name

        def __call__(self, handle, index, ptr):
            n = 16 if self.name == "pose" else 9
            calls.append((self.name, index, None if not ptr else np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), (n,)).copy()))
            return 0

    class FakeLib:
        mr_scene_set_model_pose = Spy("pose")
        mr_scene_set_model_pose_normals = Spy("normals")

    renderer = _native.DeviceRenderer.__new__(_native.DeviceRenderer)
    renderer.lib, renderer.handle, renderer._pose_keys = FakeLib(), 1, [None, None]
    scene = scenes.cube_outward(api)
    cube = scene.models[0]
    m = pose_ref.matrices(api)
    renderer.sync_poses(scene)
    assert calls == []
    cube.pose = m["rotation"]
    renderer.sync_poses(scene)
    assert [c[:2] for c in calls] == [("pose", 0)]                 # pose_normals off: the new entry point is not called
    calls.clear()
    cube.pose_normals = True
    renderer.sync_poses(scene)
    assert [c[:2] for c in calls] == [("pose", 0), ("normals", 0)]
    assert np.array_equal(calls[1][2], ref.normal_matrix(m["rotation"]).ravel())      # G row-major, the twin's nine numbers
    calls.clear()
    renderer.sync_poses(scene)
    assert calls == []
    cube.pose = m["product"]
    renderer.sync_poses(scene)
    assert [c[:2] for c in calls] == [("pose", 0), ("normals", 0)] and np.array_equal(calls[1][2], ref.normal_matrix(m["product"]).ravel())
    calls.clear()
    cube.pose_normals = False
    renderer.sync_poses(scene)
    assert [c[:2] for c in calls] == [("pose", 0), ("normals", 0)] and calls[1][2] is None
    calls.clear()
    cube.pose_normals = True
    renderer.sync_poses(scene)
    calls.clear()
    cube.pose = None                                               # the library lets go of the matrix with the pose
    renderer.sync_poses(scene)
    assert [c[:2] for c in calls] == [("pose", 0)] and calls[0][2] is None
    renderer.handle = None
