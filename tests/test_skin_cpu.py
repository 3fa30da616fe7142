"""``Model.skin`` / ``Model.bones`` (``mr_scene_set_model_skin``, ``mr_scene_set_model_bones``): what can be checked
without a GPU -- the setters and their refusals, the skinned arrays against an exact rational restatement of the chains
and against the library's host helper, the packed scene the oracle renders, the owner table of the normals, and the C
ABI's argument validation on the built library (a scene is created and filled without a device)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import scenes
import skin_ref
from py_numpy_renderer_amd import Skin

MR_E_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_native()
    from py_numpy_renderer_amd import _native
    return _native.load_library()


def _cube(api):
    return scenes.cube_small(api).models[0]


def _rows(model, joint=0):
    n = len(model.vertices)
    return np.full((n, 4), joint, dtype=np.int64), np.tile([0.4, 0.3, 0.2, 0.1], (n, 1))


# ---------------------------------------------------------------------------- the Python API
def test_skin_and_bones_default_to_none_and_store_read_only_copies(api):
    cube = _cube(api)
    assert cube.skin is None and cube.bones is None
    joints, weights = _rows(cube)
    skin = Skin(joints.astype(np.float32), weights.astype(np.float32), normals=1)      # integral floats are integers
    assert skin.joints.dtype == np.int32 and skin.weights.dtype == np.float64 and skin.normals is True
    assert skin.joints.shape == skin.weights.shape == (len(cube.vertices), 4)
    joints[0, 0] = 9                                               # copies: the caller's arrays are not looked at again
    assert skin.joints[0, 0] == 0
    for arr in (skin.joints, skin.weights):
        with pytest.raises(ValueError):
            arr[0, 0] = 1
    with pytest.raises(AttributeError):
        skin.normals = False
    cube.skin = skin
    assert cube.skin is skin and cube.bones is None
    bones = np.stack([np.eye(4, dtype=np.float32)] * 2)
    cube.bones = bones
    assert cube.bones.dtype == np.float64 and cube.bones.shape == (2, 4, 4)
    bones[0, 0, 0] = 7
    assert cube.bones[0, 0, 0] == 1.0
    with pytest.raises(ValueError):
        cube.bones[0, 0, 0] = 2.0
    cube.bones = None
    assert cube.bones is None and cube.skin is skin
    cube.bones = [np.eye(4).tolist()]
    cube.skin = None                                               # no skin, no bones
    assert cube.skin is None and cube.bones is None
    import py_numpy_renderer_amd as pkg
    assert "Skin" in pkg.__all__ and pkg.Skin is Skin


@pytest.mark.parametrize("joints, weights, normals, error", [
    (np.zeros((8, 3)), np.zeros((8, 3)), False, ValueError),       # shapes
    (np.zeros(32), np.zeros(32), False, ValueError),
    (np.zeros((8, 4)), np.zeros((7, 4)), False, ValueError),
    (np.zeros((8, 4)), np.zeros((8, 4, 1)), False, ValueError),
    (np.zeros((8, 4)), np.full((8, 4), np.nan), False, ValueError),      # weights that are not finite
    (np.zeros((8, 4)), np.full((8, 4), np.inf), False, ValueError),
    (np.full((8, 4), 0.5), np.zeros((8, 4)), False, ValueError),         # joints that are not integral
    (np.full((8, 4), np.nan), np.zeros((8, 4)), False, ValueError),
    (np.full((8, 4), -1), np.zeros((8, 4)), False, ValueError),          # ... or negative
    ("joints", np.zeros((8, 4)), False, TypeError),
    (np.zeros((8, 4)), b"weights", False, TypeError),
    (object(), np.zeros((8, 4)), False, TypeError),
    ([["a"] * 4] * 8, np.zeros((8, 4)), False, ValueError),
    (np.zeros((8, 4)), np.zeros((8, 4)), "yes", TypeError),
    (np.zeros((8, 4)), np.zeros((8, 4)), 2, TypeError),
])
def test_skin_rejects(joints, weights, normals, error):
    with pytest.raises(error):
        Skin(joints, weights, normals=normals)


def test_skin_setter_rejects_and_keeps_the_old_value(api):
    cube = _cube(api)
    n = len(cube.vertices)
    keep = Skin(*_rows(cube))
    cube.skin = keep
    with pytest.raises(TypeError):
        cube.skin = _rows(cube)                                    # a Skin, not its parts
    with pytest.raises(ValueError):
        cube.skin = Skin(np.zeros((n + 1, 4)), np.zeros((n + 1, 4)))       # one row per vertex
    assert cube.skin is keep
    cube.bones = np.stack([np.eye(4)] * 3)
    with pytest.raises(ValueError, match="bone"):
        cube.skin = Skin(np.full((n, 4), 3), np.zeros((n, 4)))     # joint 3 of 3 bones: this assignment completes the pair
    assert cube.skin is keep and len(cube.bones) == 3


@pytest.mark.parametrize("bad, error", [
    (np.eye(4), ValueError), (np.zeros((2, 3, 4)), ValueError), (np.zeros((0, 4, 4)), ValueError), (1.0, ValueError),
    (np.full((1, 4, 4), np.nan), ValueError), (np.stack([np.eye(4), np.diag([1, 1, 1, np.inf])]), ValueError),
    ("bones", TypeError), (b"0123", TypeError), (object(), TypeError), ([[["a"] * 4] * 4], ValueError),
])
def test_bones_setter_rejects_and_keeps_the_old_value(api, bad, error):
    cube = _cube(api)
    cube.skin = Skin(*_rows(cube))
    keep = np.stack([np.diag([2.0, 2.0, 2.0, 1.0])])
    cube.bones = keep
    with pytest.raises(error):
        cube.bones = bad
    assert np.array_equal(cube.bones, keep)


def test_bones_need_a_skin_and_enough_of_them(api):
    cube = _cube(api)
    with pytest.raises(ValueError, match="skin"):
        cube.bones = np.eye(4)[None]
    assert cube.bones is None
    cube.skin = Skin(*_rows(cube, joint=2))
    with pytest.raises(ValueError, match="bone"):
        cube.bones = np.stack([np.eye(4)] * 2)                     # joint 2 of 2 bones: this assignment completes the pair
    assert cube.bones is None
    cube.bones = np.stack([np.eye(4)] * 3)
    with pytest.raises(ValueError, match="bone"):
        cube.bones = np.stack([np.eye(4)] * 2)
    assert len(cube.bones) == 3


def test_a_skin_that_no_longer_fits_its_vertices_is_refused_at_render(api):
    from py_numpy_renderer_amd import _native, _pack
    scene = scenes.cube_small(api)
    cube = scene.models[0]
    cube.skin = Skin(*_rows(cube))
    cube.bones = np.eye(4)[None]
    cube.vertices = np.concatenate([cube.vertices, cube.vertices[:1]])
    with pytest.raises(ValueError, match="rows"):
        _pack.pack_scene(scene)

    class NoDevice(_native.DeviceRenderer):                        # the check comes before any device work
        def __init__(self):
            self._signature = None
    with pytest.raises(ValueError, match="rows"):
        NoDevice().sync_scene(scene)
    cube.bones = None                                              # without bones the skin is not looked at
    _pack.pack_scene(scene)


# ---------------------------------------------------------------------------- the arrays
def _exact_chain(a, b):
    """dot_chain in exact arithmetic: rn(a0 * b0), then one rounding per fma step."""
    acc = float(Fraction(a[0]) * Fraction(b[0]))
    for x, y in zip(a[1:], b[1:]):
        acc = float(Fraction(x) * Fraction(y) + Fraction(acc))
    return acc


def _exact_blend(joints, weights, bones, i):
    picked = [bones[j] for j in joints[i]]
    return [[_exact_chain([float(w) for w in weights[i]], [float(b[r][c]) for b in picked]) for c in range(4)] for r in range(4)]


@pytest.mark.parametrize("name", skin_ref.RIG_NAMES)
def test_skinned_arrays_equal_the_exact_restatement(api, name):
    """~50 vertices of the torus and the normals they own, every rig: ``skinned_vertices`` / ``skinned_normals`` (library
    helper and pure Python) against the chains in ``Fraction`` arithmetic, rounded once per step."""
    from py_numpy_renderer_amd import _pack
    scene, index = skin_ref.build(api, "torus_spot")
    model = scene.models[index]
    joints, weights, bones = skin_ref.rig(api, model, name)
    model.skin, model.bones = Skin(joints, weights, normals=True), bones
    got, pure = _pack.skinned_vertices(model), _pack.skinned_vertices(model, native=False)
    got_n, pure_n = _pack.skinned_normals(model), _pack.skinned_normals(model, native=False)
    assert got.dtype == np.float64 and got_n.dtype == np.float64
    owners = skin_ref.normal_owners(model)
    picked = list(range(0, len(model.vertices), 20))
    assert len(picked) == 50
    for i in picked:
        s = _exact_blend(joints, weights, bones, i)
        v = [float(x) for x in np.asarray(model.vertices[i], dtype=np.float64)]
        want = [_exact_chain(v, [s[r][c] for r in range(4)]) for c in range(4)]
        assert got[i].tolist() == want and pure[i].tolist() == want, i
        for q in (q for q, o in enumerate(owners) if o == i):
            nq = [float(x) for x in np.asarray(model.normals[q], dtype=np.float32).astype(np.float64)]
            want = [_exact_chain(nq, [s[r][c] for r in range(3)]) for c in range(3)]
            assert got_n[q].tolist() == want and pure_n[q].tolist() == want, q


@pytest.mark.parametrize("recipe", ["torus_spot", "kat_house", "cube_outward"])
@pytest.mark.parametrize("name", skin_ref.RIG_NAMES)
def test_the_host_helper_equals_the_pure_python_chains(lib, api, recipe, name):
    """``mr_host_skin_chain`` and its 3-vector sibling (what ``_pack`` uses when the library loads) against the pure-Python
    chains and against ``skin_ref``'s restatement, bit for bit, over whole models."""
    from py_numpy_renderer_amd import _pack
    assert _pack._fast_skin(), "the library is built: _pack must use its helpers"
    scene, index = skin_ref.build(api, recipe)
    model = scene.models[index]
    joints, weights, bones = skin_ref.rig(api, model, name)
    model.skin, model.bones = Skin(joints, weights, normals=True), bones
    fast, pure = _pack.skinned_vertices(model), _pack.skinned_vertices(model, native=False)
    want = skin_ref.skinned_vertices(model.vertices, joints, weights, bones)
    assert np.array_equal(fast.view(np.uint64), pure.view(np.uint64)) and np.array_equal(fast.view(np.uint64), want.view(np.uint64))
    assert not np.array_equal(fast, np.asarray(model.vertices, dtype=np.float64))
    fast, pure = _pack.skinned_normals(model), _pack.skinned_normals(model, native=False)
    want = skin_ref.skinned_normals(model, joints, weights, bones)
    assert np.array_equal(fast.view(np.uint64), pure.view(np.uint64)) and np.array_equal(fast.view(np.uint64), want.view(np.uint64))


def test_the_normal_owner_table_of_kat_house(api):
    """kat_house counts its ``vn`` apart from its ``v`` and indexes both from the end: the owners are the (wrapped)
    vertices at the first corner that names each normal, restated here corner by corner."""
    from py_numpy_renderer_amd import _pack
    model = scenes.kat_house(api).models[0]
    faces = np.asarray(model._faces)
    assert len(model.normals) != len(model.vertices) and (faces[..., 0] < 0).any() and (faces[..., 2] < 0).any()
    owners = _pack.normal_owners(model)
    assert owners.dtype == np.int32 and owners.shape == (len(model.normals),)
    assert owners.tolist() == skin_ref.normal_owners(model)
    assert (owners >= 0).all() and (owners < len(model.vertices)).all()
    first = faces[0, 0]
    assert owners[first[2] % len(model.normals)] == first[0] % len(model.vertices)
    # a normal no corner references is owned by nobody and keeps its value
    model.normals = np.concatenate([np.asarray(model.normals), [[0.0, 0.0, 1.0]]]).astype(np.float32)
    wrapped = faces.copy()                                         # (indices from the end would name other normals now: wrap first)
    wrapped[..., 2] = np.where(faces[..., 2] < 0, faces[..., 2] + len(model.normals) - 1, faces[..., 2])
    model._faces = wrapped
    owners = _pack.normal_owners(model)
    assert owners[-1] == -1 and (owners[:-1] >= 0).all()
    joints, weights, bones = skin_ref.rig(api, model, "bend")
    model.skin, model.bones = Skin(joints, weights, normals=True), bones
    followed = _pack.skinned_normals(model)
    assert followed[-1].tolist() == [0.0, 0.0, 1.0]
    assert np.array_equal(followed.view(np.uint64), skin_ref.skinned_normals(model, joints, weights, bones).view(np.uint64))


# ---------------------------------------------------------------------------- the packed scene
def _same_packed(a, b):
    assert len(a.models) == len(b.models) and len(a.textures) == len(b.textures)
    for k, (x, y) in enumerate(zip(a.models, b.models)):
        assert x.vertices.dtype == y.vertices.dtype and np.array_equal(x.vertices.view(np.uint64), y.vertices.view(np.uint64)), k
        assert x.vertices_are_f32 == y.vertices_are_f32 and np.array_equal(x.faces, y.faces), k
        for name in ("uv", "normals", "edge_ids"):
            p, q = getattr(x, name), getattr(y, name)
            assert (p is None and q is None) or (p.dtype == q.dtype and np.array_equal(p.view(np.uint32), q.view(np.uint32))), (k, name)
        assert (x.clip, x.depth_test, len(x.materials)) == (y.clip, y.depth_test, len(y.materials))
    for s, t in zip(a.textures, b.textures):
        assert np.array_equal(s, t)


@pytest.mark.parametrize("normals", [False, True], ids=["vertices", "normals"])
@pytest.mark.parametrize("recipe, name", [("torus_spot", "bend"), ("kat_house", "edge64"), ("cube_outward", "twist"),
                                          ("welded", "edge1"), ("diablo_floor", "single")])
def test_packed_scene_of_a_skinned_model_is_the_twins(api, oracle_mod, recipe, name, normals):
    """``pack_scene`` -- what the oracle renders -- of a skinned scene equals that of its twin array for array, and the
    oracle's renders of the two are equal."""
    from py_numpy_renderer_amd._pack import pack_scene
    scene, index = skin_ref.build(api, recipe)
    plain = pack_scene(scene)
    skin_ref.apply(api, scene, {index: name}, normals=normals)
    other = skin_ref.twin(api, recipe, name, normals=normals)
    got, want = pack_scene(scene), pack_scene(other)
    _same_packed(got, want)
    assert not got.models[index].vertices_are_f32
    assert not np.array_equal(got.models[index].vertices, plain.models[index].vertices)
    if got.models[index].normals is not None:
        assert np.array_equal(got.models[index].normals, plain.models[index].normals) != normals
    a, b = oracle_mod.render(scene, shadows=True), oracle_mod.render(other, shadows=True)
    assert np.array_equal(a.out, b.out) and np.array_equal(a.z.view(np.uint64), b.z.view(np.uint64))
    assert np.array_equal(a.winner, b.winner) and np.array_equal(a.stencil, b.stencil)
    assert np.array_equal(a.frame.view(np.uint32), b.frame.view(np.uint32)) and a.stats == b.stats
    assert a.stats["n_quads"] > 0 and len(a.silhouette) > 0


def test_skin_then_pose_with_pose_normals_packs_as_the_composed_twin(api):
    from py_numpy_renderer_amd._pack import pack_scene
    import pose_ref
    matrix = pose_ref.matrices(api)["product"]
    scene, index = skin_ref.build(api, "torus_spot")
    skin_ref.apply(api, scene, {index: "bend"}, normals=True)
    scene.models[index].pose_normals = True
    scene.models[index].pose = matrix
    other = skin_ref.twin(api, "torus_spot", "bend", normals=True, poses={index: matrix}, pose_normals=True)
    _same_packed(pack_scene(scene), pack_scene(other))
    scene.models[index].pose_normals = False
    other = skin_ref.twin(api, "torus_spot", "bend", normals=True, poses={index: matrix})
    _same_packed(pack_scene(scene), pack_scene(other))


def test_a_skin_without_bones_packs_exactly_as_no_skin(api):
    from py_numpy_renderer_amd._native import DeviceRenderer
    from py_numpy_renderer_amd._pack import pack_scene
    scene, index = skin_ref.build(api, "torus_spot")
    plain, sig = pack_scene(scene), DeviceRenderer._scene_signature(scene)
    joints, weights, bones = skin_ref.rig(api, scene.models[index], "bend")
    scene.models[index].skin = Skin(joints, weights, normals=True)
    _same_packed(pack_scene(scene), plain)
    assert pack_scene(scene).models[index].vertices_are_f32 and DeviceRenderer._scene_signature(scene) == sig
    scene.models[index].bones = bones                              # neither attribute is part of the scene's signature
    assert DeviceRenderer._scene_signature(scene) == sig
    assert not pack_scene(scene).models[index].vertices_are_f32
    scene.models[index].bones = None
    _same_packed(pack_scene(scene), plain)
    assert np.asarray(scene.models[index].vertices).dtype == np.float32


# ---------------------------------------------------------------------------- the C ABI
def _scene_with_a_quad(lib):
    from py_numpy_renderer_amd import _native
    handle = lib.mr_scene_create()
    assert handle
    verts = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1], [1, 1, 0, 1]], dtype=np.float64)
    normals = np.array([[0, 0, 1], [0, 0, 1]], dtype=np.float32)
    faces = np.array([[[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 1, 0]], [[1, 0, 0, 0], [3, 0, 1, 0], [2, 0, 1, 0]]], dtype=np.int32)
    mats = (_native.MaterialDesc * 1)()
    mats[0].tex_kd = mats[0].tex_norm = mats[0].tex_ks = -1
    d = _native.ModelDesc()
    d.vertices, d.normals, d.faces, d.materials = verts.ctypes.data, normals.ctypes.data, faces.ctypes.data, mats
    d.n_vertices, d.n_normals, d.n_faces, d.n_materials, d.vertices_are_f32, d.clip, d.depth_test = 4, 2, 2, 1, 1, 1, 1
    assert lib.mr_scene_add_model(handle, C.byref(d)) == 0
    return handle


def test_the_c_abi_validates_skins_and_bones(lib):
    handle = _scene_with_a_quad(lib)
    joints = np.array([[0, 1, 2, 2]] * 4, dtype=np.int32)
    weights = np.tile([0.25, 0.25, 0.25, 0.25], (4, 1))
    owners = np.array([0, 3], dtype=np.int32)
    bones = np.stack([np.eye(4)] * 3)
    ptr = lambda a: a.ctypes.data
    skin = lambda j=joints, w=weights, b=3, o=owners, model=0: lib.mr_scene_set_model_skin(
        handle, model, ptr(j), None if w is None else ptr(w), b, None if o is None else ptr(o))
    assert lib.mr_scene_set_model_bones(handle, 0, ptr(bones), 3) == MR_E_INVALID and b"skin" in lib.mr_last_error()
    assert skin(model=1) == MR_E_INVALID and skin(model=-1) == MR_E_INVALID
    assert skin(w=None) == MR_E_INVALID and skin(b=0) == MR_E_INVALID
    assert skin(b=2) == MR_E_INVALID and b"joint" in lib.mr_last_error()              # joint 2 of 2 bones
    assert skin(j=joints - 1) == MR_E_INVALID
    bad = weights.copy()
    bad[3, 3] = np.nan
    assert skin(w=bad) == MR_E_INVALID and b"finite" in lib.mr_last_error()
    assert skin(o=np.array([0, 4], dtype=np.int32)) == MR_E_INVALID and b"owner" in lib.mr_last_error()
    assert skin(o=np.array([-2, 0], dtype=np.int32)) == MR_E_INVALID
    assert lib.mr_scene_set_model_bones(handle, 0, ptr(bones), 3) == MR_E_INVALID     # nothing was kept of the refused skins
    assert skin() == 0 and skin(o=None) == 0 and skin(o=np.array([-1, 2], dtype=np.int32)) == 0
    out = (C.c_int32 * 4)()
    assert lib.mr_debug_skin(handle, out) == 0 and list(out) == [0, 0, 0, 0]          # a skin alone: nothing moves
    assert lib.mr_scene_set_model_bones(handle, 0, ptr(bones), 2) == MR_E_INVALID and b"number of bones" in lib.mr_last_error()
    assert lib.mr_scene_set_model_bones(handle, 1, ptr(bones), 3) == MR_E_INVALID
    bad = bones.copy()
    bad[2, 3, 3] = np.inf
    assert lib.mr_scene_set_model_bones(handle, 0, ptr(bad), 3) == MR_E_INVALID and b"finite" in lib.mr_last_error()
    assert lib.mr_scene_set_model_bones(handle, 0, ptr(bones), 3) == 0
    assert lib.mr_debug_skin(handle, out) == 0 and out[0] == 1
    assert lib.mr_scene_set_model_bones(handle, 0, None, 0) == 0                      # the rest position
    assert lib.mr_debug_skin(handle, out) == 0 and out[0] == 0
    assert lib.mr_scene_set_model_bones(handle, 0, ptr(bones), 3) == 0
    assert lib.mr_scene_set_model_skin(handle, 0, None, None, 0, None) == 0           # the skin goes, and its bones with it
    assert lib.mr_debug_skin(handle, out) == 0 and out[0] == 0
    assert lib.mr_scene_set_model_bones(handle, 0, ptr(bones), 3) == MR_E_INVALID
    times = (C.c_float * 2)()
    assert lib.mr_debug_skin_times(handle, times) == MR_E_INVALID and b"no pass" in lib.mr_last_error()
    assert lib.mr_debug_skin(handle, None) == MR_E_INVALID and lib.mr_debug_skin(None, out) == MR_E_INVALID
    lib.mr_scene_destroy(handle)
