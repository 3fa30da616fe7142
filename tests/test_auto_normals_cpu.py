"""``Model.auto_normals`` (``mr_scene_set_model_auto_normals``): what can be checked without a GPU -- the setter and its
refusals, the rebuilt normals against the contract restated in ``auto_normals_ref`` (pure Python) and against the
library's host helper (which builds and walks the sliced face lists the device walks), the precedence over the three
other ways a moved model's normals change, the keep cases, the packed scene the oracle renders, and the C ABI's
argument validation on the built library."""
import ctypes as C

import numpy as np
import pytest

import auto_normals_ref as ref
import morph_ref
import pose_ref
import skin_ref
from py_numpy_renderer_amd import _pack

MR_E_INVALID = -1
CASES = [(mesh, mode) for mesh in ref.MESHES for mode in ref.MODES] + [("torus_spot", ref.MIRROR)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_native()
    from py_numpy_renderer_amd import _native
    return _native.load_library()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _moved(api, mesh, mode, **kw):
    scene, index = ref.build(api, mesh)
    ref.apply(api, scene.models[index], mode, **kw)
    return scene, scene.models[index]


# ---------------------------------------------------------------------------- the Python API
def test_the_flag_defaults_to_false_and_is_validated_like_pose_normals(api):
    scene, index = ref.build(api, "cube_outward")
    model = scene.models[index]
    assert model.auto_normals is False
    for value, want in ((True, True), (np.bool_(False), False), (1, True), (0, False), (np.int32(1), True)):
        model.auto_normals = value
        assert model.auto_normals is want
    model.auto_normals = True
    for value in (2, -1, 1.0, "yes", None, [True], np.ones(1)):
        with pytest.raises(TypeError, match="auto_normals"):
            model.auto_normals = value
        assert model.auto_normals is True                          # (the attribute keeps its value)


def test_flag_off_at_rest_or_without_normals_is_todays_model(api):
    """``posed_normals`` returns the arrays it returns today -- the very objects -- and ``auto_normals`` ``None``."""
    scene, index = ref.build(api, "torus_spot")
    model = scene.models[index]
    model.auto_normals = True                                      # at rest
    assert _pack.auto_normals(model) is None and not _pack.auto_normals_active(model)
    assert _pack.posed_normals(model) is model.normals
    ref.apply(api, model, "all", flag=False, skin_normals=True, pose_normals=True)     # moved, the flag off
    assert _pack.auto_normals(model) is None
    want = np.asarray(skin_ref.twin(api, "torus_spot", "bend", normals=True, poses={index: model.pose}, pose_normals=True).models[index].normals)
    model.morph = None                                             # (skin_ref's twin knows no morph)
    assert np.array_equal(_bits(_pack.posed_normals(model)), _bits(want))
    bare, _ = pose_ref.build(api, (ref.pose_normals_ref.RECIPES["tetra_bare"][0], 0))
    tetra = bare.models[0]
    tetra.auto_normals, tetra.pose = True, np.eye(4)               # moved, but no normals
    assert tetra.normals is None and _pack.auto_normals(tetra) is None and _pack.posed_normals(tetra) is None
    assert _pack.pack_scene(bare).models[0].normals is None


# ---------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("mesh, mode", CASES)
def test_python_chain_and_host_helper_equal_the_reference_bit_for_bit(api, lib, mesh, mode):
    """``_pack.auto_normals(native=False)`` (the pure-Python loop) and the default path (``mr_host_auto_normals``: the
    sliced lists, walked in the kernel's order) against the hand-written chain of ``auto_normals_ref`` on every mesh."""
    verts, want, kept = ref.arrays(mesh, mode)
    scene, model = _moved(api, mesh, mode)
    assert np.array_equal(_bits(np.asarray(_pack.posed_vertices(model)).astype(np.float64)), _bits(verts)), "V"
    slow = _pack.auto_normals(model, native=False)
    assert slow.dtype == np.float32 and slow.shape == np.asarray(model.normals).shape
    assert np.array_equal(_bits(slow), _bits(want)), "pure Python"
    assert _pack._fast_auto(), "the library's helper is not in use"
    fast = _pack.auto_normals(model)
    assert np.array_equal(_bits(fast), _bits(want)), "mr_host_auto_normals"
    assert np.array_equal(_bits(_pack.posed_normals(model)), _bits(want))
    authored = np.ascontiguousarray(model.normals, dtype=np.float32)
    for q in kept:
        assert np.array_equal(_bits(want[q]), _bits(authored[q]))
    changed = np.flatnonzero((_bits(want) != _bits(authored)).any(axis=1))
    assert len(changed) + len(kept) >= len(want) - 2 and len(changed) > 0      # (a rebuilt normal may hit its authored bits by chance)
    lengths = np.linalg.norm(want[changed].astype(np.float64), axis=1)
    assert np.abs(lengths - 1.0).max() < 1e-6
    assert np.asarray(model.normals).dtype == np.float32 and not np.shares_memory(fast, model.normals)


def test_the_fan_holds_what_it_is_for(api):
    """130 normals; a hub named by 200 faces, by all three corners of 76 of them; rim normals named by one or two; a
    normal named by two corners of one face, one named by none, and one whose two faces cancel exactly."""
    scene, index = ref.build(api, "fan")
    model = scene.models[index]
    lists = ref.face_lists(model)
    assert len(model.normals) == ref.FAN_NORMALS and len(model._faces) == ref.FAN_FACES
    assert lists[0] == list(range(200))
    assert {len(l) for l in lists[1:126]} == {1, 2} and len(lists[63]) == 2 and len(lists[64]) == 2
    assert lists[ref.FAN_TWICE] == [200] and lists[129] == [200] and lists[ref.FAN_UNNAMED] == [] and lists[ref.FAN_CANCELLED] == [201, 202]
    assert ref.wrapped(model)[1][200].count(ref.FAN_TWICE) == 2 and ref.wrapped(model)[1][150] == [0, 0, 0]
    for mode in ref.MODES:
        assert ref.arrays("fan", mode)[2] == (ref.FAN_UNNAMED, ref.FAN_CANCELLED), mode
    tiny = ref.build(api, "tiny")[0].models[0]
    assert ref.face_lists(tiny) == [[0]] and ref.arrays("tiny", "pose")[2] == ()


def test_the_three_keep_cases(api, lib):
    """An empty list, a sum of length 0 (the fan's cancelled pair, and a face without area), and a sum or a length that
    is not finite keep ``float32(normals[q])``; the library's helper agrees with the Python loop on each."""
    scene, index = ref.build(api, "fan")
    model = scene.models[index]
    huge = np.asarray(model.vertices).astype(np.float64)
    huge[203:206, :3] *= 1e100                                     # face 200: a finite sum whose squared length is not
    huge[1] = huge[0]                                              # face 0 has no area: normal 1 sums to +0
    huge[100, 0] = 1e308                                           # faces 98 and 99: products overflow, the hub's sum is not finite
    huge[101, 1] = -1e308
    model.vertices = huge
    model.pose, model.auto_normals = np.eye(4), True
    slow, fast = _pack.auto_normals(model, native=False), _pack.auto_normals(model)
    assert np.array_equal(_bits(slow), _bits(fast))
    want, kept = ref.chain(model, _pack.posed_vertices(model))
    assert np.array_equal(_bits(slow), _bits(want))
    assert {0, 1, ref.FAN_TWICE, ref.FAN_UNNAMED, ref.FAN_CANCELLED, 129} <= set(kept)
    authored = np.ascontiguousarray(model.normals, dtype=np.float32)
    assert np.array_equal(_bits(slow[kept]), _bits(authored[kept])) and np.isfinite(slow).all()
    assert 30 not in kept and not np.array_equal(_bits(slow[30]), _bits(authored[30]))


def test_a_minus_zero_component_survives_the_first_face(api):
    """``acc = cr(L[0])``, not ``0 + cr(L[0])``: a component of -0.0 stays -0.0 through the division."""
    scene, index = ref.build(api, "tiny")
    model = scene.models[index]
    model.vertices = np.array([[0, 0, 0, 1], [0, 0, 1, 1], [1, -1, 0, 1]], dtype=np.float64)    # z of the product: 0 * -1 - 0 * 1 = -0.0
    model.pose, model.auto_normals = np.eye(4), True
    want, _ = ref.chain(model, _pack.posed_vertices(model))
    assert np.signbit(want[0, 2]) and want[0, 2] == 0.0 and want[0, 0] > 0.7
    for native in (False, None):
        assert np.array_equal(_bits(_pack.auto_normals(model, native=native)), _bits(want))


# ---------------------------------------------------------------------------- precedence
def test_auto_normals_supersede_normal_targets_skin_normals_and_pose_normals(api):
    """With ``normal_targets``, ``Skin(normals=True)`` and ``pose_normals`` all set, the flagged model's normals are those
    of the final geometry alone -- the arrays of the model that has none of the three -- and differ from what the three
    give without the flag."""
    scene, index = ref.build(api, "torus_spot")
    model = scene.models[index]
    normal_targets = morph_ref.shape(model, "normals")[1]
    ref.apply(api, model, "all", skin_normals=True, normal_targets=normal_targets, pose_normals=True)
    assert model.morph.normal_targets is not None and model.skin.normals and model.pose_normals
    _, want, _ = ref.arrays("torus_spot", "all")
    assert np.array_equal(_bits(_pack.posed_normals(model)), _bits(want))
    assert np.array_equal(_bits(_pack.pack_scene(scene).models[index].normals), _bits(want))
    model.auto_normals = False
    without = _pack.posed_normals(model)
    assert not np.array_equal(_bits(without), _bits(want))
    for drop in ("pose_normals", "skin", "morph"):                 # each of the three alone is superseded too
        other, m = _moved(api, "torus_spot", "all", skin_normals=drop == "skin", pose_normals=drop == "pose_normals",
                          normal_targets=normal_targets if drop == "morph" else None)
        assert np.array_equal(_bits(_pack.posed_normals(m)), _bits(want)), drop
        m.auto_normals = False
        assert not np.array_equal(_bits(_pack.posed_normals(m)), _bits(m.normals)), drop


def test_a_mirroring_pose_flips_the_normals_with_the_faces(api):
    scene, index = ref.build(api, "cube_outward")
    model = scene.models[index]
    model.auto_normals, model.pose = True, np.eye(4)
    upright = _pack.auto_normals(model)
    model.pose = np.diag([-1.0, 1.0, 1.0, 1.0])
    mirrored = _pack.auto_normals(model)
    # (x -> -x maps the cross product (x, y, z) to (x, -y, -z): the face normals of the light-facing test)
    assert np.array_equal(mirrored, upright * np.array([1, -1, -1], dtype=np.float32))         # (every step is odd in x; values, not zero signs)
    authored = np.asarray(model.normals, dtype=np.float64)
    side = np.einsum("ij,ij->i", upright.astype(np.float64), authored)         # the cube's authored normals lie on one side of its winding
    assert (np.abs(side) > 0.99).all() and len(set(np.sign(side))) == 1
    flipped = np.einsum("ij,ij->i", mirrored.astype(np.float64), authored * [-1, 1, 1])
    assert np.array_equal(flipped, -side)                          # ... and the mirrored cube's, mirrored, on the other


def test_identity_pose_rebuilds_a_mesh_at_rest(api):
    scene, index = ref.build(api, "fan")
    model = scene.models[index]
    model.auto_normals = True
    assert _pack.auto_normals(model) is None
    model.pose = np.eye(4)
    want, kept = ref.chain(model, np.asarray(model.vertices).astype(np.float64))
    assert np.array_equal(_bits(_pack.auto_normals(model)), _bits(want)) and kept == [ref.FAN_UNNAMED, ref.FAN_CANCELLED]
    assert not np.array_equal(_bits(want), _bits(np.asarray(model.normals, dtype=np.float32)))


# ---------------------------------------------------------------------------- the packed scene and the oracle
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


@pytest.mark.parametrize("mesh, mode", [("fan", "all"), ("tiny", "pose"), ("kat_house", "morph"), ("cube_outward", "skin"),
                                        ("torus_spot", "all"), ("diablo_floor", "pose")])
def test_packed_scene_and_oracle_of_a_flagged_scene_are_the_twins(api, oracle_mod, mesh, mode):
    scene, model = _moved(api, mesh, mode)
    other = ref.twin(api, mesh, mode)
    _same_packed(_pack.pack_scene(scene), _pack.pack_scene(other))
    a, b = oracle_mod.render(scene, shadows=True), oracle_mod.render(other, shadows=True)
    assert np.array_equal(a.out, b.out) and np.array_equal(a.z.view(np.uint64), b.z.view(np.uint64))
    assert np.array_equal(a.winner, b.winner) and np.array_equal(a.stencil, b.stencil)
    assert np.array_equal(a.frame.view(np.uint32), b.frame.view(np.uint32)) and a.stats == b.stats
    model.auto_normals = False
    c = oracle_mod.render(scene, shadows=True)
    assert np.array_equal(c.z.view(np.uint64), a.z.view(np.uint64)) and np.array_equal(c.stencil, a.stencil)     # normals move no geometry
    assert not np.array_equal(c.frame.view(np.uint32), a.frame.view(np.uint32)), "the flag changed no pixel"


def test_an_object_space_map_is_still_rebaked_under_pose_normals(api):
    """``pose_normals`` keeps its texel part: the packed maps are those of the twin whose maps were re-baked with G, the
    vertex normals those of the geometry."""
    recipe = ref.OBJECT_MAP
    matrix = pose_ref.matrices(api)["rotation"]
    scene, index = pose_ref.build(api, recipe)
    model = scene.models[index]
    plain = _pack.pack_scene(scene)
    ref.apply(api, model, "pose", pose_normals=True)
    other = ref.twin(api, recipe, "pose", pose_normals=True)
    got = _pack.pack_scene(scene)
    _same_packed(got, _pack.pack_scene(other))
    assert any(not np.array_equal(s, t) for s, t in zip(got.textures, plain.textures)), "no map was re-baked"
    follow = ref.pose_normals_ref.twin(api, recipe, matrix)         # (pose_normals without the flag: the same maps, other normals)
    assert not np.array_equal(_bits(got.models[index].normals), _bits(_pack.pack_scene(follow).models[index].normals))


def test_the_flag_is_no_part_of_the_scene_signature(api):
    from py_numpy_renderer_amd._native import DeviceRenderer
    scene, index = ref.build(api, "torus_spot")
    sig = DeviceRenderer._scene_signature(scene)
    scene.models[index].auto_normals = True
    scene.models[index].pose = np.eye(4)
    assert _pack.auto_normals_active(scene.models[index]) and _pack.auto_normals(scene.models[index]) is not None
    assert DeviceRenderer._scene_signature(scene) == sig
    assert np.asarray(scene.models[index].normals).dtype == np.float32


# ---------------------------------------------------------------------------- the C ABI
def _scene_with_a_quad(lib, normals=True):
    from py_numpy_renderer_amd import _native
    handle = lib.mr_scene_create()
    assert handle
    verts = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1], [1, 1, 0, 1]], dtype=np.float64)
    vn = np.array([[0, 0, 1], [0, 0, 1]], dtype=np.float32)
    faces = np.array([[[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 1, 0]], [[1, 0, 0, 0], [3, 0, 1, 0], [2, 0, 1, 0]]], dtype=np.int32)
    mats = (_native.MaterialDesc * 1)()
    mats[0].tex_kd = mats[0].tex_norm = mats[0].tex_ks = -1
    d = _native.ModelDesc()
    d.vertices, d.normals, d.faces, d.materials = verts.ctypes.data, vn.ctypes.data if normals else None, faces.ctypes.data, mats
    d.n_vertices, d.n_normals, d.n_faces, d.n_materials, d.vertices_are_f32, d.clip, d.depth_test = 4, 2 if normals else 0, 2, 1, 1, 1, 1
    assert lib.mr_scene_add_model(handle, C.byref(d)) == 0
    return handle


def test_the_c_abi_validates_the_flag_and_the_host_helper(lib):
    handle = _scene_with_a_quad(lib)
    flag = lib.mr_scene_set_model_auto_normals
    assert flag(None, 0, 1) == MR_E_INVALID
    assert flag(handle, 1, 1) == MR_E_INVALID and flag(handle, -1, 1) == MR_E_INVALID and b"range" in lib.mr_last_error()
    assert flag(handle, 0, 2) == MR_E_INVALID and flag(handle, 0, -1) == MR_E_INVALID
    assert flag(handle, 0, 1) == 0 and flag(handle, 0, 1) == 0 and flag(handle, 0, 0) == 0 and flag(handle, 0, 1) == 0
    out = (C.c_int32 * 4)()
    assert lib.mr_debug_auto_normals(handle, out) == 0 and list(out) == [0, 0, 0, 0]      # the flag alone: no pass, no lists on the device
    assert lib.mr_debug_auto_normals(handle, None) == MR_E_INVALID and lib.mr_debug_auto_normals(None, out) == MR_E_INVALID
    times = (C.c_float * 1)()
    assert lib.mr_debug_auto_normals_times(handle, times) == MR_E_INVALID and b"no pass" in lib.mr_last_error()
    lib.mr_scene_destroy(handle)
    bare = _scene_with_a_quad(lib, normals=False)
    assert flag(bare, 0, 1) == 0                                   # (a model without normals: the flag changes nothing)
    lib.mr_scene_destroy(bare)
    # the host helper: indices out of range, NULL arguments
    verts = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1]], dtype=np.float64)
    rows = np.array([[0, 0, 0, 0, 1, 0, 1, 0, 2, 0, 0, 0]], dtype=np.int32)
    vn = np.array([[1, 0, 0], [0, 1, 0], [0.6, 0, 0.8]], dtype=np.float32)
    res = np.zeros_like(vn)
    helper = lambda v=verts, r=rows, n=vn, o=res, nv=3, nn=3: lib.mr_host_auto_normals(
        None if v is None else v.ctypes.data, nv, None if r is None else r.ctypes.data, len(rows), None if n is None else n.ctypes.data, nn,
        None if o is None else o.ctypes.data)
    assert helper() == 0
    assert res.tolist() == [[0, 0, 1], [0, 0, 1], [np.float32(0.6), 0, np.float32(0.8)]]       # normal 2: no corner, kept
    assert helper(nv=2) == MR_E_INVALID and b"vertex index" in lib.mr_last_error()
    assert helper(nn=1) == MR_E_INVALID and b"normal index" in lib.mr_last_error()
    bad = rows.copy()
    bad[0, 8] = -1
    assert helper(r=bad) == MR_E_INVALID
    assert helper(v=None) == MR_E_INVALID and helper(n=None) == MR_E_INVALID and helper(o=None) == MR_E_INVALID
    assert helper(r=None) == MR_E_INVALID
