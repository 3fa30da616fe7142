"""``Model.morph`` / ``Model.morph_weights`` (``mr_scene_set_model_morph``, ``mr_scene_set_model_morph_weights``): what can
be checked without a GPU -- the setters and their refusals, the morphed arrays against the contract restated in
``morph_ref`` and against the library's host helper (which builds and walks the sliced lists the device walks), the
packed scene the oracle renders, and the C ABI's argument validation on the built library."""
import ctypes as C

import numpy as np
import pytest

import morph_ref
import pose_ref
import scenes
import skin_ref
from py_numpy_renderer_amd import Morph

MR_E_INVALID = -1
ALL_SHAPES = morph_ref.SHAPE_NAMES + ("normals",)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_native()
    from py_numpy_renderer_amd import _native
    return _native.load_library()


def _cube(api):
    return scenes.cube_small(api).models[0]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---------------------------------------------------------------------------- the Python API
def test_morph_and_weights_default_to_none_and_store_read_only_copies(api):
    cube = _cube(api)
    n = len(cube.vertices)
    assert cube.morph is None and cube.morph_weights is None
    index, delta = np.array([0.0, 2.0], dtype=np.float32), np.ones((2, 3), dtype=np.float32)     # integral floats are integers
    dense = np.zeros((n, 3))
    morph = Morph([(index, delta), dense, ([], np.zeros((0, 3)))], normal_targets=[None, ([1], [[0, 0, 1]]), None])
    assert len(morph.targets) == 3 and len(morph.normal_targets) == 3
    for i, d in morph.targets + morph.normal_targets:
        assert i.dtype == np.int32 and d.dtype == np.float64 and d.shape == (len(i), 3)
        assert not i.flags.writeable and not d.flags.writeable
    assert morph.targets[1][0].tolist() == list(range(n)) and len(morph.targets[2][0]) == 0
    assert len(morph.normal_targets[0][0]) == 0 and morph.normal_targets[1][0].tolist() == [1]
    delta[0, 0] = 9                                                # copies: the caller's arrays are not looked at again
    assert morph.targets[0][1][0, 0] == 1.0
    with pytest.raises(AttributeError):
        morph.targets = ()
    cube.morph = morph
    assert cube.morph is morph and cube.morph_weights is None
    weights = np.array([0.5, -2.0, 3.0], dtype=np.float32)         # not clamped
    cube.morph_weights = weights
    assert cube.morph_weights.dtype == np.float64 and cube.morph_weights.tolist() == [0.5, -2.0, 3.0]
    weights[0] = 7
    assert cube.morph_weights[0] == 0.5
    with pytest.raises(ValueError):
        cube.morph_weights[0] = 1.0
    cube.morph_weights = None
    assert cube.morph_weights is None and cube.morph is morph
    cube.morph_weights = [1, 2, 3]
    cube.morph = None                                              # no morph, no weights
    assert cube.morph is None and cube.morph_weights is None
    import py_numpy_renderer_amd as pkg
    assert "Morph" in pkg.__all__ and pkg.Morph is Morph


@pytest.mark.parametrize("targets, normal_targets, error", [
    ([], None, ValueError),                                                    # t >= 1
    ([np.zeros((8, 2))], None, ValueError),                                    # shapes
    ([np.zeros(8)], None, ValueError),
    ([([0, 1], np.zeros((3, 3)))], None, ValueError),
    ([([0, 1], np.zeros((2, 4)))], None, ValueError),
    ([([[0, 1]], np.zeros((2, 3)))], None, ValueError),
    ([([0.5], np.zeros((1, 3)))], None, ValueError),                           # indices that are not integral
    ([([np.nan], np.zeros((1, 3)))], None, ValueError),
    ([([-1], np.zeros((1, 3)))], None, ValueError),                            # ... or negative
    ([([3, 1, 3], np.zeros((3, 3)))], None, ValueError),                       # ... or named twice in one target
    ([([0], [[0, np.nan, 0]])], None, ValueError),                             # deltas that are not finite
    ([np.full((8, 3), np.inf)], None, ValueError),
    ("targets", None, TypeError),
    (7, None, TypeError),
    (["target"], None, TypeError),
    ([object()], None, TypeError),
    ([np.zeros((8, 3))], [], ValueError),                                      # one normal entry per target
    ([np.zeros((8, 3))], [None, None], ValueError),
    ([np.zeros((8, 3))], "normals", TypeError),
    ([np.zeros((8, 3))], [([0, 0], np.zeros((2, 3)))], ValueError),
])
def test_morph_rejects(targets, normal_targets, error):
    with pytest.raises(error):
        Morph(targets, normal_targets)


def test_morph_setter_rejects_and_keeps_the_old_value(api):
    cube = _cube(api)
    n, nn = len(cube.vertices), len(cube.normals)
    keep = Morph([np.zeros((n, 3)), ([0], [[1, 0, 0]])])
    cube.morph = keep
    with pytest.raises(TypeError):
        cube.morph = [np.zeros((n, 3))]                            # a Morph, not its parts
    with pytest.raises(ValueError, match="vertex"):
        cube.morph = Morph([([n], [[1, 0, 0]])])                   # an index past the last vertex
    with pytest.raises(ValueError, match="vertex"):
        cube.morph = Morph([np.zeros((n + 1, 3))])
    with pytest.raises(ValueError, match="normal"):
        cube.morph = Morph([np.zeros((n, 3))], [([nn], [[0, 0, 1]])])
    assert cube.morph is keep
    cube.morph_weights = [0.5, 0.5]
    with pytest.raises(ValueError, match="targets"):
        cube.morph = Morph([np.zeros((n, 3))])                     # one target, two weights: this assignment completes the pair
    assert cube.morph is keep and len(cube.morph_weights) == 2
    bare = _cube(api)
    bare.normals = None
    with pytest.raises(ValueError, match="normals"):
        bare.morph = Morph([np.zeros((n, 3))], [None])
    assert bare.morph is None


@pytest.mark.parametrize("bad, error", [
    (np.zeros((2, 1)), ValueError), (1.0, ValueError), (np.zeros(0), ValueError), ([np.nan, 0.0], ValueError),
    ([0.0, np.inf], ValueError), ([0.0], ValueError), ([0.0, 1.0, 2.0], ValueError),
    ("ww", TypeError), (b"01", TypeError), (object(), TypeError), (["a", "b"], ValueError),
])
def test_weights_setter_rejects_and_keeps_the_old_value(api, bad, error):
    cube = _cube(api)
    cube.morph = Morph([np.zeros((len(cube.vertices), 3))] * 2)
    cube.morph_weights = [0.25, 0.75]
    with pytest.raises(error):
        cube.morph_weights = bad
    assert cube.morph_weights.tolist() == [0.25, 0.75]


def test_weights_need_a_morph(api):
    cube = _cube(api)
    with pytest.raises(ValueError, match="morph"):
        cube.morph_weights = [1.0]
    assert cube.morph_weights is None


def test_a_morph_that_no_longer_fits_its_model_is_refused_at_render(api):
    from py_numpy_renderer_amd import _native, _pack
    scene = scenes.cube_small(api)
    cube = scene.models[0]
    n = len(cube.vertices)
    cube.morph = Morph([([n - 1], [[0.1, 0, 0]])])
    cube.morph_weights = [1.0]
    cube.vertices = np.asarray(cube.vertices)[:n - 1]
    with pytest.raises(ValueError, match="reaches"):
        _pack.pack_scene(scene)

    class NoDevice(_native.DeviceRenderer):                        # the check comes before any device work
        def __init__(self):
            self._signature = None
    with pytest.raises(ValueError, match="reaches"):
        NoDevice().sync_scene(scene)
    cube.morph_weights = None                                      # without weights the morph is not looked at
    _pack.active_morph(cube)


# ---------------------------------------------------------------------------- the arrays
@pytest.mark.parametrize("recipe", ["cube_outward", "kat_house", "diablo_floor"])
@pytest.mark.parametrize("name", ALL_SHAPES)
def test_the_host_helper_equals_the_pure_python_chain(lib, api, recipe, name):
    """``morphed_vertices`` / ``morphed_normals`` through ``mr_host_morph_chain`` (sliced lists, the kernel's walk)
    against the pure-Python chain and against ``morph_ref``'s restatement, bit for bit, over whole models."""
    from py_numpy_renderer_amd import _pack
    assert _pack._fast_morph(), "the library is built: _pack must use its helper"
    scene, index = morph_ref.build(api, recipe)
    model = scene.models[index]
    assert model.normals is not None
    targets, normal_targets, weights = morph_ref.shape(model, name)
    model.morph, model.morph_weights = Morph(targets, normal_targets), weights
    fast, pure = _pack.morphed_vertices(model, native=True), _pack.morphed_vertices(model, native=False)
    want = morph_ref.morphed_vertices(model.vertices, targets, weights)
    assert fast.dtype == np.float64 and fast.shape == (len(model.vertices), 4)
    assert np.array_equal(_bits(fast), _bits(pure)) and np.array_equal(_bits(fast), _bits(want))
    assert not np.array_equal(fast, np.asarray(model.vertices, dtype=np.float64))
    assert np.array_equal(fast[:, 3], np.asarray(model.vertices, dtype=np.float64)[:, 3])
    if normal_targets is None:
        assert _pack.morphed_normals(model) is None
        return
    fast, pure = _pack.morphed_normals(model, native=True), _pack.morphed_normals(model, native=False)
    want = morph_ref.morphed_normals(model.normals, normal_targets, weights)
    assert fast.dtype == np.float32 and fast.shape == np.asarray(model.normals).shape
    assert np.array_equal(_bits(fast), _bits(pure)) and np.array_equal(_bits(fast), _bits(want))
    assert not np.array_equal(fast, np.asarray(model.normals, dtype=np.float32))


def test_the_shapes_hold_what_they_promise(api):
    """On the torus: ``bands`` lists vertices 0, 1, 2 and 3 times; ``slices`` touches the seams, has an empty target, a
    lone vertex in its slice and a hub every other target lists; ``edge257`` lists every vertex at most three times."""
    scene, index = morph_ref.build(api, "torus_spot")
    model = scene.models[index]
    n = len(model.vertices)
    assert n > 517 and n % 64 != 0
    listed = lambda targets: np.bincount(np.concatenate([np.asarray(i) for i, _ in targets]).astype(np.int64), minlength=n)
    targets, _, weights = morph_ref.shape(model, "bands")
    assert set(listed(targets).tolist()) == {0, 1, 2, 3} and 0.0 in weights.tolist() and 1.5 in weights.tolist()
    targets, _, _ = morph_ref.shape(model, "slices")
    count = listed(targets)
    assert all(count[i] > 0 for i in (0, 63, 64, 255, 256, n - 1)) and len(targets[1][0]) == 0
    assert count[401] == 1 and count[384:448].sum() == 1
    assert count[517] == 4 and count[448:512].sum() == 0 and count[576:640].sum() == 0 and count[512:576].sum() == 4
    for name in ("edge256", "edge257"):
        targets, _, weights = morph_ref.shape(model, name)
        count = listed(targets)
        assert len(targets) == morph_ref.N_TARGETS[name] == len(weights) and count.min() >= 2 and count.max() == 3
        assert weights[0] != 0 and weights[-1] != 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_host_morph_chain_on_hand_made_tables(lib, n):
    """``mr_host_morph_chain`` at the slice sizes: three targets -- everyone; every third vertex, listed backwards; the
    last vertex alone -- and one without entries, widths 4 and 3, against the chain spelled out here."""
    from py_numpy_renderer_amd import _fp
    rng = np.random.default_rng(n)
    sets = [np.arange(n), np.arange(0, n, 3)[::-1].copy(), np.array([n - 1]), np.zeros(0, dtype=np.int64)]
    first = np.zeros(5, dtype=np.int32)
    first[1:] = np.cumsum([len(s) for s in sets])
    index = np.concatenate(sets).astype(np.int32)
    delta = rng.standard_normal((len(index), 3))
    w = np.array([0.75, -1.25, 0.0, 3.0])
    for width in (4, 3):
        base = rng.standard_normal((n, width))
        want = base.copy()
        for k in range(4):
            for j in range(first[k], first[k + 1]):
                for c in range(3):
                    want[index[j], c] = _fp.fma(float(w[k]), float(delta[j, c]), float(want[index[j], c]))
        out = np.full_like(base, np.nan)
        rc = lib.mr_host_morph_chain(base.ctypes.data, n, width, 4, first.ctypes.data, index.ctypes.data, delta.ctypes.data,
                                     w.ctypes.data, out.ctypes.data)
        assert rc == 0 and np.array_equal(_bits(out), _bits(want)), (n, width)
    assert lib.mr_host_morph_chain(base.ctypes.data, n, 5, 4, first.ctypes.data, index.ctypes.data, delta.ctypes.data,
                                   w.ctypes.data, out.ctypes.data) == MR_E_INVALID
    twice = index.copy()
    if n > 1:
        twice[1] = twice[0]
        assert lib.mr_host_morph_chain(base.ctypes.data, n, 3, 4, first.ctypes.data, twice.ctypes.data, delta.ctypes.data,
                                       w.ctypes.data, out.ctypes.data) == MR_E_INVALID and b"twice" in lib.mr_last_error()


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


@pytest.mark.parametrize("recipe, name", [("torus_spot", "bands"), ("kat_house", "slices"), ("cube_outward", "dense2"),
                                          ("welded", "edge257"), ("diablo_floor", "normals")])
def test_packed_scene_and_oracle_of_a_morphed_model_are_the_twins(api, oracle_mod, recipe, name):
    """``pack_scene`` -- what the oracle renders -- of a morphed scene equals that of its twin array for array, and the
    oracle's renders of the two are equal."""
    from py_numpy_renderer_amd._pack import pack_scene
    scene, index = morph_ref.build(api, recipe)
    plain = pack_scene(scene)
    morph_ref.apply(api, scene, {index: name})
    other = morph_ref.twin(api, recipe, name)
    got, want = pack_scene(scene), pack_scene(other)
    _same_packed(got, want)
    assert not got.models[index].vertices_are_f32
    assert not np.array_equal(got.models[index].vertices, plain.models[index].vertices)
    if name == "normals":
        assert not np.array_equal(got.models[index].normals, plain.models[index].normals)
    a, b = oracle_mod.render(scene, shadows=True), oracle_mod.render(other, shadows=True)
    assert np.array_equal(a.out, b.out) and np.array_equal(a.z.view(np.uint64), b.z.view(np.uint64))
    assert np.array_equal(a.winner, b.winner) and np.array_equal(a.stencil, b.stencil)
    assert np.array_equal(a.frame.view(np.uint32), b.frame.view(np.uint32)) and a.stats == b.stats
    assert a.stats["n_quads"] > 0 and len(a.silhouette) > 0


def test_morph_then_skin_then_pose_packs_as_the_composed_twin(api):
    from py_numpy_renderer_amd._pack import pack_scene
    matrix = pose_ref.matrices(api)["product"]
    scene, index = morph_ref.build(api, "torus_spot")
    skin_ref.apply(api, scene, {index: "bend"}, normals=True)      # (the rig comes from the rest shape)
    morph_ref.apply(api, scene, {index: "normals"})
    scene.models[index].pose_normals = True
    scene.models[index].pose = matrix
    other = morph_ref.twin(api, "torus_spot", "normals", rigs={index: "bend"}, skin_normals=True, poses={index: matrix}, pose_normals=True)
    _same_packed(pack_scene(scene), pack_scene(other))
    scene.models[index].bones = None
    other = morph_ref.twin(api, "torus_spot", "normals", poses={index: matrix}, pose_normals=True)
    _same_packed(pack_scene(scene), pack_scene(other))


def test_a_morph_without_weights_packs_exactly_as_no_morph(api):
    from py_numpy_renderer_amd._native import DeviceRenderer
    from py_numpy_renderer_amd._pack import pack_scene
    scene, index = morph_ref.build(api, "torus_spot")
    model = scene.models[index]
    plain, sig = pack_scene(scene), DeviceRenderer._scene_signature(scene)
    targets, normal_targets, weights = morph_ref.shape(model, "normals")
    model.morph = Morph(targets, normal_targets)
    _same_packed(pack_scene(scene), plain)
    assert pack_scene(scene).models[index].vertices_are_f32 and DeviceRenderer._scene_signature(scene) == sig
    model.morph_weights = weights                                  # neither attribute is part of the scene's signature
    assert DeviceRenderer._scene_signature(scene) == sig
    assert not pack_scene(scene).models[index].vertices_are_f32
    model.morph_weights = None
    _same_packed(pack_scene(scene), plain)
    assert np.asarray(model.vertices).dtype == np.float32


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


def test_the_c_abi_validates_morphs_and_weights(lib):
    handle = _scene_with_a_quad(lib)
    first = np.array([0, 2, 2, 5], dtype=np.int32)                 # three targets, the second without entries
    index = np.array([0, 3, 3, 1, 2], dtype=np.int32)
    delta = np.arange(15, dtype=np.float64).reshape(5, 3) * 0.01
    nfirst, nindex, ndelta = np.array([0, 1, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.ones((2, 3))
    w = np.array([0.5, 1.0, -1.0])
    ptr = lambda a: None if a is None else a.ctypes.data
    morph = lambda t=3, f=first, i=index, d=delta, nf=None, ni=None, nd=None, model=0: lib.mr_scene_set_model_morph(
        handle, model, t, ptr(f), ptr(i), ptr(d), ptr(nf), ptr(ni), ptr(nd))
    weights = lambda a=w, t=3, model=0: lib.mr_scene_set_model_morph_weights(handle, model, ptr(a), t)
    assert weights() == MR_E_INVALID and b"morph" in lib.mr_last_error()
    assert morph(model=1) == MR_E_INVALID and morph(model=-1) == MR_E_INVALID
    assert morph(t=0) == MR_E_INVALID and morph(i=None) == MR_E_INVALID and morph(d=None) == MR_E_INVALID
    assert morph(f=np.array([1, 2, 2, 5], dtype=np.int32)) == MR_E_INVALID
    assert morph(f=np.array([0, 3, 2, 5], dtype=np.int32)) == MR_E_INVALID
    assert morph(i=np.array([0, 4, 3, 1, 2], dtype=np.int32)) == MR_E_INVALID and b"range" in lib.mr_last_error()
    assert morph(i=np.array([0, -1, 3, 1, 2], dtype=np.int32)) == MR_E_INVALID
    assert morph(i=np.array([0, 3, 3, 1, 3], dtype=np.int32)) == MR_E_INVALID and b"twice" in lib.mr_last_error()
    bad = delta.copy()
    bad[4, 2] = np.nan
    assert morph(d=bad) == MR_E_INVALID and b"finite" in lib.mr_last_error()
    assert morph(nf=nfirst, ni=np.array([2, 0], dtype=np.int32), nd=ndelta) == MR_E_INVALID     # normal 2 of 2
    assert weights() == MR_E_INVALID                               # nothing was kept of the refused morphs
    assert morph() == 0 and morph(nf=nfirst, ni=nindex, nd=ndelta) == 0
    out = (C.c_int32 * 5)()
    assert lib.mr_debug_morph(handle, out) == 0 and list(out) == [0, 0, 0, 0, 0]      # a morph alone: nothing moves
    assert weights(t=2) == MR_E_INVALID and b"number of targets" in lib.mr_last_error()
    assert weights(model=1) == MR_E_INVALID
    assert weights(a=np.array([0.5, np.inf, 0.0])) == MR_E_INVALID and b"finite" in lib.mr_last_error()
    assert weights() == 0
    assert lib.mr_debug_morph(handle, out) == 0 and out[0] == 1
    assert weights(a=None, t=0) == 0                               # the rest shape
    assert lib.mr_debug_morph(handle, out) == 0 and out[0] == 0
    assert weights() == 0
    assert morph(f=None, i=None, d=None) == 0                      # the morph goes, and its weights with it
    assert lib.mr_debug_morph(handle, out) == 0 and out[0] == 0
    assert weights() == MR_E_INVALID
    times = (C.c_float * 2)()
    assert lib.mr_debug_morph_times(handle, times) == MR_E_INVALID and b"no pass" in lib.mr_last_error()
    assert lib.mr_debug_morph(handle, None) == MR_E_INVALID and lib.mr_debug_morph(None, out) == MR_E_INVALID
    lib.mr_scene_destroy(handle)
    bare = _scene_with_a_quad(lib, normals=False)
    assert lib.mr_scene_set_model_morph(bare, 0, 3, ptr(first), ptr(index), ptr(delta), ptr(nfirst), ptr(nindex), ptr(ndelta)) == MR_E_INVALID
    assert b"without normals" in lib.mr_last_error()
    lib.mr_scene_destroy(bare)
