"""GPU: ``Model.morph`` / ``Model.morph_weights`` -- morph targets in the pose pass (host_morph.h, host_pose.h;
k_morph_vertices and k_morph_normals in kernels_pose.h).

The yardstick is the twin (morph_ref.py): the recipe built afresh with the morphed model's ``vertices`` (and, with
``normal_targets``, ``normals``) replaced by the arrays the contract names, formed in pure Python.  Morphed scene and twin
hold bit-identical inputs, so everything a caller can read of their frames on one device is compared for equality; the
oracle's frame of the twin is held to the project's standing bars (z / winner / stencil / silhouette / counts bit-exact,
float frame 2e-6, uint8 +-1)."""
import functools

import numpy as np
import pytest

import morph_ref
import pose_normals_ref
import pose_ref
import scenes
import skin_ref
from morph_ref import assert_same, counted
from multilight_ref import extra_lights
from py_numpy_renderer_amd import Morph

pytestmark = pytest.mark.gpu

FUSED, CAPTURE, CACHED = 0, 1, 2
CASES = [(name, shape) for name in morph_ref.RECIPES for shape in morph_ref.SHAPE_NAMES]


@functools.lru_cache(maxsize=None)
def _morphed_and_twin(name, shape):
    """One recipe under one shape: the un-morphed frame, the morphed frame, the twin's frame (each ``counted``), the twin."""
    api = scenes.product_api()
    other = morph_ref.twin(api, name, shape)           # (first: a new Material anywhere makes every scene upload its models again)
    want = counted(other._backend(), other)
    other.close()
    scene, index = morph_ref.build(api, name)
    backend = scene._backend()
    plain = counted(backend, scene)
    morph_ref.apply(api, scene, {index: shape})
    morphed = counted(backend, scene)
    counters = backend.morph_counters()
    scene.close()
    return plain, morphed, want, other, counters


# ---------------------------------------------------------------------------- 1. morphed equals twin, exactly
@pytest.mark.parametrize("name, shape", CASES)
def test_morphed_equals_twin(name, shape):
    """Frame bytes, z bits, winner, stencil, silhouette set, float frame and every counter of ``mr_stats`` are the
    twin's; and the morph moved something: the frame is not the un-morphed one (without the feature ``Morph`` cannot be
    imported)."""
    plain, morphed, want, other, counters = _morphed_and_twin(name, shape)
    assert_same(morphed, want, f"{name} under {shape}")
    assert not np.array_equal(morphed["out"], plain["out"]), f"{name} under {shape}: the morph changed nothing"
    assert not np.array_equal(morphed["z"], plain["z"])
    assert want["stats"]["n_quads"] > 0 and len(want["silhouette0"]) > 0
    n = len(other.models[morph_ref.RECIPES[name][1]].vertices)
    assert counters[:4] == (1, morph_ref.N_TARGETS[shape], n, 0), counters
    assert counters[4] % 64 == 0 and 0 < counters[4] <= -(-n // 64) * 64 * morph_ref.N_TARGETS[shape], counters


# ---------------------------------------------------------------------------- 2. morphed equals the oracle of the twin
@pytest.mark.parametrize("name, shape", CASES)
def test_morphed_equals_the_oracle_of_the_twin(oracle_mod, name, shape):
    _, morphed, _, other, _ = _morphed_and_twin(name, shape)
    _hold_to_the_oracle(oracle_mod, morphed, other, f"{name} under {shape}")


def _hold_to_the_oracle(oracle_mod, got, other, label):
    want = oracle_mod.render(other, shadows=True)
    assert np.array_equal(got["z"], want.z.view(np.uint64)), f"{label}: z"
    assert np.array_equal(got["winner"], want.winner), f"{label}: winner"
    assert np.array_equal(got["stencil0"], want.stencil), f"{label}: stencil"
    assert set(got["silhouette0"]) == set(map(tuple, want.silhouette.tolist())), f"{label}: silhouette"
    assert got["stats"]["n_quads"] == want.stats["n_quads"], f"{label}: silhouette edges"
    assert got["stats"]["frag_tri"] == want.stats["frag_tri_pass1"], f"{label}: triangle fragments"
    assert got["stats"]["frag_quad"] == want.stats["frag_quad"], f"{label}: quad fragments"
    err = np.abs(got["frame"].view(np.float32).astype(np.float64) - want.frame.astype(np.float64)).max()
    print(f"{label}: float frame differs from the oracle's by at most {err:.3g}")
    assert err <= 2e-6, f"{label}: float frame {err}"
    assert np.abs(got["out"].astype(np.int16) - want.out.astype(np.int16)).max() <= 1, f"{label}: uint8 frame"


# ---------------------------------------------------------------------------- 3. normals that follow the morph
@pytest.mark.parametrize("name", ["diablo_floor", "torus_spot"])
def test_normals_follow_the_morph(oracle_mod, name):
    """``normal_targets``: the twin with its normals replaced too (diablo: a tangent map, ``vn`` counted apart from
    ``v``), not the frame of the same shape without them; geometry (z, stencil) is that frame's."""
    _, without, _, _, _ = _morphed_and_twin(name, "bands")
    _, morphed, want, other, counters = _morphed_and_twin(name, "normals")
    assert_same(morphed, want, f"{name} under normals")
    assert not np.array_equal(morphed["frame"], without["frame"]), "the normals did not follow"
    assert np.array_equal(morphed["z"], without["z"]) and np.array_equal(morphed["stencil0"], without["stencil0"])
    assert counters[3] == len(other.models[morph_ref.RECIPES[name][1]].normals), counters
    _hold_to_the_oracle(oracle_mod, morphed, other, f"{name} under normals")


# ---------------------------------------------------------------------------- 4. morph, then skin, then pose
@pytest.mark.parametrize("name", ["diablo_floor", "torus_spot"])
def test_skin_pose_and_pose_normals_on_top_of_the_morph(api, name):
    """The morph alone, then a ``bend`` skin with ``normals=True`` on top, then a pose, then ``pose_normals``, each a
    frame later and each its twin's; new weights under the standing skin and pose; then everything taken away again in
    reverse order, ending on the first frame bit for bit."""
    matrix = pose_ref.matrices(api)["product"]
    index = morph_ref.RECIPES[name][1]
    rigs, poses = {index: "bend"}, {index: matrix}
    steps = (dict(), dict(rigs=rigs, skin_normals=True), dict(rigs=rigs, skin_normals=True, poses=poses),
             dict(rigs=rigs, skin_normals=True, poses=poses, pose_normals=True),
             dict(frame=1, rigs=rigs, skin_normals=True, poses=poses, pose_normals=True))
    wants = []
    for kw in steps:
        other = morph_ref.twin(api, name, "normals", **kw)
        wants.append(counted(other._backend(), other))
        other.close()
    scene, index = morph_ref.build(api, name)
    backend, model = scene._backend(), scene.models[index]
    first = counted(backend, scene)
    rig = skin_ref.rig(api, model, "bend")
    morph_ref.apply(api, scene, {index: "normals"})
    assert_same(counted(backend, scene), wants[0], "morph")
    model.skin = skin_ref.Skin(rig[0], rig[1], normals=True)
    model.bones = rig[2]
    assert_same(counted(backend, scene), wants[1], "morph, then skin")
    assert not np.array_equal(wants[1]["frame"], wants[0]["frame"])
    model.pose = matrix
    assert_same(counted(backend, scene), wants[2], "morph, then skin, then pose")
    model.pose_normals = True
    assert_same(counted(backend, scene), wants[3], "morph, then skin, then pose with pose_normals")
    assert not np.array_equal(wants[3]["frame"], wants[2]["frame"])
    model.morph_weights = morph_ref.shape(model, "normals", frame=1)[2]
    assert_same(counted(backend, scene), wants[4], "new weights under the skin and the pose")
    assert not np.array_equal(wants[4]["z"], wants[3]["z"])
    model.morph_weights = morph_ref.shape(model, "normals")[2]
    assert_same(counted(backend, scene), wants[3], "the first weights again")
    model.pose_normals = False
    assert_same(counted(backend, scene), wants[2], "pose_normals taken away")
    model.pose = None
    assert_same(counted(backend, scene), wants[1], "the pose taken away")
    model.skin = None
    assert_same(counted(backend, scene), wants[0], "the skin taken away")
    model.morph_weights = None
    assert_same(counted(backend, scene), first, "morph_weights = None")
    assert backend.morph_counters()[0] == 0                        # (the other counters are the last pass's)
    scene.close()


def test_a_pose_with_pose_normals_straight_on_the_morph(api):
    """No skin between: the morph's normals go through the normal matrix, and new weights bring new normals."""
    matrix = pose_ref.matrices(api)["rotation"]
    wants = []
    for frame in (0, 1):
        other = morph_ref.twin(api, "torus_spot", "normals", frame=frame, poses={0: matrix}, pose_normals=True)
        wants.append(counted(other._backend(), other))
        other.close()
    scene, index = morph_ref.build(api, "torus_spot")
    backend, model = scene._backend(), scene.models[index]
    model.pose, model.pose_normals = matrix, True
    backend.render(scene, shadows=True)
    for frame in (0, 1, 0):
        morph_ref.apply(api, scene, {index: "normals"}, frame=frame)
        assert_same(counted(backend, scene), wants[frame], f"weights {frame} under the pose")
    scene.close()


# ---------------------------------------------------------------------------- 5. several models in one pass
@pytest.mark.parametrize("floor_shape", ["dense2", "edge257"])
def test_two_morphed_models_and_a_posed_one(api, floor_shape):
    """diablo (five targets), the cube (posed, no morph) and the 4-vertex floor (2 or 257 targets) in one scene: the
    rows', the slices' and the weight table's offsets all differ from 0 for the floor, whose targets -- most of them
    without entries on four vertices -- follow diablo's five in the weight table."""
    recipe = pose_normals_ref.SMALL_AND_LARGE                      # [diablo, cube, floor]
    shapes, poses = {0: "normals", 2: floor_shape}, {1: pose_ref.matrices(api)["rotation"]}
    other = morph_ref.twin(api, recipe, shapes, poses=poses)
    want = counted(other._backend(), other)
    scene, _ = morph_ref.build(api, recipe)
    backend = scene._backend()
    plain = counted(backend, scene)
    morph_ref.apply(api, scene, shapes)
    scene.models[1].pose = poses[1]
    assert_same(counted(backend, scene), want, "three models")
    n = [len(m.vertices) for m in scene.models]
    assert backend.morph_counters()[:4] == (2, 5 + morph_ref.N_TARGETS[floor_shape], n[0] + n[2], len(scene.models[0].normals))
    assert backend.pose_counters()[2:] == (1, sum(n))
    # the floor alone goes back to rest: its weights leave the table, diablo's stay
    scene.models[2].morph_weights = None
    third = morph_ref.twin(api, recipe, {0: "normals"}, poses=poses)
    assert_same(counted(backend, scene), counted(third._backend(), third), "the floor at rest")
    assert backend.morph_counters()[:3] == (1, 5, n[0])
    scene.models[0].morph = None
    scene.models[1].pose = None
    assert_same(counted(backend, scene), plain, "all at rest")
    scene.close(), other.close(), third.close()


# ---------------------------------------------------------------------------- 6. a sequence
def test_a_morphing_torus(api):
    """Eight frames with new weights each: every frame its twin's, one full commit at most (the torus' faces lose their
    float32 bit once), one pass per frame over the torus' vertices and no others; weights left alone launch nothing;
    ``morph_weights = None`` gives the first frame back."""
    want = {}
    for i in range(1, 9):
        other = morph_ref.twin(api, "torus_spot", "bands", frame=i)
        want[i] = counted(other._backend(), other)
        other.close()
    scene, index = morph_ref.build(api, "torus_spot")
    backend = scene._backend()
    torus = scene.models[index]
    first = counted(backend, scene)
    targets, _, _ = morph_ref.shape(torus, "bands")
    torus.morph = Morph(targets)
    assert_same(counted(backend, scene), first, "a morph without weights")
    commits0, passes0 = backend.pose_counters()[:2]
    assert (commits0, passes0) == (1, 0) and backend.morph_counters() == (0, 0, 0, 0, 0)
    for i in range(1, 9):
        torus.morph_weights = morph_ref.shape(torus, "bands", frame=i)[2]
        got = counted(backend, scene)
        assert_same(got, want[i], f"frame {i}")
        commits, passes, posed, written = backend.pose_counters()
        assert commits - commits0 <= 1 and passes == i and posed == 0 and written == len(torus.vertices), (i, commits, passes, written)
        assert backend.morph_counters()[:4] == (1, 5, len(torus.vertices), 0)
        assert not np.array_equal(got["out"], first["out"])
    times = backend.morph_times()
    assert times["morph_vertices"] > 0 and times["morph_normals"] == 0
    torus.morph_weights = np.array(torus.morph_weights)            # the same weights in a new array: nothing to do
    assert_same(counted(backend, scene), want[8], "weights unchanged")
    assert backend.pose_counters()[:2] == (commits, 8)
    torus.morph_weights = None
    assert_same(counted(backend, scene), first, "morph_weights = None")
    assert backend.morph_counters()[0] == 0
    scene.close()


# ---------------------------------------------------------------------------- 7. the silhouette cache
def test_the_silhouette_cache_follows_the_weights(api):
    """Standing light: the first frame after new weights tests every edge again (path 0 or 1), frames with the weights
    left alone reach the cached path, and new weights start over; all frames are the twin's."""
    wants = {}
    for frame in (0, 1):
        other = morph_ref.twin(api, "torus_spot", "dense2", frame=frame)
        wants[frame] = counted(other._backend(), other)
        other.close()
    scene, index = morph_ref.build(api, "torus_spot")
    backend = scene._backend()
    for _ in range(3):
        backend.render(scene, shadows=True)
    assert backend.sil_cache()[0] == CACHED
    commits = backend.pose_counters()[0]
    scene.models[index].morph = Morph(morph_ref.shape(scene.models[index], "dense2")[0])     # (once: the weights are what changes)
    for frame in (0, 1):
        scene.models[index].morph_weights = morph_ref.shape(scene.models[index], "dense2", frame=frame)[2]
        paths = []
        for k in range(4):
            got = counted(backend, scene)
            paths.append(backend.sil_cache()[0])
            assert_same(got, wants[frame], f"weights {frame}, frame {k} (path {paths[-1]})")
        assert paths[0] in (FUSED, CAPTURE) and paths[-1] == CACHED, paths
        assert backend.sil_cache()[1] == wants[frame]["stats"]["n_quads"]
    assert backend.pose_counters()[:2] == (commits + 1, 2)
    scene.close()


# ---------------------------------------------------------------------------- 8. the other frame kinds
def _pair(api, name, shape="bands", prepare=lambda scene: None):
    other = morph_ref.twin(api, name, shape)
    prepare(other)
    scene, index = morph_ref.build(api, name)
    prepare(scene)
    scene._backend().render(scene, shadows=True)                   # (at rest first: the weights arrive between frames)
    morph_ref.apply(api, scene, {index: shape})
    return scene, other


def test_supersampled(api):
    def prepare(scene):
        scene.supersample = 2
    scene, other = _pair(api, "torus_spot", prepare=prepare)
    assert_same(counted(scene._backend(), scene), counted(other._backend(), other), "supersample = 2")
    assert np.array_equal(scene.render(), other.render())
    scene.close(), other.close()


def test_three_lights(api):
    def prepare(scene):
        for light in extra_lights(api)[:2]:
            scene.add_light(light)
    scene, other = _pair(api, "diablo_floor", "normals", prepare=prepare)
    assert_same(counted(scene._backend(), scene, lights=3), counted(other._backend(), other, lights=3), "three lights")
    scene.close(), other.close()


def test_overlay(api):
    scene, other = _pair(api, "cube_outward", "dense2")
    assert_same(counted(scene._backend(), scene, overlay=True), counted(other._backend(), other, overlay=True), "overlay")
    scene.draw_debug_frustum = other.draw_debug_frustum = True
    assert np.array_equal(scene.render(), other.render())
    scene.close(), other.close()


def _band_taps(backend, h, band):
    """z / winner / stencil of the rows of a band (the taps count screen rows from the bottom, the band output rows)."""
    rows = slice(h - band[1], h - band[0])
    return [backend.read_z().view(np.uint64)[rows].copy(), backend.read_winner()[rows].copy(), backend.read_stencil()[rows].copy()]


def test_row_band(api):
    scene, other = _pair(api, "torus_spot", "slices")
    h = scene.resolution[0]
    whole = other.render().copy()
    for band in ((0, 64), (48, 112), (112, h)):
        # (without the fragment counters: a counted frame never culls clusters, a band without them does by default)
        got = scene._backend().render(scene, shadows=True, counters=False, keep_buffers=True, row_band=band).copy()
        taps = _band_taps(scene._backend(), h, band)
        want = other._backend().render(other, shadows=True, counters=False, keep_buffers=True, row_band=band).copy()
        assert np.array_equal(got, want) and np.array_equal(got, whole[band[0]:band[1]]), band
        for a, b in zip(taps, _band_taps(other._backend(), h, band)):
            assert np.array_equal(a, b), band
    scene.close(), other.close()


def test_render_async_with_new_weights_each_frame(api):
    """Eight frames two deep, new weights in front of each: the pass drains the frames in flight, and every frame is its
    twin's synchronous one."""
    scene, index = morph_ref.build(api, "torus_spot")
    scene.render()
    queue, got = [], []
    for i in range(1, 9):
        morph_ref.apply(api, scene, {index: "bands"}, frame=i) if i == 1 else setattr(
            scene.models[index], "morph_weights", morph_ref.shape(scene.models[index], "bands", frame=i)[2])
        queue.append(scene.render_async())
        if len(queue) >= 2:
            got.append(queue.pop(0).result().copy())
    got += [p.result().copy() for p in queue]
    assert scene._backend().pose_counters()[1] == 8
    scene.close()
    for i in range(1, 9):
        other = morph_ref.twin(api, "torus_spot", "bands", frame=i)
        assert np.array_equal(got[i - 1], other.render()), f"frame {i}"
        other.close()


def test_a_float32_model_morphed_and_unmorphed_again(api):
    """torus_spot's torus is float32: its faces lose the float32 bit with the weights (one ordinary commit) and get it
    back with ``morph_weights = None`` (another), and the last frame is the first bit for bit."""
    scene, index = morph_ref.build(api, "torus_spot")
    backend, torus = scene._backend(), scene.models[index]
    assert np.asarray(torus.vertices).dtype == np.float32
    first = counted(backend, scene)
    assert backend.pose_counters()[:2] == (1, 0)
    morph_ref.apply(api, scene, {index: "slices"})
    other = morph_ref.twin(api, "torus_spot", "slices")
    assert_same(counted(backend, scene), counted(other._backend(), other), "morphed")
    assert backend.pose_counters()[:2] == (2, 1)
    torus.morph_weights = None
    assert_same(counted(backend, scene), first, "un-morphed again")
    assert backend.pose_counters()[0] == 3
    scene.close(), other.close()
