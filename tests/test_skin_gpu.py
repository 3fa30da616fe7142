"""GPU: ``Model.skin`` / ``Model.bones`` -- linear-blend skinning in the pose pass (host_pose.h; k_skin_vertices and
k_skin_normals in kernels_pose.h).

The yardstick is the twin (skin_ref.py): the recipe built afresh with the skinned model's ``vertices`` (and, with
``normals=True``, ``normals``) replaced by the arrays the contract names, formed in pure Python.  Skinned scene and twin
hold bit-identical inputs, so everything a caller can read of their frames on one device is compared for equality; the
oracle's frame of the twin is held to the project's standing bars (z / winner / stencil / silhouette / counts bit-exact,
float frame 2e-6, uint8 +-1)."""
import functools

import numpy as np
import pytest

import pose_normals_ref
import pose_ref
import scenes
import skin_ref
from multilight_ref import extra_lights
from py_numpy_renderer_amd import Skin
from skin_ref import assert_same, counted

pytestmark = pytest.mark.gpu

FUSED, CAPTURE, CACHED = 0, 1, 2
CASES = [(name, rig) for name in skin_ref.RECIPES for rig in skin_ref.RIG_NAMES]


@functools.lru_cache(maxsize=None)
def _skinned_and_twin(name, rig, normals=False):
    """One recipe under one rig: the un-skinned frame, the skinned frame, the twin's frame (each ``counted``), the twin."""
    api = scenes.product_api()
    other = skin_ref.twin(api, name, rig, normals=normals)          # (first: a new Material anywhere makes every scene upload its models again)
    want = counted(other._backend(), other)
    other.close()
    scene, index = skin_ref.build(api, name)
    backend = scene._backend()
    plain = counted(backend, scene)
    skin_ref.apply(api, scene, {index: rig}, normals=normals)
    skinned = counted(backend, scene)
    counters = backend.skin_counters()
    scene.close()
    return plain, skinned, want, other, counters


# ---------------------------------------------------------------------------- 1. skinned equals twin, exactly
@pytest.mark.parametrize("name, rig", CASES)
def test_skinned_equals_twin(name, rig):
    """Frame bytes, z bits, winner, stencil, silhouette set, float frame and every counter of ``mr_stats`` are the
    twin's; and the skin moved something: the frame is not the un-skinned one (without the feature ``skin`` and ``bones``
    are two attributes nobody reads)."""
    plain, skinned, want, other, counters = _skinned_and_twin(name, rig)
    assert_same(skinned, want, f"{name} under {rig}")
    assert not np.array_equal(skinned["out"], plain["out"]), f"{name} under {rig}: the skin changed nothing"
    assert not np.array_equal(skinned["z"], plain["z"])
    assert want["stats"]["n_quads"] > 0 and len(want["silhouette0"]) > 0
    assert counters == (1, skin_ref.N_BONES[rig], len(other.models[skin_ref.RECIPES[name][1]].vertices), 0), counters


# ---------------------------------------------------------------------------- 2. skinned equals the oracle of the twin
@pytest.mark.parametrize("name, rig", CASES)
def test_skinned_equals_the_oracle_of_the_twin(oracle_mod, name, rig):
    _, skinned, _, other, _ = _skinned_and_twin(name, rig)
    _hold_to_the_oracle(oracle_mod, skinned, other, f"{name} under {rig}")


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


# ---------------------------------------------------------------------------- 3. normals that follow the skin
@pytest.mark.parametrize("name, rig", [("diablo_floor", "bend"), ("diablo_floor", "edge64"), ("torus_spot", "twist"), ("torus_spot", "edge1")])
def test_normals_follow_the_skin(oracle_mod, name, rig):
    """``Skin(..., normals=True)``: the twin with its normals replaced too (diablo: a tangent map, ``vn`` counted apart
    from ``v``), not the frame of ``normals=False``; geometry (z, winner, stencil) is that of ``normals=False``."""
    _, without, _, _, _ = _skinned_and_twin(name, rig)
    _, skinned, want, other, counters = _skinned_and_twin(name, rig, True)
    assert_same(skinned, want, f"{name} under {rig}, normals=True")
    assert not np.array_equal(skinned["frame"], without["frame"]), "the normals did not follow"
    assert np.array_equal(skinned["z"], without["z"]) and np.array_equal(skinned["stencil0"], without["stencil0"])
    assert counters[3] == len(other.models[skin_ref.RECIPES[name][1]].normals), counters
    _hold_to_the_oracle(oracle_mod, skinned, other, f"{name} under {rig}, normals=True")


@pytest.mark.parametrize("name", ["diablo_floor", "torus_spot"])
def test_pose_and_pose_normals_on_top_of_the_skin(api, name):
    """Skin first, then pose; the normals take S[:3, :3] of their owner, then G, and are rounded once.  The pose arrives
    a frame after the skin, the normal matrix a frame after the pose; taking all three away again gives the first frame."""
    matrix = pose_ref.matrices(api)["product"]
    index = skin_ref.RECIPES[name][1]
    wants = []
    for kw in (dict(), dict(poses={index: matrix}), dict(poses={index: matrix}, pose_normals=True)):
        other = skin_ref.twin(api, name, "bend", normals=True, **kw)
        wants.append(counted(other._backend(), other))
        other.close()
    scene, index = skin_ref.build(api, name)
    backend, model = scene._backend(), scene.models[index]
    first = counted(backend, scene)
    skin_ref.apply(api, scene, {index: "bend"}, normals=True)
    assert_same(counted(backend, scene), wants[0], "skin")
    model.pose = matrix
    assert_same(counted(backend, scene), wants[1], "skin, then pose")
    model.pose_normals = True
    assert_same(counted(backend, scene), wants[2], "skin, then pose with pose_normals")
    assert not np.array_equal(wants[2]["frame"], wants[1]["frame"])
    model.bones = skin_ref.rig(api, model, "bend", frame=1)[2]     # new bones under a standing pose
    other = skin_ref.twin(api, name, "bend", normals=True, frame=1, poses={index: matrix}, pose_normals=True)
    assert_same(counted(backend, scene), counted(other._backend(), other), "new bones under the pose")
    other.close()
    model.pose = None
    model.bones = skin_ref.rig(api, model, "bend")[2]
    assert_same(counted(backend, scene), wants[0], "the pose taken away")
    model.skin = None
    assert_same(counted(backend, scene), first, "skin = None")
    scene.close()


# ---------------------------------------------------------------------------- 4. one bone, weight 1: a pose
@pytest.mark.parametrize("name", ["torus_spot", "cube_outward"])
def test_one_bone_of_weight_one_is_a_pose(api, name):
    """The ``single`` rig blends one matrix (no -0.0 entry) with weight 1 and zeroes: S is that matrix bit for bit, and
    the frame is the one ``pose =`` that matrix gives."""
    matrix = skin_ref.single_matrix(api)
    assert not np.signbit(matrix[matrix == 0]).any()
    _, skinned, _, _, _ = _skinned_and_twin(name, "single")
    scene, index = skin_ref.build(api, name)
    scene.models[index].pose = matrix
    assert_same(counted(scene._backend(), scene), skinned, f"{name}: pose = the bone")
    scene.close()


# ---------------------------------------------------------------------------- 5. several models in one pass
@pytest.mark.parametrize("floor_rig", ["edge64", "edge65"])
def test_two_skinned_models_and_a_posed_one(api, floor_rig):
    """diablo (3 bones), the cube (posed, no skin) and the 4-vertex floor (64 or 65 bones) in one scene: the rows', the
    joints' and the bone table's offsets all differ from 0 for the floor.  With 65 bones on the floor the pass is over
    the staged kernel's capacity and diablo goes through the plain one too."""
    recipe = pose_normals_ref.SMALL_AND_LARGE                      # [diablo, cube, floor]
    rigs, poses = {0: "bend", 2: floor_rig}, {1: pose_ref.matrices(api)["rotation"]}
    other = skin_ref.twin(api, recipe, rigs, normals=True, poses=poses)
    want = counted(other._backend(), other)
    scene, _ = skin_ref.build(api, recipe)
    backend = scene._backend()
    plain = counted(backend, scene)
    skin_ref.apply(api, scene, rigs, normals=True)
    scene.models[1].pose = poses[1]
    assert_same(counted(backend, scene), want, "three models")
    n = [len(m.vertices) for m in scene.models]
    followed = sum(len(scene.models[k].normals) for k in rigs if scene.models[k].normals is not None)
    assert backend.skin_counters() == (2, 3 + skin_ref.N_BONES[floor_rig], n[0] + n[2], followed)
    assert backend.pose_counters()[2:] == (1, sum(n))
    # the floor alone goes back to rest: its bones leave the table, diablo's stay
    scene.models[2].bones = None
    third = skin_ref.twin(api, recipe, {0: "bend"}, normals=True, poses=poses)
    assert_same(counted(backend, scene), counted(third._backend(), third), "the floor at rest")
    assert backend.skin_counters()[:3] == (1, 3, n[0])
    scene.models[0].bones = None
    scene.models[1].pose = None
    assert_same(counted(backend, scene), plain, "all at rest")
    scene.close(), other.close(), third.close()


def test_a_skinned_model_beside_a_posed_floor(api):
    """cube_outward: the cube (8 vertices, float64 already) skinned, its second model -- the floor -- posed, no skin."""
    poses = {1: pose_ref.matrices(api)["translation"]}
    other = skin_ref.twin(api, "cube_outward", "twist", poses=poses)
    scene, index = skin_ref.build(api, "cube_outward")
    skin_ref.apply(api, scene, {index: "twist"})
    scene.models[1].pose = poses[1]
    backend = scene._backend()
    assert_same(counted(backend, scene), counted(other._backend(), other), "skinned cube, posed floor")
    assert backend.pose_counters()[:3] == (1, 1, 1) and backend.skin_counters()[:3] == (1, 4, 8)
    scene.close(), other.close()


# ---------------------------------------------------------------------------- 6. a sequence
def test_a_bending_torus(api):
    """Eight frames with new bones each: every frame its twin's, one full commit at most (the torus' faces lose their
    float32 bit once), one pass per frame over the torus' vertices and no others; ``bones = None`` gives the first
    frame back."""
    want = {}
    for i in range(1, 9):
        other = skin_ref.twin(api, "torus_spot", "bend", frame=i)
        want[i] = counted(other._backend(), other)
        other.close()
    scene, index = skin_ref.build(api, "torus_spot")
    backend = scene._backend()
    torus = scene.models[index]
    first = counted(backend, scene)
    joints, weights, _ = skin_ref.rig(api, torus, "bend")
    torus.skin = Skin(joints, weights)
    assert_same(counted(backend, scene), first, "a skin without bones")
    commits0, passes0 = backend.pose_counters()[:2]
    assert (commits0, passes0) == (1, 0) and backend.skin_counters() == (0, 0, 0, 0)
    for i in range(1, 9):
        torus.bones = skin_ref.rig(api, torus, "bend", frame=i)[2]
        got = counted(backend, scene)
        assert_same(got, want[i], f"frame {i}")
        commits, passes, posed, written = backend.pose_counters()
        assert commits - commits0 <= 1 and passes == i and posed == 0 and written == len(torus.vertices), (i, commits, passes, written)
        assert backend.skin_counters() == (1, 3, len(torus.vertices), 0)
        assert not np.array_equal(got["out"], first["out"])
    times = backend.skin_times()
    assert times["skin_vertices"] > 0 and times["skin_normals"] == 0
    torus.bones = None
    assert_same(counted(backend, scene), first, "bones = None")
    assert backend.skin_counters()[0] == 0
    scene.close()


# ---------------------------------------------------------------------------- 7. the silhouette cache
def test_the_silhouette_cache_follows_the_bones(api):
    """Standing light: the first frame after new bones tests every edge again (path 0 or 1), frames with the bones left
    alone reach the cached path, and new bones start over; all frames are the twin's."""
    wants = {}
    for frame in (0, 1):
        other = skin_ref.twin(api, "torus_spot", "twist", frame=frame)
        wants[frame] = counted(other._backend(), other)
        other.close()
    scene, index = skin_ref.build(api, "torus_spot")
    backend = scene._backend()
    for _ in range(3):
        backend.render(scene, shadows=True)
    assert backend.sil_cache()[0] == CACHED
    commits = backend.pose_counters()[0]
    joints, weights, _ = skin_ref.rig(api, scene.models[index], "twist")
    scene.models[index].skin = Skin(joints, weights)               # (once: the bones are what changes)
    for frame in (0, 1):
        scene.models[index].bones = skin_ref.rig(api, scene.models[index], "twist", frame=frame)[2]
        paths = []
        for k in range(4):
            got = counted(backend, scene)
            paths.append(backend.sil_cache()[0])
            assert_same(got, wants[frame], f"bones {frame}, frame {k} (path {paths[-1]})")
        assert paths[0] in (FUSED, CAPTURE) and paths[-1] == CACHED, paths
        assert backend.sil_cache()[1] == wants[frame]["stats"]["n_quads"]
    assert backend.pose_counters()[:2] == (commits + 1, 2)
    scene.close()


# ---------------------------------------------------------------------------- 8. the other frame kinds
def _pair(api, name, rig="bend", normals=False, prepare=lambda scene: None):
    other = skin_ref.twin(api, name, rig, normals=normals)
    prepare(other)
    scene, index = skin_ref.build(api, name)
    prepare(scene)
    scene._backend().render(scene, shadows=True)                   # (at rest first: the bones arrive between frames)
    skin_ref.apply(api, scene, {index: rig}, normals=normals)
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
    scene, other = _pair(api, "diablo_floor", normals=True, prepare=prepare)
    assert_same(counted(scene._backend(), scene, lights=3), counted(other._backend(), other, lights=3), "three lights")
    scene.close(), other.close()


def test_overlay(api):
    scene, other = _pair(api, "cube_outward", "twist")
    assert_same(counted(scene._backend(), scene, overlay=True), counted(other._backend(), other, overlay=True), "overlay")
    scene.draw_debug_frustum = other.draw_debug_frustum = True
    assert np.array_equal(scene.render(), other.render())
    scene.close(), other.close()


def _band_taps(backend, h, band):
    """z / winner / stencil of the rows of a band (the taps count screen rows from the bottom, the band output rows)."""
    rows = slice(h - band[1], h - band[0])
    return [backend.read_z().view(np.uint64)[rows].copy(), backend.read_winner()[rows].copy(), backend.read_stencil()[rows].copy()]


def test_row_band(api):
    scene, other = _pair(api, "torus_spot", "twist")
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
        assert np.array_equal(scene._backend().render(scene, shadows=True, row_band=band), want), band     # counted
    scene.close(), other.close()


def test_render_async_with_new_bones_each_frame(api):
    """Eight frames two deep, new bones in front of each: the pass drains the frames in flight, and every frame is its
    twin's synchronous one."""
    scene, index = skin_ref.build(api, "torus_spot")
    scene.render()
    queue, got = [], []
    joints, weights, _ = skin_ref.rig(api, scene.models[index], "bend")
    scene.models[index].skin = Skin(joints, weights)
    for i in range(1, 9):
        scene.models[index].bones = skin_ref.rig(api, scene.models[index], "bend", frame=i)[2]
        queue.append(scene.render_async())
        if len(queue) >= 2:
            got.append(queue.pop(0).result().copy())
    got += [p.result().copy() for p in queue]
    assert scene._backend().pose_counters()[1] == 8
    scene.close()
    for i in range(1, 9):
        other = skin_ref.twin(api, "torus_spot", "bend", frame=i)
        assert np.array_equal(got[i - 1], other.render()), f"frame {i}"
        other.close()


def test_bones_that_overflow_the_lists(api):
    """Lists sized for nothing: the skinned frame goes through the existing regrow path and is the twin's, counted and
    asynchronous."""
    other, later = skin_ref.twin(api, "torus_spot", "edge64"), skin_ref.twin(api, "torus_spot", "edge64", frame=2)
    scene, index = skin_ref.build(api, "torus_spot")
    backend = scene._backend()
    backend.render(scene, shadows=True)
    backend.set_list_capacities(small_pairs=4, big_pairs=2, quads=3, work=16)
    skin_ref.apply(api, scene, {index: "edge64"})
    assert_same(counted(backend, scene), counted(other._backend(), other), "small lists")
    backend.set_list_capacities(small_pairs=4, big_pairs=2, quads=3, work=16)
    scene.models[index].bones = skin_ref.rig(api, scene.models[index], "edge64", frame=2)[2]
    frame = scene.render_async().result()
    assert backend.pose_counters()[:2] == (2, 2)
    assert np.array_equal(frame, later.render())
    scene.close(), other.close(), later.close()


# ---------------------------------------------------------------------------- 9. the cluster records
CONE_RECIPE = (lambda api: scenes.torus_spot(api, resolution=(180, 320), nu=8, nv=200), 0)         # 3 200 faces + 2: 51 clusters


def _face_corners(scene):
    """(F, 3, 3) float64 world-space corners and (F, 3) unit normals of a twin's faces, models concatenated."""
    corners = []
    for model in scene.models:
        v = np.asarray(model.vertices, dtype=np.float64)
        corners.append(v[np.asarray(model._faces)[..., 0], :3])
    corners = np.concatenate(corners)
    n = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    return corners, n / np.linalg.norm(n, axis=1, keepdims=True)


@pytest.mark.parametrize("rig", ["bend", "twist"])
def test_cluster_records_are_conservative(api, rig):
    """The records the pass builds on the device (k_clusters) from skinned vertices, read back: every cluster's box holds
    every skinned corner of its 64 faces, and every face's unit normal lies in its cone.  No cluster is skipped.  (The
    rigs keep w = 1: a cluster whose corners have another w has no box to check.)"""
    other = skin_ref.twin(api, CONE_RECIPE, rig)
    scene, index = skin_ref.build(api, CONE_RECIPE)
    backend = scene._backend()
    backend.render(scene, shadows=True)
    host_built = backend.read_clusters().copy()
    skin_ref.apply(api, scene, {index: rig})
    backend.render(scene, shadows=True)
    assert backend.pose_counters()[:2] == (2, 1)
    rec = backend.read_clusters()
    corners, normals = _face_corners(other)
    n_faces = len(corners)
    assert len(rec) == 51 == len(host_built) == -(-n_faces // 64)
    assert not np.array_equal(rec["lo"], host_built["lo"])
    coned = 0
    for c in range(len(rec)):
        faces = slice(64 * c, min(64 * c + 64, n_faces))
        pts = corners[faces].reshape(-1, 3)
        lo, hi = rec["lo"][c].astype(np.float64), rec["hi"][c].astype(np.float64)
        assert np.isfinite(lo).all() and np.isfinite(hi).all(), c
        assert (pts >= lo).all() and (pts <= hi).all(), f"cluster {c}: a corner outside the box"
        assert (hi - pts.max(axis=0) < 1e-6).all() and (pts.min(axis=0) - lo < 1e-6).all(), f"cluster {c}: the box is loose"
        if rec["cos_half"][c] < -1:
            continue                                               # no cone: nothing is claimed
        coned += 1
        axis = rec["axis"][c].astype(np.float64)
        assert abs(np.linalg.norm(axis) - 1) < 1e-6, c
        dots = normals[faces] @ axis
        assert dots.min() >= float(rec["cos_half"][c]) - 1e-7, f"cluster {c}: a normal outside the cone ({dots.min()} < {rec['cos_half'][c]})"
        assert float(rec["sin_half"][c]) ** 2 + float(rec["cos_half"][c]) ** 2 >= 1 - 1e-6, c
    print(f"{coned} of {len(rec)} clusters have a cone")
    assert coned > 0, "no cluster has a cone: the case proves nothing about cones"
    # the twin's records, built on the host, claim the same cones up to the summation order
    other._backend().render(other, shadows=True)
    want = other._backend().read_clusters()
    assert np.array_equal(rec["cos_half"] < -1, want["cos_half"] < -1)
    assert np.abs(rec["axis"] - want["axis"]).max() < 1e-6 and np.abs(rec["cos_half"] - want["cos_half"]).max() < 1e-6
    assert np.array_equal(rec["lo"], want["lo"]) and np.array_equal(rec["hi"], want["hi"])
    scene.close(), other.close()
