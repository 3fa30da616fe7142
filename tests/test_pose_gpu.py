"""GPU: ``Model.pose`` -- a model moved between frames by the pose pass on the device (host_pose.h, kernels_pose.h).

The yardstick is the twin (pose_ref.py): the recipe built afresh with the posed model's vertices replaced by
``matmul_chain(float64(vertices), M)``.  Posed scene and twin hold bit-identical inputs, so everything a caller can
read of their frames on one device is compared for equality; the oracle's frame of the twin is held to the project's
standing bars (z / winner / stencil / silhouette / counts bit-exact, float frame 2e-6, uint8 +-1)."""
import functools

import numpy as np
import pytest

import pose_ref
import scenes
from multilight_ref import extra_lights
from pose_ref import assert_same, counted

pytestmark = pytest.mark.gpu

FUSED, CAPTURE, CACHED = 0, 1, 2
CASES = [(name, m) for name in pose_ref.RECIPES for m in pose_ref.MATRIX_NAMES]


@functools.lru_cache(maxsize=None)
def _posed_and_twin(name, mname):
    """One recipe under one pose: the un-posed frame, the posed frame, the twin's frame (each ``counted``) and the twin."""
    api = scenes.product_api()
    matrix = pose_ref.matrices(api)[mname]
    scene, index = pose_ref.build(api, name)
    backend = scene._backend()
    plain = counted(backend, scene)
    scene.models[index].pose = matrix
    posed = counted(backend, scene)
    scene.close()
    other = pose_ref.twin(api, name, matrix)
    want = counted(other._backend(), other)
    other.close()
    return plain, posed, want, other


# ---------------------------------------------------------------------------- 1. posed equals twin, exactly
@pytest.mark.parametrize("name, mname", CASES)
def test_posed_equals_twin(name, mname):
    """Frame bytes, z bits, winner, stencil, silhouette set, float frame and every counter of ``mr_stats`` are the
    twin's; and the pose moved something: the frame is not the un-posed one (today ``pose`` would be ignored)."""
    plain, posed, want, _ = _posed_and_twin(name, mname)
    assert_same(posed, want, f"{name} under {mname}")
    assert not np.array_equal(posed["out"], plain["out"]), f"{name} under {mname}: the pose changed nothing"
    assert not np.array_equal(posed["z"], plain["z"])
    assert want["stats"]["n_quads"] > 0 and len(want["silhouette0"]) > 0


# ---------------------------------------------------------------------------- 2. posed equals the oracle of the twin
@pytest.mark.parametrize("name, mname", CASES)
def test_posed_equals_the_oracle_of_the_twin(oracle_mod, name, mname):
    _, posed, _, other = _posed_and_twin(name, mname)
    want = oracle_mod.render(other, shadows=True)
    label = f"{name} under {mname}"
    assert np.array_equal(posed["z"], want.z.view(np.uint64)), f"{label}: z"
    assert np.array_equal(posed["winner"], want.winner), f"{label}: winner"
    assert np.array_equal(posed["stencil0"], want.stencil), f"{label}: stencil"
    assert set(posed["silhouette0"]) == set(map(tuple, want.silhouette.tolist())), f"{label}: silhouette"
    assert posed["stats"]["n_quads"] == want.stats["n_quads"], f"{label}: silhouette edges"
    assert posed["stats"]["frag_tri"] == want.stats["frag_tri_pass1"], f"{label}: triangle fragments"
    assert posed["stats"]["frag_quad"] == want.stats["frag_quad"], f"{label}: quad fragments"
    err = np.abs(posed["frame"].view(np.float32).astype(np.float64) - want.frame.astype(np.float64)).max()
    print(f"{label}: float frame differs from the oracle's by at most {err:.3g}")
    assert err <= 2e-6, f"{label}: float frame {err}"
    assert np.abs(posed["out"].astype(np.int16) - want.out.astype(np.int16)).max() <= 1, f"{label}: uint8 frame"


# ---------------------------------------------------------------------------- 3. a sequence
def test_a_turning_torus(api):
    """Eight frames, the torus turned 3 degrees further on each: every frame its twin's, one full commit at most (the
    torus' faces lose their float32 bit once), one pass per frame over the torus' vertices and no others; ``pose = None``
    gives the first frame back."""
    want = {}
    for i in range(1, 9):           # (the twins first: a new Material anywhere makes every scene upload its models again)
        other = pose_ref.twin(api, "torus_spot", pose_ref.turn(api, 3.0 * i))
        want[i] = counted(other._backend(), other)
        other.close()
    scene, index = pose_ref.build(api, "torus_spot")
    backend = scene._backend()
    torus = scene.models[index]
    first = counted(backend, scene)
    commits0, passes0, posed0, _ = backend.pose_counters()
    assert (commits0, passes0, posed0) == (1, 0, 0)
    for i in range(1, 9):
        torus.pose = pose_ref.turn(api, 3.0 * i)
        got = counted(backend, scene)
        assert_same(got, want[i], f"frame {i}")
        commits, passes, posed, written = backend.pose_counters()
        assert commits - commits0 <= 1 and passes == i and posed == 1 and written == len(torus.vertices), (i, commits, passes, posed, written)
        assert not np.array_equal(got["out"], first["out"])
    torus.pose = None
    assert_same(counted(backend, scene), first, "pose = None")
    assert backend.pose_counters()[2] == 0
    scene.close()


def test_pose_none_returns_the_first_frame(api):
    scene, index = pose_ref.build(api, "torus_spot")
    backend = scene._backend()
    first = counted(backend, scene)
    frame_only = scene.render().copy()
    for i in (1, 2):
        scene.models[index].pose = pose_ref.turn(api, 3.0 * i)
        assert not np.array_equal(scene.render(), frame_only)
    scene.models[index].pose = None
    assert np.array_equal(scene.render(), frame_only)
    assert_same(counted(backend, scene), first, "pose = None")
    assert backend.pose_counters()[2] == 0
    # a float64 model keeps its flags: posing it and letting go of it again commits nothing
    scene, index = pose_ref.build(api, "cube_outward")
    backend = scene._backend()
    first = counted(backend, scene)
    scene.models[index].pose = pose_ref.matrices(api)["mirror"]
    assert not np.array_equal(counted(backend, scene)["out"], first["out"])
    scene.models[index].pose = None
    assert_same(counted(backend, scene), first, "float64 model, pose = None")
    assert backend.pose_counters()[:3] == (1, 2, 0)
    scene.close()


# ---------------------------------------------------------------------------- 4. the silhouette cache
def test_the_silhouette_cache_follows_the_pose(api):
    """Standing light: the first frame after a pose change tests every edge again (path 0 or 1), three frames with
    the pose left alone reach the cached path, and a new pose starts over; all frames are the twin's."""
    wants = {}
    for mname in ("rotation", "product"):
        other = pose_ref.twin(api, "torus_spot", pose_ref.matrices(api)[mname])
        wants[mname] = counted(other._backend(), other)
        other.close()
    scene, index = pose_ref.build(api, "torus_spot")
    backend = scene._backend()
    for _ in range(3):
        backend.render(scene, shadows=True)
    assert backend.sil_cache()[0] == CACHED
    commits = backend.pose_counters()[0]
    for mname in ("rotation", "product"):
        want = wants[mname]
        scene.models[index].pose = pose_ref.matrices(api)[mname]
        paths = []
        for k in range(4):
            got = counted(backend, scene)
            paths.append(backend.sil_cache()[0])
            assert_same(got, want, f"{mname}, frame {k} (path {paths[-1]})")
        assert paths[0] in (FUSED, CAPTURE) and paths[-1] == CACHED, paths
        assert backend.sil_cache()[1] == want["stats"]["n_quads"]
    assert backend.pose_counters()[:2] == (commits + 1, 2)         # the second pose found the cache dropped by its pass alone
    scene.close()


# ---------------------------------------------------------------------------- 5. the other frame kinds
def _pair(api, name, mname="product", prepare=lambda scene: None):
    matrix = pose_ref.matrices(api)[mname]
    other = pose_ref.twin(api, name, matrix)     # (first: a new Material anywhere makes every scene upload its models again)
    prepare(other)
    scene, index = pose_ref.build(api, name)
    prepare(scene)
    scene._backend().render(scene, shadows=True)                   # (un-posed first: the pose arrives between frames)
    scene.models[index].pose = matrix
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
    scene, other = _pair(api, "diablo_floor", prepare=prepare)
    assert_same(counted(scene._backend(), scene, lights=3), counted(other._backend(), other, lights=3), "three lights")
    scene.close(), other.close()


def test_overlay(api):
    scene, other = _pair(api, "cube_outward", "rotation")
    assert_same(counted(scene._backend(), scene, overlay=True), counted(other._backend(), other, overlay=True), "overlay")
    scene.draw_debug_frustum = other.draw_debug_frustum = True
    assert np.array_equal(scene.render(), other.render())
    scene.close(), other.close()


def _band_taps(backend, h, band):
    """z / winner / stencil of the rows of a band (the taps count screen rows from the bottom, the band output rows)."""
    rows = slice(h - band[1], h - band[0])
    return [backend.read_z().view(np.uint64)[rows].copy(), backend.read_winner()[rows].copy(), backend.read_stencil()[rows].copy()]


def test_row_band(api):
    scene, other = _pair(api, "torus_spot", "rotation")
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


def test_render_async_with_a_new_pose_each_frame(api):
    """Eight frames two deep, a new pose in front of each: the pass drains the frames in flight, and every frame is
    its twin's synchronous one."""
    scene, index = pose_ref.build(api, "torus_spot")
    scene.render()
    queue, got = [], []
    for i in range(1, 9):
        scene.models[index].pose = pose_ref.turn(api, 3.0 * i)
        queue.append(scene.render_async())
        if len(queue) >= 2:
            got.append(queue.pop(0).result().copy())
    got += [p.result().copy() for p in queue]
    assert scene._backend().pose_counters()[1] == 8
    scene.close()
    for i in range(1, 9):
        other = pose_ref.twin(api, "torus_spot", pose_ref.turn(api, 3.0 * i))
        assert np.array_equal(got[i - 1], other.render()), f"frame {i}"
        other.close()


def test_a_pose_that_overflows_the_lists(api):
    """Lists sized for nothing and the model posed to three times its size: the frame goes through the existing regrow
    path and is the twin's."""
    big, flipped = np.diag([3.0, 3.0, 3.0, 1.0]), np.diag([3.0, 3.0, -3.0, 1.0])
    other, other_flipped = pose_ref.twin(api, "torus_spot", big), pose_ref.twin(api, "torus_spot", flipped)
    scene, index = pose_ref.build(api, "torus_spot")
    backend = scene._backend()
    backend.render(scene, shadows=True)
    backend.set_list_capacities(small_pairs=4, big_pairs=2, quads=3, work=16)
    scene.models[index].pose = big
    assert_same(counted(backend, scene), counted(other._backend(), other), "3x scale, small lists")
    backend.set_list_capacities(small_pairs=4, big_pairs=2, quads=3, work=16)
    scene.models[index].pose = flipped
    frame = scene.render_async().result()
    assert backend.pose_counters()[:2] == (2, 2)
    assert np.array_equal(frame, other_flipped.render())
    scene.close(), other.close(), other_flipped.close()


# ---------------------------------------------------------------------------- 6. the cluster records
CLUSTER_RECIPE = (lambda api: scenes.torus_spot(api, resolution=(180, 320), nu=80, nv=50), 0)      # 8 000 faces + 2: 126 clusters
# Faces follow each other round the tube, so a cluster of the recipe above covers 32 of its 50 cells, 230 degrees of it,
# and has no cone.  With 200 cells round the tube a cluster covers 58 degrees: these clusters have cones (as c4's do).
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


@pytest.mark.parametrize("recipe, n_clusters, min_coned", [(CLUSTER_RECIPE, 126, 0), (CONE_RECIPE, 51, 40)], ids=["80x50", "8x200"])
@pytest.mark.parametrize("mname", ["rotation", "product"])
def test_cluster_records_are_conservative(api, mname, recipe, n_clusters, min_coned):
    """The records the pass builds on the device (k_clusters), read back: every cluster's box holds every posed corner
    of its 64 faces, and every face's unit normal lies in its cone.  No cluster is skipped."""
    matrix = pose_ref.matrices(api)[mname]
    other = pose_ref.twin(api, recipe, matrix)
    scene, index = pose_ref.build(api, recipe)
    backend = scene._backend()
    backend.render(scene, shadows=True)
    host_built = backend.read_clusters().copy()
    scene.models[index].pose = matrix
    backend.render(scene, shadows=True)
    assert backend.pose_counters()[:2] == (2, 1)
    rec = backend.read_clusters()
    corners, normals = _face_corners(other)
    n_faces = len(corners)
    assert len(rec) == n_clusters == len(host_built) == -(-n_faces // 64)
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
    assert coned >= min_coned, coned
    # the twin's records, built on the host, claim the same cones up to the summation order
    other._backend().render(other, shadows=True)
    want = other._backend().read_clusters()
    assert np.array_equal(rec["cos_half"] < -1, want["cos_half"] < -1)
    assert np.abs(rec["axis"] - want["axis"]).max() < 1e-6 and np.abs(rec["cos_half"] - want["cos_half"]).max() < 1e-6
    assert np.array_equal(rec["lo"], want["lo"]) and np.array_equal(rec["hi"], want["hi"])
    scene.close(), other.close()


def _uncounted(backend, scene, h, band=None):
    """A frame without the fragment counters -- a counted frame never culls clusters (host_frame.h, cluster_cull_mode)
    -- with its buffers kept: frame bytes, z, winner, stencil (of the band's rows, if any)."""
    out = backend.render(scene, shadows=True, counters=False, keep_buffers=True, row_band=band).copy()
    return [out] + _band_taps(backend, h, band or (0, h))


def _all_equal(got, want, label):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"{label}: {('frame', 'z', 'winner', 'stencil')[k]} differs"


@pytest.mark.parametrize("recipe, must_cull", [(CLUSTER_RECIPE, False), (CONE_RECIPE, True)], ids=["80x50", "8x200"])
def test_cluster_culling_with_device_built_records(api, monkeypatch, recipe, must_cull):
    """Culling by the device-built records changes nothing but the work: whole frame (forced on) and row band (on by
    default) equal the twin's un-culled ones, and the posed scene drops clusters wherever the twin, with host-built
    records, does.  (The clusters of the 80 x 50 torus reach most of the way round the tube and have no cones: whether
    any goes there is only printed; those of the 8 x 200 torus are patches, and there clusters must go.)"""
    matrix = pose_ref.matrices(api)["rotation"]
    other = pose_ref.twin(api, recipe, matrix)
    scene, index = pose_ref.build(api, recipe)
    backend = scene._backend()
    backend.render(scene, shadows=True)
    scene.models[index].pose = matrix
    h = scene.resolution[0]
    band = (h // 4, h // 2)
    monkeypatch.setenv("MR_CLUSTER_CULL", "0")
    want = _uncounted(other._backend(), other, h)
    want_band = _uncounted(other._backend(), other, h, band)
    assert other._backend().clusters_culled() == 0
    monkeypatch.setenv("MR_CLUSTER_CULL", "1")
    _all_equal(_uncounted(backend, scene, h), want, "MR_CLUSTER_CULL=1, whole frame")
    monkeypatch.delenv("MR_CLUSTER_CULL")
    _all_equal(_uncounted(backend, scene, h, band), want_band, "row band, culling on by default")
    assert np.array_equal(scene.render(row_band=band), want_band[0])
    monkeypatch.setenv("MR_CLUSTER_CULL", "count")
    counts = {}
    for label, sc in (("posed", scene), ("twin", other)):
        be = sc._backend()
        _all_equal(_uncounted(be, sc, h), want, f"MR_CLUSTER_CULL=count, {label}, whole frame")
        whole = be.clusters_culled()
        _all_equal(_uncounted(be, sc, h, band), want_band, f"MR_CLUSTER_CULL=count, {label}, rows {band}")
        counts[label] = (whole, be.clusters_culled())
    print(f"clusters culled (whole frame, rows {band}): posed {counts['posed']}, twin {counts['twin']}")
    for got, host in zip(counts["posed"], counts["twin"]):
        assert got >= 1 or host == 0, counts
    assert not must_cull or min(counts["twin"]) > 0, f"the twin culls nothing: the case proves nothing ({counts})"
    scene.close(), other.close()
