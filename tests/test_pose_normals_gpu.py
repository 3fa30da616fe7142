"""GPU: ``Model.pose_normals`` -- a posed model's vertex normals and object-space normal maps transformed by the pose
pass on the device (host_pose.h apply_pose_normals; kernels_pose.h k_pose_normals, k_pose_texels).

The yardstick is the twin (pose_normals_ref.py): the recipe built afresh with the posed model's vertices, normals and
object-space maps replaced by what the definition says.  Posed scene and twin hold bit-identical inputs, so everything
a caller can read of their frames on one device is compared for equality; the oracle's frame of the twin is held to the
project's standing bars (z / winner / stencil / silhouette / counts bit-exact, float frame 2e-6, uint8 +-1)."""
import functools

import numpy as np
import pytest

import pose_normals_ref as ref
import pose_ref
import scenes
from multilight_ref import extra_lights
from pose_ref import assert_same, counted

pytestmark = pytest.mark.gpu

CASES = [(name, m) for name in ref.RECIPES for m in ref.MATRIX_NAMES]


@functools.lru_cache(maxsize=None)
def _posed_and_twin(name, mname):
    """One recipe under one pose with ``pose_normals``: the frame with the attribute off, the frame with it on, the
    twin's frame (each ``counted``) and the twin."""
    api = scenes.product_api()
    matrix = pose_ref.matrices(api)[mname]
    scene, index = ref.build(api, name)
    backend = scene._backend()
    scene.models[index].pose = matrix
    without = counted(backend, scene)
    scene.models[index].pose_normals = True
    posed = counted(backend, scene)
    scene.close()
    other = ref.twin(api, name, matrix)
    want = counted(other._backend(), other)
    other.close()
    return without, posed, want, other


# ---------------------------------------------------------------------------- 1. posed equals twin, exactly
@pytest.mark.parametrize("name, mname", CASES)
def test_posed_equals_twin(name, mname):
    """Frame bytes, z bits, winner, stencil, silhouette set, float frame and every counter of ``mr_stats`` are the
    twin's.  The attribute changed the shading and nothing else -- but on tetra_bare, which has neither normals nor an
    object-space map: there the frame is the one without it."""
    without, posed, want, _ = _posed_and_twin(name, mname)
    assert_same(posed, want, f"{name} under {mname}")
    for key in ("z", "winner", "stencil0", "silhouette0"):
        assert np.array_equal(posed[key], without[key]), f"{name} under {mname}: {key} follows the pose, not the normals"
    if name == "tetra_bare":
        assert_same(posed, without, f"{name} under {mname}: nothing to transform")
    else:
        assert not np.array_equal(posed["frame"], without["frame"]), f"{name} under {mname}: pose_normals changed nothing"


@pytest.mark.parametrize("name", ["diablo_floor", "diablo_nm_object"])
def test_a_translation_leaves_the_shading_alone(api, name):
    """G = I: the normals and texels the pass writes are the model's own (a component that is -0.0 comes out as +0.0,
    which no frame shows), so the frame with ``pose_normals`` is the frame without it, and the twin's."""
    matrix = pose_ref.matrices(api)["translation"]
    other = ref.twin(api, name, matrix)
    want = counted(other._backend(), other)
    other.close()
    scene, index = ref.build(api, name)
    backend = scene._backend()
    scene.models[index].pose = matrix
    without = counted(backend, scene)
    scene.models[index].pose_normals = True
    posed = counted(backend, scene)
    assert backend.pose_counters()[1] == 2                         # the attribute alone ran a pass
    assert_same(posed, without, f"{name}: pose_normals under a translation")
    assert_same(posed, want, f"{name} under the translation")
    times = backend.pose_normals_times()
    assert times["pose_normals"] > 0 and (times["pose_texels"] > 0) == (name == "diablo_nm_object"), times
    scene.close()


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


# ---------------------------------------------------------------------------- 3. state changes on one scene
@pytest.mark.parametrize("name", ["diablo_nm_object", "diablo_floor"])
def test_state_changes_on_one_scene(api, name):
    """rotation with normals -> the attribute off (today's posed frame) -> on again -> ``pose = None`` (the first frame)
    -> a new pose, each frame its twin's.  diablo is a float32 model: posing it and letting go of it cost a commit each
    (its faces lose and regain FF_VERTS_F32), and nothing else does; a change of the attribute alone is a pass that
    writes no vertex."""
    m = pose_ref.matrices(api)
    want = {}
    for key, other in (("rotation, on", ref.twin(api, name, m["rotation"])), ("rotation, off", pose_ref.twin(api, ref.RECIPES[name], m["rotation"])),
                       ("product, on", ref.twin(api, name, m["product"]))):
        want[key] = counted(other._backend(), other)
        other.close()
    scene, index = ref.build(api, name)
    backend = scene._backend()
    model = scene.models[index]
    first = counted(backend, scene)
    assert backend.pose_counters()[:3] == (1, 0, 0)
    model.pose_normals = True
    assert_same(counted(backend, scene), first, "the attribute without a pose")
    assert backend.pose_counters()[:3] == (1, 0, 0)
    model.pose = m["rotation"]
    assert_same(counted(backend, scene), want["rotation, on"], "rotation, on")
    assert backend.pose_counters() == (2, 1, 1, len(model.vertices))
    model.pose_normals = False
    assert_same(counted(backend, scene), want["rotation, off"], "rotation, off")
    assert backend.pose_counters() == (2, 2, 1, 0)
    model.pose_normals = True
    assert_same(counted(backend, scene), want["rotation, on"], "rotation, on again")
    assert backend.pose_counters() == (2, 3, 1, 0)
    model.pose = None
    assert_same(counted(backend, scene), first, "pose = None")
    assert backend.pose_counters()[:3] == (3, 3, 0)
    model.pose = m["product"]
    assert_same(counted(backend, scene), want["product, on"], "product, on")
    assert backend.pose_counters() == (4, 4, 1, len(model.vertices))
    times = backend.pose_normals_times()
    assert set(times) == {"pose_normals", "pose_texels"} and all(0 <= v < 100 for v in times.values()), times
    assert set(backend.pose_times()) == set(backend.POSE_TIME_NAMES)
    scene.close()


# ---------------------------------------------------------------------------- 4. two models, one object-space map
def test_two_models_share_one_map(api):
    """Two quads whose materials hold one texture array, posed differently, first one with ``pose_normals``, then the
    other, then both: each model samples its own re-baked copy or the original, as its twin does.  The second quad is a
    float64 model: nothing but its first pose costs a commit (the first quad's float32 flip)."""
    m = pose_ref.matrices(api)
    poses = {0: m["rotation"], 1: m["mirror"]}
    want = {}
    for which in ((0,), (1,), (0, 1), ()):
        other = ref.twin(api, ref.TWO_QUADS, poses, normals=which)
        want[which] = counted(other._backend(), other)
        other.close()
    assert not np.array_equal(want[(0,)]["frame"], want[(1,)]["frame"]) and not np.array_equal(want[(0, 1)]["frame"], want[()]["frame"])
    scene, _ = ref.build(api, ref.TWO_QUADS)
    backend = scene._backend()
    backend.render(scene, shadows=True)
    for k, matrix in poses.items():
        scene.models[k].pose = matrix
    for which in ((0,), (1,), (0, 1), (0,), (), (1,)):
        for k in (0, 1):
            scene.models[k].pose_normals = k in which
        assert_same(counted(backend, scene), want[which], f"pose_normals on {which}")
    assert backend.pose_counters()[0] == 2
    scene.close()


# ---------------------------------------------------------------------------- 5. table boundaries
def test_two_posed_models_in_one_pass(api):
    """diablo (2 519 normals: nine workgroups and part of a tenth) and the cube (fewer normals than one workgroup has
    threads) posed in one pass with different matrices: the workgroup -> row table and the range guards."""
    m = pose_ref.matrices(api)
    poses = {0: m["rotation"], 1: m["product"]}
    other = ref.twin(api, ref.SMALL_AND_LARGE, poses)
    want = counted(other._backend(), other)
    counts = [len(model.normals) for model in other.models[:2]]
    assert counts[0] % 256 != 0 and counts[0] > 256 > counts[1] > 0, counts
    other.close()
    scene, _ = ref.build(api, ref.SMALL_AND_LARGE)
    backend = scene._backend()
    plain = counted(backend, scene)
    for k, matrix in poses.items():
        ref.pose(scene.models[k], matrix)
    assert_same(counted(backend, scene), want, "two posed models")
    assert backend.pose_counters()[1:3] == (1, 2)
    scene.models[1].pose = None                      # the cube lets go: its normals come back, diablo's stay
    ref.pose(scene.models[0], m["mirror"])
    other = ref.twin(api, ref.SMALL_AND_LARGE, {0: m["mirror"]})
    assert_same(counted(backend, scene), counted(other._backend(), other), "one posed model")
    other.close()
    for model in scene.models[:2]:
        model.pose = None
    assert_same(counted(backend, scene), plain, "pose = None")
    scene.close()


# ---------------------------------------------------------------------------- 6. the other frame kinds
def _pair(api, name, mname="product", prepare=lambda scene: None):
    matrix = pose_ref.matrices(api)[mname]
    other = ref.twin(api, name, matrix)          # (first: a new Material anywhere makes every scene upload its models again)
    prepare(other)
    scene, index = ref.build(api, name)
    prepare(scene)
    scene._backend().render(scene, shadows=True)                   # (un-posed first: pose and matrix arrive between frames)
    ref.pose(scene.models[index], matrix)
    return scene, other


def test_supersampled(api):
    def prepare(scene):
        scene.supersample = 2
    scene, other = _pair(api, "diablo_nm_object", prepare=prepare)
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


def test_row_band(api):
    scene, other = _pair(api, "diablo_nm_object", "rotation")
    h = scene.resolution[0]
    whole = other.render().copy()
    for band in ((0, 64), (48, 112), (112, h)):
        got = scene._backend().render(scene, shadows=True, counters=False, keep_buffers=True, row_band=band).copy()
        want = other._backend().render(other, shadows=True, counters=False, keep_buffers=True, row_band=band).copy()
        assert np.array_equal(got, want) and np.array_equal(got, whole[band[0]:band[1]]), band
        assert np.array_equal(scene._backend().render(scene, shadows=True, row_band=band), want), band     # counted
    scene.close(), other.close()


def test_render_async_and_render_frames_with_a_new_rotation_each_frame(api):
    """Eight frames two deep, a new rotation in front of each (``render_async``, then ``render_frames``): the pass
    drains the frames in flight, and every frame is its twin's synchronous one."""
    want = []
    for i in range(1, 9):
        other = ref.twin(api, "diablo_floor", pose_ref.turn(api, 3.0 * i))
        want.append(other.render().copy())
        other.close()
    scene, index = ref.build(api, "diablo_floor")
    model = scene.models[index]
    model.pose_normals = True
    scene.render()
    queue, got = [], []
    for i in range(1, 9):
        model.pose = pose_ref.turn(api, 3.0 * i)
        queue.append(scene.render_async())
        if len(queue) >= 2:
            got.append(queue.pop(0).result().copy())
    got += [p.result().copy() for p in queue]
    assert scene._backend().pose_counters()[1] == 8

    def views():
        for i in range(8, 0, -1):
            model.pose = pose_ref.turn(api, 3.0 * i)
            yield scene.camera, scene.debug_camera
    again = [frame.copy() for frame in scene.render_frames(views(), depth=2)]
    scene.close()
    for i in range(8):
        assert np.array_equal(got[i], want[i]), f"render_async, frame {i + 1}"
        assert np.array_equal(again[7 - i], want[i]), f"render_frames, frame {i + 1}"
